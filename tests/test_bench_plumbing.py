"""CPU: bench.py's MIOpen find-db seeding (plumbing; no GPU, MIOpen is never initialised here), its argument checks
and its --dump-outputs writer."""
import importlib
import os
import stat
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_seed_miopen_db_copies_the_shipped_db_to_a_private_scratch_dir(tmp_path, monkeypatch):
    bench = _bench()
    src = os.path.join(ROOT, "wssdl_bus_amd", "miopen_db", "config")
    assert os.path.isdir(src) and any(f.endswith(".ufdb.txt") for f in os.listdir(src))
    monkeypatch.delenv("MIOPEN_USER_DB_PATH", raising=False)
    monkeypatch.delenv("MIOPEN_CUSTOM_CACHE_DIR", raising=False)
    monkeypatch.setenv("TMPDIR", str(tmp_path))
    import tempfile
    tempfile.tempdir = None                                     # re-read TMPDIR
    try:
        dst, note = bench.seed_miopen_db()
        assert dst and dst.startswith(str(tmp_path)) and "miopen_db" in note
        assert stat.S_IMODE(os.stat(dst).st_mode) == 0o700          # mkdtemp: private, unpredictable name
        assert os.environ["MIOPEN_USER_DB_PATH"] == os.path.join(dst, "config")
        assert sorted(os.listdir(os.environ["MIOPEN_USER_DB_PATH"])) == sorted(os.listdir(src))
        assert os.path.isdir(os.environ["MIOPEN_CUSTOM_CACHE_DIR"])
        assert bench.miopen_db_grew(dst) is False
        with open(os.path.join(dst, "config", os.listdir(src)[0]), "a") as fh:
            fh.write("x")                                           # what a search would do
        assert bench.miopen_db_grew(dst) is True
        # two calls never share a directory
        monkeypatch.delenv("MIOPEN_USER_DB_PATH")
        monkeypatch.delenv("MIOPEN_CUSTOM_CACHE_DIR")
        dst2, _ = bench.seed_miopen_db()
        assert dst2 and dst2 != dst
        # a caller that already points MIOpen somewhere is left alone
        monkeypatch.setenv("MIOPEN_USER_DB_PATH", "/somewhere/else")
        assert bench.seed_miopen_db()[0] is None and os.environ["MIOPEN_USER_DB_PATH"] == "/somewhere/else"
    finally:
        tempfile.tempdir = None


def test_seed_miopen_db_fails_closed_on_another_miopen_build(tmp_path, monkeypatch):
    """A find-db written by another MIOpen build would be ignored by MIOpen, which would then search for
    minutes on every rank: the seeding refuses and bench.py falls back to the heuristic solver choice."""
    bench = _bench()
    monkeypatch.delenv("MIOPEN_USER_DB_PATH", raising=False)
    monkeypatch.delenv("MIOPEN_CUSTOM_CACHE_DIR", raising=False)
    fake = tmp_path / "repo"
    cfgdir = fake / "wssdl_bus_amd" / "miopen_db" / "config"
    cfgdir.mkdir(parents=True)
    (cfgdir / "gfx950100.HIP.9_9_9_19990101-1-1-gdeadbeef00.ufdb.txt").write_text("")
    monkeypatch.setattr(bench, "ROOT", str(fake))
    dst, note = bench.seed_miopen_db()
    assert dst is None and "9_9_9" in note
    assert "MIOPEN_USER_DB_PATH" not in os.environ


def _bench_cli(*argv):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_bench_refuses_arguments_it_cannot_honour_before_touching_the_gpu():
    """--steps sets the number of timed steps, so zero is refused; --save-fixed-rois saves the roofline leg's RoI set,
    which only a --full run builds.  Both fail at argument parsing (exit 2), before torch is imported."""
    p = _bench_cli("--steps", "0")
    assert p.returncode == 2 and b"--steps" in p.stderr and not p.stdout.strip()
    p = _bench_cli("--save-fixed-rois", "rois.npy", "--steps", "1")
    assert p.returncode == 2 and b"--full" in p.stderr and not p.stdout.strip()
    assert not os.path.exists(os.path.join(ROOT, "rois.npy"))


def test_dump_outputs_writes_what_the_step_returned(tmp_path):
    import torch
    bench = _bench()
    out = dict(loss=torch.tensor(1.25), rpn_loss_box=torch.tensor(0.5, dtype=torch.float64),
               mil_cross_entropy=torch.tensor(0.75, dtype=torch.float16))
    bench.dump_outputs(str(tmp_path / "a"), out)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["loss.npy", "rpn_loss_box.npy", "mil_cross_entropy.npy"])
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert got["loss"].dtype == np.float32 and got["loss"] == 1.25
    assert got["rpn_loss_box"].dtype == np.float64 and got["mil_cross_entropy"].dtype == np.float32
    # the test forward returns per-class detections
    bench.dump_outputs(str(tmp_path / "c"), {1: np.ones((3, 5), np.float32), 2: torch.zeros((0, 5))})
    assert sorted(os.listdir(tmp_path / "c")) == ["dets_class1.npy", "dets_class2.npy"]
    assert np.load(tmp_path / "c" / "dets_class1.npy").shape == (3, 5)
    assert np.load(tmp_path / "c" / "dets_class2.npy").shape == (0, 5)


def test_seed_miopen_db_gives_miopen_writable_copies_of_a_read_only_checkout(tmp_path, monkeypatch):
    """MIOpen writes to both shipped databases (find results, kernels, sqlite's journal beside the kernel cache): a copy
    that kept a read-only checkout's mode bits made its first convolution fail (`attempt to write a readonly database`,
    miopenStatusInternalError).  The scratch copy is owner-writable whatever the modes of the source."""
    import shutil
    bench = _bench()
    monkeypatch.delenv("MIOPEN_USER_DB_PATH", raising=False)
    monkeypatch.delenv("MIOPEN_CUSTOM_CACHE_DIR", raising=False)
    fake = tmp_path / "repo"
    shutil.copytree(os.path.join(ROOT, "wssdl_bus_amd", "miopen_db"), str(fake / "wssdl_bus_amd" / "miopen_db"))
    ro = [str(p) for p in (fake / "wssdl_bus_amd" / "miopen_db").rglob("*")] + [str(fake / "wssdl_bus_amd" / "miopen_db")]
    for p in ro:
        os.chmod(p, 0o555 if os.path.isdir(p) else 0o444)
    monkeypatch.setattr(bench, "ROOT", str(fake))
    try:
        dst, note = bench.seed_miopen_db()
        assert dst and "miopen_db" in note
        seen = 0
        for r, ds, fs in os.walk(dst):
            for x in ds + fs:
                mode = stat.S_IMODE(os.stat(os.path.join(r, x)).st_mode)
                assert mode & 0o600 == 0o600 and (mode & 0o100 or not os.path.isdir(os.path.join(r, x))), (x, oct(mode))
                seen += 1
        assert seen == len(ro) - 1                                  # config/, cache/ and every file in them
        assert bench.miopen_db_grew(dst) is False
    finally:
        for p in ro:
            os.chmod(p, 0o755 if os.path.isdir(p) else 0o644)
