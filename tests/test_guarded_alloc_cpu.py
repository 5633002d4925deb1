"""The guard-band and poison harness of tests/guarded_alloc.py, proved on CPU tensors against
fake ops with seeded defects: each defect must be reported, with the right call site, and a
clean op must pass all four poisons.  No kernel is involved."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

import guarded_alloc as ga
from guarded_alloc import GUARD, POISONS, guarded, run_case

CPU = ("cpu",)
N = 37                      # f32 elements: 148 bytes, no multiple of 256 or of 64


def _line_of(fn, marker):
    """Line number of the line of `fn` that carries the comment `# <marker>`."""
    src, first = inspect.getsourcelines(fn)
    hits = [first + i for i, l in enumerate(src) if l.rstrip().endswith("# " + marker)]
    assert len(hits) == 1, (marker, hits)
    return hits[0]


def _poke(t, byte_offset, value=0x11):
    """One byte written relative to the tensor's first byte, the way a kernel with a wrong
    index would: through the raw address, not through the view.  Under the plain allocator the
    write is left out: on the device it would land in the caching allocator's slack, unseen; here
    the neighbours of a small CPU tensor are malloc's own headers."""
    if t.untyped_storage().nbytes() >= t.numel() * t.element_size() + 2 * GUARD:
        ctypes.memset(t.data_ptr() + byte_offset, value, 1)


def _inputs():
    g = torch.Generator().manual_seed(5)
    return {"x": torch.randn(N, generator=g)}


# ---- fake ops --------------------------------------------------------------------------
def clean_op(inp):
    ws = torch.empty((N,), dtype=torch.float32)          # ALLOC-WS
    out = torch.empty_like(inp["x"])                     # ALLOC-OUT
    cnt = torch.zeros((1,), dtype=torch.int32)
    extra = inp["x"].new_empty((3, 5))
    ws.copy_(inp["x"] * 2)
    out.copy_(ws + 1)
    cnt += N
    extra.fill_(2.5)
    return out, cnt, extra


def make_overrun_op(offset_of):
    def op(inp):
        ws = torch.empty((N,), dtype=torch.float32)      # ALLOC-WS
        out = torch.empty((N,), dtype=torch.float32)     # ALLOC-OUT
        ws.copy_(inp["x"])
        out.copy_(ws)
        _poke(ws, offset_of(ws))
        return out
    return op


def stale_read_op(inp):
    ws = torch.empty((N,), dtype=torch.float32)          # ALLOC-WS
    out = torch.empty((N,), dtype=torch.float32)
    out.copy_(inp["x"] + ws.view(torch.int32).to(torch.float32))       # reads ws before writing it
    return out


def fmax_stale_op(inp):
    stale = torch.empty((N,), dtype=torch.float32)       # ALLOC-WS
    out = torch.empty((N,), dtype=torch.float32)
    out.copy_(torch.fmax(inp["x"], stale))               # fmax ignores NaN, like v_max_f32
    return out


def unwritten_tail_op(inp):
    out = torch.empty((N,), dtype=torch.float32)         # ALLOC-OUT
    out[:N - 1].copy_(inp["x"][:N - 1])
    return out


def scribble_op(inp):
    out = torch.empty((N,), dtype=torch.float32)
    out.copy_(inp["x"])
    inp["x"][3] = 7.0
    return out


def no_alloc_op(inp):
    return inp["x"] * 2


# ---- the allocator ---------------------------------------------------------------------
def test_guarded_layout_and_poison():
    with guarded(0xFF, CPU) as reg:
        t = torch.empty((N,), dtype=torch.float32)
        d = torch.empty(2, 3, dtype=torch.float64)
        z = torch.zeros((5,), dtype=torch.int32)
        e = torch.empty_like(t)
        n = t.new_empty((4,), dtype=torch.int64)
    assert reg.count() == 5
    assert reg.guarded_bytes() == 4 * N + 48 + 20 + 4 * N + 32
    r = reg.records[0]
    assert r.buf.numel() == GUARD + 4 * N + GUARD and r.nbytes == 4 * N
    assert t.data_ptr() == r.buf.data_ptr() + GUARD              # the view starts at GUARD ...
    assert t.shape == (N,) and t.is_contiguous()
    assert t.untyped_storage().nbytes() == r.buf.numel()
    assert int(r.buf[GUARD + 4 * N]) == 0xA5                      # ... and the next byte after it is guard
    assert bool((r.buf[:GUARD] == 0xA5).all()) and bool((r.buf[GUARD + 4 * N:] == 0xA5).all())
    assert bool(torch.isnan(t).all()) and bool(torch.isnan(d).all()) and d.shape == (2, 3)
    assert bool((z == 0).all()) and bool((n == -1).all()) and bool(torch.isnan(e).all())
    reg.check()
    assert torch.empty is reg._orig["empty"] and torch.zeros is reg._orig["zeros"]
    assert torch.empty_like is reg._orig["empty_like"] and torch.Tensor.new_empty is reg._orig["new_empty"]


def test_finite_poisons_are_the_documented_values():
    with guarded(0x7F, CPU):
        a = torch.empty((2,), dtype=torch.float32)
    with guarded(0xFE, CPU):
        b = torch.empty((2,), dtype=torch.float32)
    assert a.view(torch.int32).tolist() == [0x7F7F7F7F] * 2 and 3.39e38 < float(a[0]) < 3.40e38
    assert -1.70e38 < float(b[0]) < -1.69e38
    assert POISONS == (0x00, 0xFF, 0x7F, 0xFE)


def test_passed_through_unguarded():
    with guarded(0xFF, CPU) as reg:
        m = torch.empty((8,), device="meta")
        z = torch.empty((0, 4))
        f = torch.empty((1, 3, 4, 4), memory_format=torch.channels_last)
        o = torch.empty((3,), out=torch.ones(3))
    assert reg.count() == 0 and reg.passed_through == 4
    assert m.device.type == "meta" and z.numel() == 0 and f.shape == (1, 3, 4, 4) and o.shape == (3,)
    with guarded(0xFF) as reg:                  # the product default guards CUDA only
        c = torch.empty((8,))
    assert reg.count() == 0 and c.untyped_storage().nbytes() == 32


def test_restored_after_an_exception():
    orig = (torch.empty, torch.zeros, torch.empty_like, torch.Tensor.new_empty)
    with pytest.raises(RuntimeError):
        with guarded(0x00, CPU):
            raise RuntimeError("boom")
    assert (torch.empty, torch.zeros, torch.empty_like, torch.Tensor.new_empty) == orig


# ---- seeded defects --------------------------------------------------------------------
@pytest.mark.parametrize("where,offset_of,side", [
    ("byte -1", lambda t: -1, "before"),
    ("byte nbytes", lambda t: t.numel() * 4, "after"),
    ("byte nbytes+GUARD-1", lambda t: t.numel() * 4 + GUARD - 1, "after"),
])
def test_overrun_is_reported_with_site_side_and_offsets(where, offset_of, side):
    op = make_overrun_op(offset_of)
    with guarded(0x00, CPU) as reg:
        op(_inputs())
    v = reg.violations()
    line = _line_of(make_overrun_op, "ALLOC-WS")
    assert len(v) == 1, v
    site, got_side, lo, hi, nbytes = v[0]
    assert nbytes == 4 * N
    assert site.endswith("test_guarded_alloc_cpu.py:%d" % line), (site, line)
    assert got_side == side and lo == hi == offset_of(torch.empty(N))
    with pytest.raises(ga.GuardViolation) as e:
        reg.check()
    assert "test_guarded_alloc_cpu.py:%d" % line in str(e.value) and side in str(e.value)
    with pytest.raises(AssertionError) as e:
        run_case(op, _inputs(), name=where, devices=CPU)
    assert "test_guarded_alloc_cpu.py:%d" % line in str(e.value) and "guard " + side in str(e.value)


def test_two_sided_overrun_reports_lowest_and_highest():
    def op(inp):
        ws = torch.empty((N,), dtype=torch.float32)
        ws.zero_()
        for off in (-300, -7, 4 * N + 2, 4 * N + 511):
            _poke(ws, off)
        return ws
    with guarded(0xFF, CPU) as reg:
        op(None)
    assert [v[1:] for v in reg.violations()] == [("before", -300, -7, 4 * N), ("after", 4 * N + 2, 4 * N + 511, 4 * N)]


def test_one_call_site_with_several_sizes_names_the_size_that_was_hit():
    def op(inp):
        bufs = [torch.empty((n,), dtype=torch.uint8) for n in (5, 300, 77)]            # one site, three sizes
        _poke(bufs[1], 300)
        return bufs
    with guarded(0x00, CPU) as reg:
        op(None)
    assert [v[1:] for v in reg.violations()] == [("after", 300, 300, 300)]
    with pytest.raises(ga.GuardViolation) as e:
        reg.check()
    assert "the 300-byte allocation" in str(e.value)


def test_workspace_read_before_write_changes_with_the_poison():
    with pytest.raises(AssertionError) as e:
        run_case(stale_read_op, _inputs(), name="stale", devices=CPU, poisons=(0xFF,))
    msg = str(e.value)
    assert "depends on what the allocations held" in msg
    assert "test_guarded_alloc_cpu.py:%d" % _line_of(stale_read_op, "ALLOC-WS") in msg


def test_nan_blind_max_passes_nan_poison_and_is_caught_by_0x7f():
    inp = _inputs()
    want = inp["x"].clone()                                     # max over the inputs alone
    with guarded(0xFF, CPU):
        got = fmax_stale_op(inp)
    assert not ga.bit_differences(want, got)                    # NaN poison alone passes the bug
    with guarded(0x7F, CPU):
        got = fmax_stale_op(inp)
    d = ga.bit_differences(want, got)
    assert d and "bytes differ" in d[0]                         # +3.39e38 wins every max
    assert bool((got == got[0]).all()) and float(got[0]) > 3.39e38


def test_run_case_catches_the_nan_blind_max():
    with pytest.raises(AssertionError) as e:
        run_case(fmax_stale_op, _inputs(), name="fmax", devices=CPU, poisons=(0x7F,))
    assert "test_guarded_alloc_cpu.py:%d" % _line_of(fmax_stale_op, "ALLOC-WS") in str(e.value)


def test_unwritten_last_element():
    with pytest.raises(AssertionError) as e:
        run_case(unwritten_tail_op, _inputs(), name="tail", devices=CPU, poisons=(0xFF,))
    msg = str(e.value)
    assert "first at byte %d" % (4 * (N - 1)) in msg and "last at byte %d" % (4 * N - 1) in msg
    assert "test_guarded_alloc_cpu.py:%d" % _line_of(unwritten_tail_op, "ALLOC-OUT") in msg


def test_unwritten_last_element_can_be_declared_undefined():
    run_case(unwritten_tail_op, _inputs(), name="tail", devices=CPU, defined=lambda out: out[:N - 1])


def test_scribble_on_an_input():
    with pytest.raises(AssertionError) as e:
        run_case(scribble_op, _inputs(), name="scribble", devices=CPU)
    assert "wrote to an input" in str(e.value) and "'x'" in str(e.value)
    run_case(scribble_op, _inputs(), name="scribble", devices=CPU, inplace=("x",))


def test_case_that_allocates_nothing_fails_the_floor():
    with pytest.raises(AssertionError) as e:
        run_case(no_alloc_op, _inputs(), name="vacuous", devices=CPU)
    assert "0 allocations guarded, the case declares at least 1" in str(e.value)
    with pytest.raises(AssertionError):
        run_case(unwritten_tail_op, _inputs(), name="floor2", devices=CPU, min_allocations=2,
                 defined=lambda out: out[:N - 1])
    with pytest.raises(AssertionError):
        run_case(clean_op, _inputs(), name="floor0", devices=CPU, min_allocations=0)


def test_raised_flag_fails_the_case():
    with pytest.raises(AssertionError) as e:
        run_case(clean_op, _inputs(), name="flag", devices=CPU, flags_raised=lambda: True)
    assert "flag was raised" in str(e.value)


# ---- clean op --------------------------------------------------------------------------
def test_clean_op_passes_all_four_poisons(capsys):
    totals = {}
    base = run_case(clean_op, _inputs(), name="clean", devices=CPU, min_allocations=4,
                    flags_raised=lambda: False, totals=totals)
    assert torch.equal(base[0], _inputs()["x"] * 2 + 1)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("memcheck clean")]
    assert len(lines) == 4
    for l, p in zip(lines, POISONS):
        assert re.match(r"memcheck clean poison=0x%02X allocations=4 guarded_bytes=%d ok$"
                        % (p, 4 * N + 4 * N + 4 + 60), l), l
    assert totals == {"allocations": 16, "guarded_bytes": 4 * (8 * N + 64), "runs": 4}


def test_nan_results_compare_equal_bitwise():
    def op(inp):
        out = torch.empty((N,), dtype=torch.float32)
        out.copy_(inp["x"])
        out[2] = float("nan")
        return {"out": out, "n": 3, "np": out.numpy().copy(), "f": float("nan")}
    run_case(op, _inputs(), name="nan", devices=CPU)


# ---- autograd ---------------------------------------------------------------------------
class _Scale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        out = torch.empty_like(x)
        arg = torch.empty((x.numel(),), dtype=torch.float64)
        out.copy_(x * w)
        arg.copy_(x.double().reshape(-1))
        ctx.save_for_backward(x, w, arg)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, arg = ctx.saved_tensors
        gx = torch.empty_like(g)
        gw = torch.zeros((1,), dtype=g.dtype)
        gx.copy_(g * w)
        gw += (g.double().reshape(-1) * arg).sum().to(g.dtype)
        return gx, gw


def test_autograd_function_on_guarded_tensors_back_propagates():
    g = torch.Generator().manual_seed(9)
    x0, w0 = torch.randn(5, 7, generator=g), torch.tensor([1.5])

    def op(inp):
        x = inp["x"].clone().requires_grad_(True)
        w = inp["w"].clone().requires_grad_(True)
        y = _Scale.apply(x, w)
        (y * y).sum().backward()
        return y.detach(), x.grad, w.grad

    y, gx, gw = run_case(op, {"x": x0, "w": w0}, name="autograd", devices=CPU, min_allocations=4)
    assert torch.allclose(y, x0 * 1.5)
    assert torch.allclose(gx, 2 * x0 * 1.5 * 1.5)
    assert torch.allclose(gw, (2 * x0 * 1.5 * x0).sum().reshape(1))
    with guarded(0xFF, CPU) as reg:
        fresh = torch.empty((3,), dtype=torch.float64)
    assert bool(torch.isnan(fresh).all()) and reg.count() == 1
