"""CPU: RoIAlign without a GPU -- the reference of tests/roi_align_reference.py against itself, the declared C surface,
the argument validation of the exports (nothing is launched), the cfg keys and the layer's dispatch, the snapshot's record
of the pooling mode."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import roi_align_reference as ref
from wssdl_bus_amd.fast_rcnn.config import cfg, cfg_from_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("wssdl_roi_align_tables_bytes", "wssdl_roi_align_tables", "wssdl_roi_align_forward",
           "wssdl_roi_align_backward_workspace_bytes", "wssdl_roi_align_backward_prepare", "wssdl_roi_align_backward")


@pytest.fixture
def pool_cfg():
    """cfg's three RoI pooling keys, put back afterwards."""
    old = cfg.ROI_POOL_MODE, cfg.ROI_ALIGN_SAMPLING, cfg.ROI_ALIGN_ALIGNED
    yield cfg
    cfg.ROI_POOL_MODE, cfg.ROI_ALIGN_SAMPLING, cfg.ROI_ALIGN_ALIGNED = old


# ------------------------------------------------------------------------------------- the reference against itself ---
def _dyadic_rois():
    """RoIs whose geometry is exact in f32 at scale 1/16 with 4 x 4 bins and S = 2: starts k + 0.5 cells, lengths 4 or 8 cells."""
    return np.array([[0, 24, 40, 24 + 128, 40 + 64], [1, 56, 24, 56 + 64, 24 + 128], [0, 8, 8, 8 + 64, 8 + 64]], np.float32)


def test_constant_map_gives_the_constant_for_interior_rois():
    c = ref.make_case('mixed')
    N, H, W, C = c['shape']
    data = np.full((N, H, W, 2), 3.25, np.float32)
    interior = c['rois'][[i for i in range(41) if i not in c['rows'].values()]]
    for aligned in (False, True):
        for S in (1, 2, 3):
            t = ref.tables(interior, N, H, W, 7, 7, c['scale'], S, aligned)
            top, _ = ref.forward(data, t, S)
            # the f32 tables are taken as given: h = 1.0f - l is one rounding (<= 2^-25) away from 1 - l, per axis
            assert np.abs(top - 3.25).max() <= 3.25 * 2 * 2.0 ** -25 * (1 + 1e-6)


def test_linear_ramp_gives_the_value_at_each_bin_centre():
    N, H, W = 2, 13, 19
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    data = np.stack([0.5 * hh - 0.25 * ww + 2.0, 0.125 * hh + 1.5 * ww - 3.0], axis=-1)[None].repeat(N, 0).astype(np.float32)
    rois, P, S = _dyadic_rois(), 4, 2
    t = ref.tables(rois, N, H, W, P, P, 1.0 / 16, S, True)
    top, _ = ref.forward(data, t, S)
    for r, (_, x1, y1, x2, y2) in enumerate(rois.astype(np.float64)):
        ys = (y1 / 16 - 0.5) + (np.arange(P) + 0.5) * ((y2 - y1) / 16 / P)
        xs = (x1 / 16 - 0.5) + (np.arange(P) + 0.5) * ((x2 - x1) / 16 / P)
        want = np.stack([0.5 * ys[:, None] - 0.25 * xs[None, :] + 2.0, 0.125 * ys[:, None] + 1.5 * xs[None, :] - 3.0], axis=-1)
        assert np.abs(top[r] - want).max() <= 1e-12


@pytest.mark.parametrize("aligned", [False, True])
def test_direct_form_equals_separable_form_on_mixed(aligned):
    c = ref.make_case('mixed')
    for S in (1, 2, 3):
        t = ref.tables(c['rois'], *c['shape'][:3], c['PH'], c['PW'], c['scale'], S, aligned)
        top, _ = ref.forward(c['data'], t, S)
        assert np.abs(top - ref.forward_separable(c['data'], t, S)).max() <= 1e-12


@pytest.mark.parametrize("aligned", [False, True])
def test_adjoint_identity(aligned):
    c = ref.make_case('mixed')
    r = ref.reference('mixed', 2, aligned)
    g, x = c['grad'].astype(np.float64), c['data'].astype(np.float64)
    lhs, rhs = (r['top'] * g).sum(), (x * r['diff']).sum()
    assert abs(lhs - rhs) <= 1e-12 * np.abs(r['top'] * g).sum()
    # a box listed twice counts twice: the twins' rows have the same tables, and both rows' gradients are in the adjoint
    a, b = c['rows']['twin_a'], c['rows']['twin_b']
    assert a != b and np.array_equal(r['top'][a], r['top'][b])


def test_case_mixed_holds_what_it_promises():
    c = ref.make_case('mixed')
    rois, rows = c['rois'], c['rows']
    assert rois.shape == (41, 5) and c['shape'] == (3, 13, 19, 160)
    live = ref.live_rows(rois, 3)
    assert not live[[rows['pad'], rows['beyond'], rows['nan'], rows['inf']]].any()
    idx = rois[live, 0]
    assert set(idx.tolist()) == {0.0, 1.0} and (np.diff(idx) < 0).any()          # interleaved; image 2 has no live RoI
    for aligned in (False, True):
        t = ref.tables(rois, 3, 13, 19, 7, 7, c['scale'], 2, aligned)
        w = t['yh'] + t['yl']
        assert not w[rows['void']].any() and not (t['xh'] + t['xl'])[rows['void']].any()
        assert (t['win'][~live, 0] == -1).all() and not w[~live].any()
        for k in ('ylo', 'yhi'):
            assert t[k].min() >= 0 and t[k].max() <= 12
        for k in ('xlo', 'xhi'):
            assert t[k].min() >= 0 and t[k].max() <= 18
    assert rois[rows['flipped'], 3] < rois[rows['flipped'], 1]
    assert (rois[rows['tiny'], 3] - rois[rows['tiny'], 1]) * c['scale'] < 1


# --------------------------------------------------------------------------------------------------- the C surface ---
def test_header_and_ctypes_table_declare_the_exports():
    from wssdl_bus_amd import _lib
    text = open(os.path.join(ROOT, "include", "wssdl_bus_hip.h")).read()
    declared = set(re.findall(r"WSSDL_API[^;(]*?\b(wssdl_\w+)\s*\(", text))
    for name in EXPORTS:
        assert name in declared and name in _lib.SYMBOLS, name


@pytest.fixture(scope="module")
def L():
    from wssdl_bus_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    yield lib
    # the exports clear the thread's last error on entry: leave it clear for whoever looks next
    assert lib.wssdl_roi_align_tables(None, 0, 1, 1, 1, 7, 7, 1.0, 2, 1, None, 0, None) == 0
    assert lib.wssdl_last_error() == b""


class _Args(object):
    """A valid call of each export (R = 5 on a 2 x 6 x 9 x 8 map); the 'device' pointers are host arrays nobody reads."""

    def __init__(self, lib):
        self.lib = lib
        self.R, self.N, self.H, self.W, self.C, self.PH, self.PW, self.S, self.aligned = 5, 2, 6, 9, 8, 7, 7, 2, 1
        self.nt = lib.wssdl_roi_align_tables_bytes(self.R, self.PH, self.PW, self.S)
        self.nws = lib.wssdl_roi_align_backward_workspace_bytes(self.R, self.N, self.H, self.W)
        self.keep = [np.zeros(max(n, 16), np.uint8) for n in (self.R * 5 * 4, self.nt, self.nws, 64, 64, 64, 64)]
        p = [ctypes.c_void_p(a.ctypes.data) for a in self.keep]
        self.rois, self.tables, self.ws, self.bottom, self.top, self.top_diff, self.bottom_diff = p

    def call(self, export, **change):
        a = _Args.__new__(_Args)
        a.__dict__.update(self.__dict__)
        a.__dict__.update(change)
        if export == "tables":
            return a.lib.wssdl_roi_align_tables(a.rois, a.R, a.N, a.H, a.W, a.PH, a.PW, 0.0625, a.S, a.aligned, a.tables, a.nt, None)
        if export == "forward":
            return a.lib.wssdl_roi_align_forward(a.bottom, a.N, a.H, a.W, a.C, a.R, a.PH, a.PW, a.S, a.tables, a.nt, a.top, None)
        if export == "prepare":
            return a.lib.wssdl_roi_align_backward_prepare(a.R, a.N, a.H, a.W, a.PH, a.PW, a.S, a.tables, a.nt, a.ws, a.nws, None)
        assert export == "backward"
        return a.lib.wssdl_roi_align_backward(a.top_diff, a.R, a.N, a.H, a.W, a.C, a.PH, a.PW, a.S, a.tables, a.nt, a.ws, a.nws,
                                              a.bottom_diff, None)


_COMMON = [dict(S=0), dict(S=5), dict(S=-1), dict(N=0), dict(H=0), dict(W=-3), dict(PH=0), dict(PH=17), dict(PW=0), dict(PW=17),
           dict(R=-1), dict(tables=None), dict(nt=8)]
_INVALID = {
    "tables": _COMMON + [dict(rois=None), dict(aligned=2)],
    "forward": _COMMON + [dict(C=0), dict(bottom=None), dict(top=None)],
    "prepare": _COMMON + [dict(ws=None), dict(nws=4)],
    "backward": _COMMON + [dict(C=0), dict(top_diff=None), dict(bottom_diff=None), dict(ws=None), dict(nws=4)],
}


@pytest.mark.parametrize("export", sorted(_INVALID))
def test_invalid_arguments_return_status_1_before_any_launch(L, export):
    a = _Args(L)
    assert a.nt == 5 * (4 * 7 * 2 + 4 * 7 * 2 + 5) * 4 and a.nws > 0
    for change in _INVALID[export]:
        # (a launch on this machine could only come back as WSSDL_ERR_LAUNCH = 3 or crash on the host arrays)
        assert a.call(export, **change) == 1, (export, change)
        assert L.wssdl_last_error() != b"", (export, change)
    # R = 0 is a valid call that launches nothing (the backward's zero fill is enqueued work: GPU tests)
    if export != "backward":
        assert a.call(export, R=0, rois=None, tables=None, nt=0, ws=None, nws=0, bottom=None, top=None) == 0
        assert L.wssdl_last_error() == b""


def test_size_queries(L):
    assert L.wssdl_roi_align_tables_bytes(0, 7, 7, 2) == 0
    assert L.wssdl_roi_align_tables_bytes(3, 7, 7, 0) == 0 and L.wssdl_roi_align_tables_bytes(3, 17, 7, 2) == 0
    assert L.wssdl_roi_align_tables_bytes(3, 3, 5, 3) == 3 * (4 * 3 * 3 + 4 * 5 * 3 + 5) * 4
    assert L.wssdl_roi_align_backward_workspace_bytes(0, 1, 5, 6) > 0 and L.wssdl_roi_align_backward_workspace_bytes(5, 0, 5, 6) == 0


# ------------------------------------------------------------------------------------------------ cfg and the layer ---
def test_cfg_keys_and_set_cfgs(pool_cfg):
    from wssdl_bus_amd.roi_pooling_layer import roi_align_op
    assert (cfg.ROI_POOL_MODE, cfg.ROI_ALIGN_SAMPLING, cfg.ROI_ALIGN_ALIGNED) == ('max', 2, True)
    assert roi_align_op.pool_mode() == 'max'
    cfg_from_list(['ROI_POOL_MODE', 'align', 'ROI_ALIGN_SAMPLING', '4', 'ROI_ALIGN_ALIGNED', 'False'])
    assert roi_align_op.settings() == dict(mode='align', sampling=4, aligned=False)
    cfg_from_list(['ROI_POOL_MODE', 'average'])
    with pytest.raises(ValueError):
        roi_align_op.pool_mode()


@pytest.mark.parametrize("entry", ["train", "train_alter", "test"])
def test_set_cfgs_on_the_command_lines(pool_cfg, entry, capsys):
    import importlib
    from wssdl_bus_amd.main import _common
    mod = importlib.import_module("wssdl_bus_amd.main." + entry)
    if entry == "test":
        args = mod.parse_args(["--trained_model", "m.pt", "--set_cfgs", "ROI_POOL_MODE", "align"])
    else:
        args = mod.parser().parse_args(["--output_dir", "out", "--set_cfgs", "ROI_POOL_MODE", "align"])
    _common.setup(args, seed=False)
    assert cfg.ROI_POOL_MODE == 'align' and "'ROI_POOL_MODE': 'align'" in capsys.readouterr().out


def test_layer_dispatch(pool_cfg, monkeypatch):
    from wssdl_bus_amd.networks import network
    calls = []
    monkeypatch.setattr(network.roi_pool_op, "roi_pool_autograd",
                        lambda *a, **k: calls.append(("max", a, k)) or (torch.ones(1), None))
    monkeypatch.setattr(network.roi_align_op, "roi_align_autograd", lambda *a, **k: calls.append(("align", a, k)) or torch.zeros(1))
    data, rois = torch.zeros(1, 2, 2, 1), torch.zeros(1, 5)

    def run():
        net = network.Network({'feat': data, 'rois': (rois, 'labels')})
        net.feed('feat', 'rois').roi_pool(7, 7, 1.0 / 16, name='roi_pool')
        return net.get_output('roi_pool')

    assert run().item() == 1.0                      # 'max': exactly today's call
    kind, a, k = calls.pop()
    assert kind == "max" and a[0] is data and a[1] is rois and a[2:] == (7, 7, 1.0 / 16) and k == dict(return_argmax=False)
    cfg.ROI_POOL_MODE = 'align'
    assert run().item() == 0.0
    kind, a, k = calls.pop()
    assert kind == "align" and a[0] is data and a[1] is rois and a[2:] == (7, 7, 1.0 / 16) and not k
    cfg.ROI_POOL_MODE = 'mean'
    with pytest.raises(ValueError):
        run()
    assert not calls


def test_adaptive_sampling_is_a_value_error():
    from wssdl_bus_amd.roi_pooling_layer import roi_align_op
    for S in (0, 5, -1):
        with pytest.raises(ValueError):
            roi_align_op._Geom((1, 4, 4, 8), torch.zeros(2, 5), 7, 7, 1.0 / 16, S, True)


# ------------------------------------------------------------------------------------------------------ snapshots ---
class _Net(object):
    def __init__(self):
        self.w = torch.zeros(2)

    def state_dict(self):
        return {'w': self.w.clone()}

    def load_state_dict(self, sd, strict=True):
        self.w = sd['w'].clone()


class _Opt(object):
    def state_dict(self):
        return {}

    def load_state_dict(self, sd):
        pass


class _Solver(object):
    def __init__(self):
        self.net, self.optimizer, self.optimizer_ws, self.rop = _Net(), _Opt(), None, None
        self.opt, self.lr, self.lr_scheduling, self.max_iters, self.global_step = 'adam', 1e-3, 'const', 5, 0

    def check_flags(self):
        pass


def test_snapshot_records_the_pooling_mode(pool_cfg, tmp_path):
    from wssdl_bus_amd.fast_rcnn import snapshot
    cfg.ROI_POOL_MODE = 'align'
    path = snapshot.save_snapshot(_Solver(), str(tmp_path), 'Stubnet_bus', 2, {}, {})
    assert snapshot.load_file(path)['roi_pool'] == dict(mode='align', sampling=2, aligned=True)
    assert snapshot.restore(path, _Solver(), {})[0] == 3
    cfg.ROI_ALIGN_SAMPLING = 4
    with pytest.raises(ValueError):
        snapshot.restore(path, _Solver(), {})
    cfg.ROI_ALIGN_SAMPLING = 2
    cfg.ROI_POOL_MODE = 'max'
    with pytest.raises(ValueError):
        snapshot.restore(path, _Solver(), {})
    # a file from before the key existed was written under 'max'
    state = snapshot.load_file(path)
    del state['roi_pool']
    old = str(tmp_path / 'old.pt')
    torch.save(state, old)
    assert snapshot.restore(old, _Solver(), {})[0] == 3
    cfg.ROI_POOL_MODE = 'align'
    with pytest.raises(ValueError):
        snapshot.restore(old, _Solver(), {})
