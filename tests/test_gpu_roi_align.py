"""GPU: RoIAlign (csrc/roi_align.hip) against tests/roi_align_reference.py -- the device tables bit for bit against the
f32 restatement, EVERY element of top and of the gradient inside its counted bound around the f64 direct form, exact
zeros where the reference has exact zeros, the same bits on a second run, the autograd wiring, and the 'roi_pool' layer
of the networks under cfg.ROI_POOL_MODE = 'align'.  Each configuration runs the device once; its results are shared."""
import numpy as np
import pytest

import roi_align_reference as ref

pytestmark = pytest.mark.gpu

CONFIGS = [('mixed', S, a) for S in (1, 2, 4) for a in (False, True)] + \
          [(name, ref.make_case(name)['S'], a) for name in ('axes', 'wide', 'many', 'empty') for a in (False, True)]
_IDS = ['%s-S%d-%s' % (n, S, 'aligned' if a else 'legacy') for n, S, a in CONFIGS]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd import _lib
    _lib.lib()
    return torch


_runs = {}


def device_run(torch, name, S, aligned):
    """tables, top and bottom_diff of the NumPy ops (twice), and of the autograd pair, for one configuration."""
    key = (name, S, aligned)
    if key not in _runs:
        from wssdl_bus_amd.roi_pooling_layer import roi_align_op as op
        c = ref.make_case(name)
        args = (c['PH'], c['PW'], c['scale'], S, aligned)
        out = dict(tables=op.roi_align_tables(c['rois'], c['shape'], *args))
        for k in ('', '2'):
            out['top' + k] = op.roi_align(c['data'], c['rois'], *args)
            out['diff' + k] = op.roi_align_grad(c['data'], c['rois'], c['grad'], *args)
        data = torch.from_numpy(c['data']).cuda().requires_grad_(True)
        top = op.roi_align_autograd(data, torch.from_numpy(c['rois']).cuda(), *args)
        top.backward(torch.from_numpy(c['grad']).cuda())
        out['auto_top'], out['auto_diff'] = top.detach().cpu().numpy(), data.grad.cpu().numpy()
        _runs[key] = out
    return _runs[key]


def _inside(what, got, want, bound):
    """Every element inside its bound; the figures are printed first."""
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("%s: max |error| %.3e, max error / bound %.3f, elements %d" % (what, float(err.max()) if err.size else 0.0, ratio, err.size))
    assert np.isfinite(got).all()
    assert (err <= bound).all(), what


@pytest.mark.parametrize("name,S,aligned", CONFIGS, ids=_IDS)
def test_tables_equal_the_f32_restatement_bit_for_bit(torch_cuda, name, S, aligned):
    got, want = device_run(torch_cuda, name, S, aligned)['tables'], ref.reference(name, S, aligned)['tables']
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k


@pytest.mark.parametrize("name,S,aligned", CONFIGS, ids=_IDS)
def test_top_inside_its_bound_everywhere(torch_cuda, name, S, aligned):
    c, got, want = ref.make_case(name), device_run(torch_cuda, name, S, aligned), ref.reference(name, S, aligned)
    assert got['top'].shape == (len(c['rois']), c['PH'], c['PW'], c['shape'][3]) and got['top'].dtype == np.float32
    _inside("top %s S=%d aligned=%s" % (name, S, aligned), got['top'], want['top'], want['top_bound'])
    zero = want['top_bound'] == 0                           # dead rows and void samples: exact zeros
    assert not got['top'][zero].any()
    dead = want['tables']['win'][:, 0] < 0
    assert not got['top'][dead].any()
    if name == 'mixed':
        assert dead.sum() == 5 and not got['top'][c['rows']['void']].any()
        assert np.array_equal(got['top'][c['rows']['twin_a']], got['top'][c['rows']['twin_b']])
    assert np.array_equal(got['top'].view(np.int32), got['top2'].view(np.int32))              # the same bits on every run


@pytest.mark.parametrize("name,S,aligned", CONFIGS, ids=_IDS)
def test_gradient_inside_its_bound_everywhere(torch_cuda, name, S, aligned):
    c, got, want = ref.make_case(name), device_run(torch_cuda, name, S, aligned), ref.reference(name, S, aligned)
    assert got['diff'].shape == c['shape'] and got['diff'].dtype == np.float32
    # (the reference's adjoint runs over every row: the box listed twice in 'mixed' counts once per copy)
    _inside("bottom_diff %s S=%d aligned=%s" % (name, S, aligned), got['diff'], want['diff'], want['diff_bound'])
    assert not got['diff'][~want['touched']].any()          # untouched cells are written, with exact zeros
    assert not got['diff'][want['diff_bound'] == 0].any()
    if name == 'mixed':
        assert not got['diff'][c['empty_image']].any() and got['diff'][0].any() and got['diff'][1].any()
    if name == 'empty':
        assert not got['diff'].any()
    assert np.array_equal(got['diff'].view(np.int32), got['diff2'].view(np.int32))


def test_gradient_counts_a_box_listed_twice_twice(torch_cuda):
    """Dropping one twin's row from the gradient changes the cells of its window by far more than the bound."""
    from wssdl_bus_amd.roi_pooling_layer import roi_align_op as op
    c = ref.make_case('mixed')
    got, want = device_run(torch_cuda, 'mixed', 2, True), ref.reference('mixed', 2, True)
    g = c['grad'].copy()
    g[c['rows']['twin_b']] = 0
    once = op.roi_align_grad(c['data'], c['rois'], g, c['PH'], c['PW'], c['scale'], 2, True)
    t = ref.tables(c['rois'], *c['shape'][:3], c['PH'], c['PW'], c['scale'], 2, True)
    want_once, bound_once, _ = ref.adjoint(g, t, c['shape'], 2)
    _inside("bottom_diff with one twin silenced", once, want_once, bound_once)
    moved = np.abs(got['diff'].astype(np.float64) - once) > 4 * want['diff_bound']
    win = t['win'][c['rows']['twin_b']]
    assert moved[0, win[1]:win[2] + 1, win[3]:win[4] + 1].mean() > 0.9 and not moved[1].any()


@pytest.mark.parametrize("name,S,aligned", CONFIGS, ids=_IDS)
def test_autograd_agrees_with_the_op_pair(torch_cuda, name, S, aligned):
    got = device_run(torch_cuda, name, S, aligned)
    assert np.array_equal(got['auto_top'].view(np.int32), got['top'].view(np.int32))
    assert np.array_equal(got['auto_diff'].view(np.int32), got['diff'].view(np.int32))


def test_arguments_the_ops_refuse(torch_cuda):
    from wssdl_bus_amd import _lib
    from wssdl_bus_amd.roi_pooling_layer import roi_align_op as op
    c = ref.make_case('axes')
    with pytest.raises(ValueError):
        op.roi_align(c['data'], c['rois'], 3, 5, c['scale'], 0, True)              # adaptive sampling
    with pytest.raises((ValueError, _lib.HipCallError)):
        op.roi_align(c['data'], c['rois'], 17, 5, c['scale'], 2, True)


# ------------------------------------------------------------------------------------------------- the networks ---
@pytest.fixture
def align_mode():
    from wssdl_bus_amd.fast_rcnn.config import cfg
    old = cfg.ROI_POOL_MODE, cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG
    cfg.ROI_POOL_MODE = 'align'
    yield cfg
    cfg.ROI_POOL_MODE, cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG = old
    from wssdl_bus_amd.roi_pooling_layer import roi_pooling_op
    assert not roi_pooling_op.flags_raised()                # nothing here may leave a deferred device flag up


def test_layer_returns_the_align_result(torch_cuda, align_mode):
    torch = torch_cuda
    from wssdl_bus_amd.networks.network import Network
    c = ref.make_case('mixed')
    data, rois = torch.from_numpy(c['data']).cuda(), torch.from_numpy(c['rois']).cuda()
    net = Network({'feat': data, 'rois': rois})
    net.feed('feat', 'rois').roi_pool(7, 7, c['scale'], name='roi_pool')
    want = device_run(torch, 'mixed', 2, True)['top']                       # cfg's defaults: S = 2, aligned
    assert np.array_equal(net.get_output('roi_pool').cpu().numpy().view(np.int32), want.view(np.int32))
    net.feed('feat', 'rois').roi_align(7, 7, c['scale'], name='explicit', sampling_ratio=4, aligned=False)
    want = device_run(torch, 'mixed', 4, False)['top']
    assert np.array_equal(net.get_output('explicit').cpu().numpy().view(np.int32), want.view(np.int32))
    # back under 'max' the layer is RoI max pooling again (interior boxes only: a box reaching far outside the map would
    # raise the max pair's deferred window flag, which belongs to whoever polls it next)
    align_mode.ROI_POOL_MODE = 'max'
    inside = torch.from_numpy(c['rois'][[c['rows']['whole'], c['rows']['twin_a'], c['rows']['tiny']]]).cuda()
    net2 = Network({'feat': data, 'rois': inside})
    net2.feed('feat', 'rois').roi_pool(7, 7, c['scale'], name='max')
    from oracle import c_oracle
    want_max, _ = c_oracle.roi_pool_forward(c['data'], inside.cpu().numpy(), 7, 7, c['scale'], "cuda")
    assert np.array_equal(net2.get_output('max').cpu().numpy(), want_max)


def test_resnet18_train_step_and_test_forward_under_align(torch_cuda, align_mode):
    torch, cfg = torch_cuda, align_mode
    from wssdl_bus_amd import synthetic
    from wssdl_bus_amd.fast_rcnn.train_bus import SolverWrapper
    from wssdl_bus_amd.networks.factory_bus import get_network
    from wssdl_bus_amd.roi_pooling_layer import roi_align_op
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG = 1, 1, "reference"
    np.random.seed(3)
    torch.manual_seed(3)
    calls = []
    real = roi_align_op.roi_align_autograd
    roi_align_op.roi_align_autograd = lambda *a, **k: calls.append(a[1].shape[0]) or real(*a, **k)
    try:
        net = get_network("Resnet_train", 18).cuda().to(memory_format=torch.channels_last)
        blobs = synthetic.make_batch(1, 1, 320, 480, seed=3)
        solver = SolverWrapper(net)
        losses = solver.joint_backward(blobs)
        for k in ("loss", "mil_cross_entropy", "rpn_cross_entropy", "rpn_loss_box", "cross_entropy", "loss_box"):
            assert torch.isfinite(losses[k]).all(), k
        grads = [p.grad for p in net.trunk.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(g).all() for g in grads) and any(bool(g.any()) for g in grads)
        solver._apply()
        assert len(calls) == 1 and calls[0] > 0
        net.eval()
        with torch.no_grad():
            out = net(blobs['data'], blobs['im_info'], None, None, is_training=False, is_ws=False, test_net=True)
        assert len(calls) == 2 and out['roi_pool'].shape[0] == calls[1] and torch.isfinite(out['cls_prob']).all()
    finally:
        roi_align_op.roi_align_autograd = real
