"""The validation pass without a GPU: loss_op.multi_task_loss_per_image on CPU tensors (its torch path) against the
f64 reference of tests/loss_reference.py, and SolverWrapper.validate driven by a stub network whose forward returns
prepared layers.  No HIP kernel runs here; test_gpu_validation.py holds the device op to the same reference."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import loss_reference as R
import validation_cases as V


@pytest.fixture(scope="module", autouse=True)
def allowance():
    """the bounds' allowance for exp / log1p, measured on this machine's torch as test_loss_reference_cpu.py does"""
    ex, lg = R.lib_grids()
    we = R.lib_accuracy(torch.exp(ex), torch.exp(ex.double()))
    wl = R.lib_accuracy(torch.log1p(lg), torch.log1p(lg.double()))
    R.set_allowance(we[0], wl[0])
    yield


# seed, N, H, W, A, K, rows per image, regime per image, nan images
CASES = {
    "four_images": (11, 4, 16, 15, 9, 3, [0, 1, 128, 300], ["normal", "correct", "shift12", "wrong"], (1,)),
    "one_cell": (12, 1, 1, 1, 1, 3, [1], ["normal"], ()),
    "k32": (13, 2, 7, 13, 9, 32, [5, 70], ["tie2", "shift10"], ()),
}


@pytest.mark.parametrize("name", list(CASES))
def test_per_image_losses_inside_the_reference_bounds(name):
    """Every image's four values lie inside the bounds loss_reference counts for the four values of that image's
    single-image case; rows interleave, and padding rows with weights and rows of no image are in the list."""
    from wssdl_bus_amd.fast_rcnn.loss_op import multi_task_loss_per_image
    seed, N, H, W, A, K, rows, regimes, nan_images = CASES[name]
    c = V.make_val_case(seed, N, H, W, A, K, rows, regimes, shuffle=True, nan_images=nan_images, junk=True)
    losses, counts = multi_task_loss_per_image(*V.layer_args(c), N)
    assert losses.shape == (N, 4) and counts.shape == (N, 2) and losses.dtype == torch.float32
    V.per_image_ratios(c, losses)
    for i in range(N):
        assert math.isnan(float(losses[i, 0])) == (i in nan_images)
        assert math.isnan(float(losses[i, 2])) == (rows[i] == 0)
        assert float(counts[i, 1]) == rows[i]
        assert float(counts[i, 0]) == float((c["rpn_labels"][i] != -1).sum())


def test_per_image_op_refuses_autograd_inputs():
    from wssdl_bus_amd.fast_rcnn.loss_op import multi_task_loss_per_image
    c = V.make_val_case(14, 1, 2, 2, 1, 3, [2], ["normal"])
    args = list(V.layer_args(c))
    args[0] = args[0].clone().requires_grad_(True)
    with pytest.raises(RuntimeError):
        multi_task_loss_per_image(*args, 1)
    with torch.no_grad():
        multi_task_loss_per_image(*args, 1)


# ----------------------------------------------------------------- validate with a stub network

class _Stub(nn.Module):
    """forward returns the prepared layers of the next batch; `script` may hold an exception instead"""
    alter = False

    def __init__(self, script):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))
        self.script = list(script)
        self.seen = []                                   # (net.training, cfg.TRAIN.IMS_PER_BATCH, grad mode) per forward

    def forward(self, data, im_info, gt_boxes, num_gt_boxes, is_training=True, is_ws=False):
        from wssdl_bus_amd.fast_rcnn.config import cfg
        assert is_training is False and is_ws is False
        self.seen.append((self.training, int(cfg.TRAIN.IMS_PER_BATCH), torch.is_grad_enabled()))
        item = self.script.pop(0)
        if isinstance(item, Exception):
            raise item
        return item

    def weight_decay_params(self):
        return []


def _layers_and_blobs(seed, n, rows):
    c = V.make_val_case(seed, n, 3, 4, 2, 3, rows, ["normal"] * n)
    a = V.layer_args(c)
    layers = {"rpn_cls_score": a[0], "rpn_bbox_pred": a[1], "cls_score": a[2], "bbox_pred": a[3], "rpn-data": a[4],
              "roi-data": a[5]}
    im_info = torch.tensor([[48.0, 64.0, 1.0, 1 + (i % 2)] for i in range(n)])
    blobs = {"data": torch.zeros((n, 48, 64, 3)), "im_info": im_info, "gt_boxes": torch.zeros((n, 20, 5)),
             "num_gt_boxes": torch.ones((n,), dtype=torch.int32)}
    return c, layers, blobs


def _expected_rows(c, layers, blobs, n, step, alter):
    """[n, 6] f64 from the pieces validate is specified by: supervised terms of each image's slice in f64
    (mt_reference), their sum, and mil_loss on the image's rows as one bag"""
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    from wssdl_bus_amd.mil import core as M
    funcs = [M.get_mass_max_logit, M.get_mal_max_logit] if alter else [M.get_mal_max_logit, M.get_mal_max_logit]
    out = np.zeros((n, 6))
    for i in range(n):
        ref = R.mt_reference(V.slice_case(c, i))
        out[i, 1:5] = ref["terms"]
        out[i, 0] = sum(np.float32(t) for t in ref["terms"])
        rows = (c["rois"][:, 0] == i).nonzero().squeeze(1)
        out[i, 5] = float(T.mil_loss(c["cls"][rows], torch.zeros(rows.numel()), blobs["im_info"][i:i + 1, 3].to(torch.int32),
                                     1, step, funcs, counts_host=[rows.numel()]))
    return out


@pytest.fixture
def restore_cfg():
    from wssdl_bus_amd.fast_rcnn.config import cfg
    old = cfg.TRAIN.IMS_PER_BATCH
    yield cfg
    cfg.TRAIN.IMS_PER_BATCH = old


@pytest.mark.parametrize("alter", [False, True])
def test_validate_means_order_and_restored_state(restore_cfg, alter):
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    cfg = restore_cfg
    cfg.TRAIN.IMS_PER_BATCH = 7
    c2, l2, b2 = _layers_and_blobs(21, 2, [6, 9])
    c1, l1, b1 = _layers_and_blobs(22, 1, [4])
    net = _Stub([l2, l1])
    net.alter = alter
    net.train()
    solver = T.SolverWrapper(net, lr=0.01)
    solver.global_step = 4100
    out = solver.validate(iter([b2, b1]))
    want = np.concatenate([_expected_rows(c2, l2, b2, 2, 4100, alter), _expected_rows(c1, l1, b1, 1, 4100, alter)])
    assert T.VAL_TERMS == ("total", "rpn_cross_entropy", "rpn_loss_box", "cross_entropy", "loss_box", "mil_cross_entropy")
    assert list(out)[:6] == list(T.VAL_TERMS)
    assert out["n_images"] == 3 and out["per_image"].shape == (3, 6) and out["per_image"].dtype == np.float32
    # f32 values of O(1) against f64: a few roundings of the value itself (the counted bounds are test 1's business)
    np.testing.assert_allclose(out["per_image"], want, rtol=1e-5, atol=1e-7)
    for k, name in enumerate(T.VAL_TERMS):
        assert out[name] == pytest.approx(float(out["per_image"][:, k].astype(np.float64).mean()), rel=1e-12)
    p = out["per_image"]
    assert np.array_equal(p[:, 0], ((p[:, 1] + p[:, 2]) + p[:, 3]) + p[:, 4])          # the f32 sum, in the order of :519
    assert net.seen == [(False, 2, False), (False, 1, False)]         # eval mode, n per forward, no grad
    assert net.training is True and cfg.TRAIN.IMS_PER_BATCH == 7
    assert solver.global_step == 4100 and net.w.grad is None
    net.eval()
    net.script = [l1]
    solver.validate([b1])
    assert net.training is False                                      # the flag it had, not "train"


def test_validate_restores_state_when_the_forward_raises(restore_cfg):
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    cfg = restore_cfg
    cfg.TRAIN.IMS_PER_BATCH = 5
    _, l2, b2 = _layers_and_blobs(23, 2, [3, 3])
    net = _Stub([l2, ValueError("boom")])
    net.train()
    solver = T.SolverWrapper(net, lr=0.01, lr_scheduling="rop")
    with pytest.raises(ValueError, match="boom"):
        solver.validate([b2, b2])
    assert net.seen[-1][:2] == (False, 2)
    assert net.training is True and cfg.TRAIN.IMS_PER_BATCH == 5
    assert solver.rop.best == math.inf and solver.rop.wait == 0       # a failed pass feeds nothing


def test_validate_feeds_the_plateau_schedule(restore_cfg):
    """ReduceLROnPlateau's documented quirk: the first halving comes at the (patience + 1)-th = sixth pass without
    improvement, not before; feed_schedule=False leaves the schedule alone; the other schedules ignore the pass."""
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    _, la, ba = _layers_and_blobs(24, 1, [5])
    net = _Stub([])
    solver = T.SolverWrapper(net, lr=0.01, lr_scheduling="rop")
    net.script = [la]
    first = solver.validate([ba])                                     # sets `best`
    assert solver.rop.best == first["total"] and solver.current_lr() == 0.01
    net.script = [la]
    solver.validate([ba], feed_schedule=False)
    assert solver.rop.wait == 0                                       # not fed
    for k in range(1, 7):
        net.script = [la]                                             # the same loss again: no improvement
        solver.validate([ba])
        assert solver.current_lr() == (0.01 if k < 6 else 0.005), k
    const = T.SolverWrapper(_Stub([la]), lr=0.01)
    const.validate([ba])
    assert const.current_lr() == 0.01 and const.rop is None
