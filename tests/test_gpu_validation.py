"""-m gpu: the validation pass on the device.  The per-image loss op (csrc/loss.hip: wssdl_multi_task_loss_per_image
through loss_op.multi_task_loss_per_image) against the f64 reference of tests/loss_reference.py evaluated on every
image's single-image slice, its consistency with the batch op, its determinism, the wiring of
train_bus.validation_losses on real forwards of both networks, SolverWrapper.validate end to end, and the export's
argument checks.  The bounds are the ones loss_reference counts (its allowance for expf / log1pf measured on this
device by the module's fixture, as test_gpu_loss_reference.py does); none was chosen by looking at a result."""
import ctypes

import numpy as np
import pytest
import torch

import loss_reference as R
import validation_cases as V

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOG = {}

# seed, N, H, W, A, K, rows per image, regime per image, nan images.  "four_images": 2160 anchors and 8640 box elements
# per image (more than one workgroup of 2048, no multiple of it), an empty image, one row, more than MTL_BLOCK rows.
CASES = {
    "four_images": (31, 4, 16, 15, 9, 3, [0, 1, 128, 300], ["normal", "correct", "shift12", "wrong"], (1,)),
    "one_cell": (32, 1, 1, 1, 1, 3, [1], ["normal"], ()),
}
_cache = {}


def _case(name, plain=False):
    """the case on the device, built once.  plain: no NaN image, rows in layer order, no padding rows with weights
    and no rows of no image (what the batch op can be compared on)."""
    key = (name, plain)
    if key not in _cache:
        seed, N, H, W, A, K, rows, regimes, nan_images = CASES[name]
        _cache[key] = V.make_val_case(seed, N, H, W, A, K, rows, regimes, shuffle=not plain,
                                      nan_images=() if plain else nan_images, junk=not plain, device=DEV)
    return _cache[key]


def _probe(L, x, which):
    from wssdl_bus_amd import _lib
    y = torch.empty_like(x)
    _lib.check(L.wssdl_loss_libm_probe(_lib.ptr(x), x.numel(), which, _lib.ptr(y), _lib.stream()), "wssdl_loss_libm_probe")
    return y


@pytest.fixture(scope="module")
def L():
    """the library, with the bounds' allowance measured on this device over the grids and the cases' own arguments"""
    assert torch.cuda.is_available()
    from wssdl_bus_amd import _lib
    lib = _lib.lib()
    ex, lg = R.lib_grids(DEV)
    R.ALLOW.update(exp=0, log1p=0)                              # provisional: only the cases' arguments are taken here
    args, z1 = [ex], [lg]
    for name in CASES:
        for plain in (False, True):
            c = _case(name, plain)
            for ref in [R.mt_reference(V.slice_case(c, i)) for i in range(c["dims"][0])] + [R.mt_reference(c)]:
                args.append(ref["args"])
                z1.append(ref["z1"])
    a, z1 = torch.cat(args).contiguous(), torch.cat(z1).contiguous()
    R.ALLOW.clear()
    we = R.lib_accuracy(_probe(lib, a, 0), torch.exp(a.double()))
    wl = R.lib_accuracy(_probe(lib, z1, 1), torch.log1p(z1.double()))
    print("loss-lib-allowance %s" % R.set_allowance(we[0], wl[0]))
    yield lib
    for k in sorted(LOG):
        print("validation-worst %s %.4g" % (k, LOG[k]))


def _per_image(c):
    from wssdl_bus_amd.fast_rcnn.loss_op import multi_task_loss_per_image
    return multi_task_loss_per_image(*V.layer_args(c), c["dims"][0])


def _batch(c):
    from wssdl_bus_amd.fast_rcnn.loss_op import multi_task_loss
    with torch.no_grad():
        return multi_task_loss(*V.layer_args(c), c["dims"][0])


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- 1: the kernel against the f64 reference

@pytest.mark.parametrize("name", list(CASES))
def test_per_image_kernel_inside_the_reference_bounds(L, name):
    """every image's four values inside the bounds counted for that image's single-image case: interleaved rows,
    padding rows with weights, rows of image -1 and N, an empty image, an image without labelled anchors (NaN)"""
    seed, N, H, W, A, K, rows, regimes, nan_images = CASES[name]
    c = _case(name)
    losses, counts = _per_image(c)
    assert losses.shape == (N, 4) and counts.shape == (N, 2)
    V.per_image_ratios(c, losses, LOG)
    for i in range(N):
        assert bool(torch.isnan(losses[i, 0])) == (i in nan_images)
        assert bool(torch.isnan(losses[i, 2])) == (rows[i] == 0)
        assert float(counts[i, 1]) == rows[i]
        assert float(counts[i, 0]) == float((c["rpn_labels"][i] != -1).sum())
    if name == "four_images":
        assert int((c["rois"][:, 0] == -1).sum()) == 1 and int((c["rois"][:, 0] == N).sum()) == 1
        pad = c["labels"].reshape(-1) == -1
        assert int(pad.sum()) == 9 and bool((c["outw"][pad].sum(1) > 0).all())
        img = c["rois"][:, 0]
        assert int((img[1:] != img[:-1]).sum()) > 100            # the images interleave


# ---------------------------------------------------------------- 2: consistency with the batch op

def test_per_image_values_combine_to_the_batch_op(L):
    """mean of rpn_loss_box, and the count-weighted means of the other three, against multi_task_loss on the same
    inputs; tolerance = the batch value's counted bound + the combination of the per-image values' counted bounds
    (an error of at most b_i in value i moves a weighted mean by at most the same weighted mean of the b_i)"""
    c = _case("four_images", plain=True)
    N = c["dims"][0]
    losses, counts = _per_image(c)
    batch = _batch(c).double().cpu()
    ref_b = R.mt_reference(c)
    refs = [R.mt_reference(V.slice_case(c, i)) for i in range(N)]
    v, n = losses.double().cpu(), counts.double().cpu()
    b = torch.tensor([r["b_terms"] for r in refs], dtype=torch.float64)

    def weighted(x, w):
        keep = w > 0                                             # (an image without rows: NaN times a zero count)
        return float((x[keep] * w[keep]).sum() / w[keep].sum())
    got = [weighted(v[:, 0], n[:, 0]), float(v[:, 1].mean()), weighted(v[:, 2], n[:, 1]), weighted(v[:, 3], n[:, 1])]
    tol = [weighted(b[:, 0], n[:, 0]), float(b[:, 1].mean()), weighted(b[:, 2], n[:, 1]), weighted(b[:, 3], n[:, 1])]
    ratios = {}
    for k, name in enumerate(("rpn_ce", "rpn_box", "ce", "box")):
        print("validation-combine %s per-image %.9g batch %.9g tolerance %.3g" % (name, got[k], float(batch[k]),
                                                                                 tol[k] + ref_b["b_terms"][k]))
        ratios["combine_" + name] = R.ratio(got[k], float(batch[k]), tol[k] + ref_b["b_terms"][k])
    R.check_ratios("four_images", ratios, LOG)
    assert float(n[:, 0].sum()) == float((c["rpn_labels"] != -1).sum()) and float(n[:, 1].sum()) == c["n_rows"]


# ---------------------------------------------------------------- 3: determinism

def test_per_image_op_is_deterministic_and_leaves_the_batch_op_alone(L):
    c = _case("four_images")
    before = _batch(c)
    l1, n1 = _per_image(c)
    l2, n2 = _per_image(c)
    after = _batch(c)
    assert torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(n1), _bits(n2))
    assert torch.equal(_bits(before), _bits(after))


# ---------------------------------------------------------------- 4: wiring on real forwards

@pytest.fixture()
def cfg_guard():
    from wssdl_bus_amd.fast_rcnn.config import cfg
    old = (cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG, cfg.TRAIN.USE_BRN)
    yield cfg
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG, cfg.TRAIN.USE_BRN = old


def _net(name, seed):
    from wssdl_bus_amd.networks.factory_bus import get_network
    torch.manual_seed(seed)
    return get_network(name, 18).cuda().to(memory_format=torch.channels_last)


@pytest.mark.parametrize("net_name", ["Resnet_train", "Resnet_train_alter"])
def test_validation_losses_equal_the_sliced_losses(L, cfg_guard, net_name):
    """validation_losses on one eval forward of two images against supervised_loss on hand-sliced per-image layers
    (inside the sum of the two ops' counted bounds for that image's case) and mil_loss on the image's rows as one bag
    (the same arithmetic: bit-equal)"""
    from wssdl_bus_amd import synthetic
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    from wssdl_bus_amd.mil import core as M
    cfg = cfg_guard
    alter = net_name.endswith("_alter")
    cfg.SAMPLING_RNG = "device"
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = 2, 2
    net = _net(net_name, 41)
    net.eval()
    blobs = synthetic.make_batch(2, 0, 320, 480, seed=41)
    step = 4100
    with torch.no_grad():
        layers = dict(net(blobs["data"], blobs["im_info"], blobs["gt_boxes"], blobs["num_gt_boxes"], is_training=False,
                          is_ws=False))
        got = T.validation_losses(layers, blobs["im_info"], 2, step, alter)
        assert set(got) == set(T.VAL_TERMS) and all(tuple(t.shape) == (2,) for t in got.values())
        rois, labels, tg, inw, outw = layers["roi-data"]
        N, H, W, A2 = layers["rpn_cls_score"].shape
        funcs = [M.get_mass_max_logit, M.get_mal_max_logit] if alter else [M.get_mal_max_logit, M.get_mal_max_logit]
        for i in range(2):
            rows = (rois[:, 0] == i).nonzero().squeeze(1)
            assert rows.numel() > 0
            sl = {"rpn_cls_score": layers["rpn_cls_score"][i:i + 1].contiguous(),
                  "rpn_bbox_pred": layers["rpn_bbox_pred"][i:i + 1].contiguous(),
                  "rpn-data": tuple(t[i:i + 1].contiguous() for t in layers["rpn-data"]),
                  "roi-data": (rois[rows], labels[rows], tg[rows], inw[rows], outw[rows]),
                  "cls_score": layers["cls_score"][rows], "bbox_pred": layers["bbox_pred"][rows]}
            cfg.TRAIN.IMS_PER_BATCH = 1
            try:
                want = T.supervised_loss(sl, [], None if alter else int(cfg.TRAIN.IMS_PER_BATCH))
            finally:
                cfg.TRAIN.IMS_PER_BATCH = 2
            case = dict(rpn_cls=sl["rpn_cls_score"], rpn_box=sl["rpn_bbox_pred"], rpn_labels=sl["rpn-data"][0],
                        rpn_tg=sl["rpn-data"][1], rpn_inw=sl["rpn-data"][2], rpn_outw=sl["rpn-data"][3],
                        cls=sl["cls_score"].contiguous(), box=sl["bbox_pred"].contiguous(), labels=labels[rows],
                        tg=tg[rows], inw=inw[rows], outw=outw[rows], dims=(1, H, W, A2 // 2, 1), n_rows=int(rows.numel()),
                        rows_total=int(rows.numel()), K=3, gl=torch.ones(4, device=DEV))
            ref = R.mt_reference(case)
            ratios = {}
            for k, name in enumerate(("rpn_cross_entropy", "rpn_loss_box", "cross_entropy", "loss_box")):
                ratios["wiring_" + name] = R.ratio(got[name][i], float(want[name]), 2.0 * ref["b_terms"][k])
            R.check_ratios("%s[%d]" % (net_name, i), ratios, LOG)
            total = ((got["rpn_cross_entropy"][i] + got["rpn_loss_box"][i]) + got["cross_entropy"][i]) + got["loss_box"][i]
            assert torch.equal(got["total"][i], total) and bool(torch.isfinite(total))
            mil = T.mil_loss(layers["cls_score"][rows].contiguous(), rois[rows, 0] - float(i),
                             blobs["im_info"][i:i + 1, 3].to(torch.int32), 1, step, funcs)
            assert torch.equal(got["mil_cross_entropy"][i], mil), (float(got["mil_cross_entropy"][i]), float(mil))


# ---------------------------------------------------------------- 5: validate end to end

@pytest.mark.parametrize("brn", [False, True])
def test_validate_end_to_end_changes_nothing(L, cfg_guard, brn):
    """two blobs (2 images, 1 image) through SolverWrapper.validate after one train step: three per-image rows, every
    state_dict tensor (running statistics; with brn the renorm buffers) bit-equal, global_step unchanged, no .grad
    left, and the next train step still runs"""
    from wssdl_bus_amd import synthetic
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    cfg = cfg_guard
    cfg.SAMPLING_RNG = "device"
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = 2, 2
    cfg.TRAIN.USE_BRN = brn
    net = _net("Resnet_train", 43)
    net.train()
    solver = T.SolverWrapper(net)
    train_blobs = synthetic.make_batch(2, 2, 320, 480, seed=43)
    solver.train_step_joint(train_blobs)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    assert any(k.endswith("running_mean") for k in state) and any("renorm_mean" in k for k in state) == brn
    if brn:                                                      # the train step has moved the renorm state off its zeros
        assert any(bool(v.any()) for k, v in state.items() if "renorm_mean" in k)
    step = solver.global_step
    out = solver.validate([synthetic.make_batch(2, 0, 320, 480, seed=44), synthetic.make_batch(1, 0, 320, 480, seed=45)])
    assert out["n_images"] == 3 and out["per_image"].shape == (3, 6)
    assert np.isfinite(out["per_image"]).all() and np.isfinite(out["total"])
    assert list(out)[:6] == list(T.VAL_TERMS)
    after = net.state_dict()
    assert set(after) == set(state)
    changed = [k for k in state if not torch.equal(state[k], after[k])]
    assert not changed, changed
    assert solver.global_step == step and net.training and int(cfg.TRAIN.IMS_PER_BATCH) == 2
    assert all(p.grad is None for p in net.parameters())
    losses = solver.train_step_joint(train_blobs)
    assert bool(torch.isfinite(losses["loss"])) and solver.global_step == step + 1
    solver.check_flags()


# ---------------------------------------------------------------- 6: argument validation

def test_export_rejects_invalid_arguments(L):
    from wssdl_bus_amd import _lib
    c = _case("one_cell")
    a = V.layer_args(c)
    N, H, W, A, _ = c["dims"]
    K = c["K"]
    need = L.wssdl_multi_task_loss_per_image_workspace_bytes(N, H, W, A)
    assert need > 0 and L.wssdl_multi_task_loss_per_image_workspace_bytes(0, H, W, A) == 0
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    losses = torch.full((N, 4), -7.0, device=DEV)
    counts = torch.full((N, 2), -7.0, device=DEV)
    p = _lib.ptr

    def call(K=K, losses_p=p(losses), ws_bytes=need, stride=5):
        return L.wssdl_multi_task_loss_per_image(
            p(a[0]), p(a[4][0]), p(a[1]), p(a[4][1]), p(a[4][2]), p(a[4][3]), N, H, W, A, p(a[2]), p(a[5][1]), p(a[3]),
            p(a[5][2]), p(a[5][3]), p(a[5][4]), c["n_rows"], K, p(a[5][0]), stride, losses_p, p(counts), p(ws), ws_bytes,
            _lib.stream())
    bad = _lib.ERR_INVALID_ARGUMENT
    assert call(K=1) == bad and call(K=33) == bad
    assert call(losses_p=ctypes.c_void_p(None)) == bad
    assert call(ws_bytes=need - 1) == bad
    assert call(stride=0) == bad
    torch.cuda.synchronize()
    assert bool((losses == -7.0).all()) and bool((counts == -7.0).all())       # nothing was launched
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert bool((counts >= 0).all())
