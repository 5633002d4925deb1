"""-m gpu: the detection half of the validation pass.  wssdl_decode_detections (csrc/decode_detect.hip) against the
NumPy statement of its arithmetic (tests/decode_reference.py), val_detect.validation_detections on a constructed layers
dict, SolverWrapper.validate(..., gt_roidb=...) end to end, and the export's argument checks.

Every comparison with the statement is BIT FOR BIT.  That is derived, not measured: the library is built with
-ffp-contract=off, so each f32 multiply, add and subtract is one IEEE operation on both sides; the f32 division is
correctly rounded on both sides; the exponential is an f64 exp rounded once to f32, and test_val_detect_cpu.py checks
that no exp of any case lies within 4 f64 ulps of an f32 rounding boundary, so two faithful f64 exps round alike."""
import ctypes

import numpy as np
import pytest
import torch

import decode_reference as D

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -7.0
_want = {}


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a, order="C")).to(DEV, dtype)              # (a copy: the cases are read-only)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _statement(name, given):
    """the statement of a run, computed once"""
    if (name, given) not in _want:
        c = D.case(name)
        _want[(name, given)] = D.statement(c["rois"], c["deltas"], c["im_info"], c["n_images"], c["bounds"] if given else None)
        _want[(name, given)].setflags(write=False)
    return _want[(name, given)]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from wssdl_bus_amd import _lib
    return _lib.lib()


def _raw(L, c, given, R=None, out=None):
    """the export itself on the case's first R rows, writing into `out` (default: R + 5 rows of sentinels)"""
    from wssdl_bus_amd import _lib
    R = c["rois"].shape[0] if R is None else R
    K = c["K"]
    rois, deltas, info = _t(c["rois"]), _t(c["deltas"]), _t(c["im_info"])
    bounds = _t(c["bounds"]) if given else None
    if out is None:
        out = torch.full((R + 5, 4 * K), SENTINEL, device=DEV)
    rc = L.wssdl_decode_detections(_lib.ptr(rois), _lib.ptr(deltas), R, K, _lib.ptr(info), int(info.shape[1]), c["n_images"],
                                   _lib.ptr(bounds), _lib.ptr(out), _lib.stream())
    torch.cuda.synchronize()
    return rc, out


# ---------------------------------------------------------------- 1: the kernel against the f32 statement

@pytest.mark.parametrize("name,given", D.RUNS)
def test_kernel_equals_the_statement_bit_for_bit(L, name, given):
    from wssdl_bus_amd import _lib
    from wssdl_bus_amd.fast_rcnn.val_detect import decode_detections_device
    c = D.case(name)
    assert bool(D.exp_is_safe(D.exp_arguments(c)).all())              # the precondition of bit equality
    want = _statement(name, given)
    R = c["rois"].shape[0]
    rc, out = _raw(L, c, given)
    assert rc == _lib.OK
    got = out.cpu().numpy()
    differ = _bits(got[:R]) != _bits(want)
    print("decode-kernel %s bounds=%s: %d of %d values differ from the statement" % (name, given, int(differ.sum()), differ.size))
    assert not differ.any(), np.argwhere(differ)[:8]
    live, _ = D.live_rows(c["rois"], c["n_images"])
    assert bool((got[:R][~live] == 0).all()) and bool((_bits(got[:R][~live]) == 0).all())      # dead rows: +0.0
    assert bool((got[R:] == SENTINEL).all())                          # nothing written past row R
    rc2, out2 = _raw(L, c, given)
    assert rc2 == _lib.OK and np.array_equal(_bits(out2), _bits(out))  # two runs, the same bits
    # the Python wrapper is the same op
    py = decode_detections_device(_t(c["rois"]), _t(c["deltas"]), _t(c["im_info"]), c["n_images"],
                                  _t(c["bounds"]) if given else None)
    assert tuple(py.shape) == want.shape and np.array_equal(_bits(py), _bits(want))


def test_no_rows_is_a_no_op(L):
    from wssdl_bus_amd import _lib
    from wssdl_bus_amd.fast_rcnn.val_detect import decode_detections_device
    c = D.case("one_row")
    rc, out = _raw(L, c, True, R=0)
    assert rc == _lib.OK and bool((out == SENTINEL).all())
    py = decode_detections_device(torch.zeros((0, 5), device=DEV), torch.zeros((0, 8), device=DEV), _t(c["im_info"]), 1)
    assert tuple(py.shape) == (0, 8)


# ---------------------------------------------------------------- 2: validation_detections on a constructed forward

class _cfg_set(object):
    """with _cfg_set(node, KEY=value, ...): sets and restores"""

    def __init__(self, node, **kv):
        self.node, self.kv = node, kv

    def __enter__(self):
        self.old = {k: self.node.get(k) for k in self.kv}
        for k, v in self.kv.items():
            self.node[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                self.node.pop(k, None)
            else:
                self.node[k] = v
        return False


def _reference_route(scores, boxes, rois, n_images, K, thresh, cap, agnostic):
    """per image: test_bus.postprocess_detections through its step-by-step path (per-class hip_nms calls, the union
    pass under the flag, boolean masks) on that image's rows of (scores, boxes) -> [{j: numpy [n,5]}]"""
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.test_bus import postprocess_detections
    out = []
    for i in range(n_images):
        rows = torch.nonzero(rois[:, 0] == i).reshape(-1)
        with _cfg_set(cfg.TEST, CLS_AGNOSTIC_NMS=agnostic, FUSED_POST_DETECTIONS=False):
            d = postprocess_detections(scores[rows].contiguous(), boxes[rows].contiguous(), K, thresh, cap)
        out.append({j: d[j].cpu().numpy() for j in range(1, K)})
    return out


@pytest.mark.parametrize("agnostic", [False, True])
def test_validation_detections_on_constructed_layers(L, agnostic):
    """the mixed case as a layers dict (cls_prob and bbox_pred carry extra rows past the rois' count, as the combined
    wiring's weak rows do), with im_shapes and without; the cap at 300 (idle) and at 12 (it cuts)"""
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.fast_rcnn.val_detect import validation_detections
    c = D.case("mixed")
    N, K, R = c["n_images"], c["K"], c["rois"].shape[0]
    pad = lambda a: np.concatenate((a, np.full((7, a.shape[1]), 0.25, np.float32)), 0)      # noqa: E731
    layers = {"cls_prob": _t(pad(c["scores"])), "bbox_pred": _t(pad(c["deltas"])),
              "roi-data": (_t(c["rois"]), None, None, None, None)}
    info = _t(c["im_info"])
    removed = 0
    with _cfg_set(cfg.TRAIN, BATCH_SIZE=c["span"]), _cfg_set(cfg.TEST, CLS_AGNOSTIC_NMS=not agnostic):
        for given, cap in ((True, 300), (False, 12)):
            dets, counts = validation_detections(layers, info, N, thresh=0.05, max_per_image=cap,
                                                 im_shapes=c["im_shapes"] if given else None, agnostic=agnostic)
            assert tuple(dets.shape) == (N, K - 1, c["span"], 5) and tuple(counts.shape) == (N, K - 1)
            n = counts.cpu().numpy()
            dets = dets.cpu().numpy()
            want = _reference_route(_t(c["scores"]), _t(_statement("mixed", given)), _t(c["rois"]), N, K, 0.05, cap, agnostic)
            assert not n[0].any() and n[1].sum() > 0 and n[2].sum() > 2
            for i in range(N):
                for j in range(1, K):
                    got = dets[i, j - 1, :n[i, j - 1]]
                    assert got.shape == want[i][j].shape, (given, i, j, got.shape, want[i][j].shape)
                    assert np.array_equal(_bits(got), _bits(want[i][j])), (given, i, j)
            if cap == 12:
                assert n[2].sum() == 12
            else:
                live = int((c["scores"][c["rois"][:, 0] == 2][:, 1:] > 0.05).sum())
                removed += live - int(n[2].sum())
    assert removed > 0                                                 # the NMS is not idle
    # agnostic=None reads the flag
    with _cfg_set(cfg.TRAIN, BATCH_SIZE=c["span"]), _cfg_set(cfg.TEST, CLS_AGNOSTIC_NMS=agnostic):
        d2, c2 = validation_detections(layers, info, N, max_per_image=12)
    assert np.array_equal(c2.cpu().numpy(), n)
    for j in range(K - 1):
        assert np.array_equal(_bits(d2[2, j, :n[2, j]]), _bits(dets[2, j, :n[2, j]]))
    with pytest.raises(ValueError):
        validation_detections(layers, info, N, im_shapes=c["im_shapes"][:2])


# ---------------------------------------------------------------- 3: validate end to end

@pytest.fixture()
def cfg_guard():
    from wssdl_bus_amd.fast_rcnn.config import cfg
    old = (cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG, cfg.TRAIN.USE_BRN)
    yield cfg
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, cfg.SAMPLING_RNG, cfg.TRAIN.USE_BRN = old


def _tensors(obj, prefix=""):
    """every tensor of a (nested) state dict, cloned: {path: tensor}"""
    out = {}
    if isinstance(obj, torch.Tensor):
        out[prefix] = obj.detach().clone()
    elif isinstance(obj, dict):
        for k, v in obj.items():
            out.update(_tensors(v, "%s/%s" % (prefix, k)))
    elif isinstance(obj, (list, tuple)):
        for k, v in enumerate(obj):
            out.update(_tensors(v, "%s/%d" % (prefix, k)))
    return out


def _same_tensors(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def _np_state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _equal_nan(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def test_validate_with_gt_roidb_end_to_end(L, cfg_guard, monkeypatch):
    """the network, image size and batches of test_gpu_validation's end-to-end test.  validate(batches) and
    validate(batches, gt_roidb=gt) from the same state and sampler state; the second pass's own forwards (their
    layers recorded on the way into validation_detections) then go through the reference route of the test above
    (statement boxes, step-by-step post-detection) image by image, and the host scores that all_boxes.  (The layers
    are recorded, not recomputed: a third forward of the same batch was seen to sample other RoIs in one run.)"""
    from wssdl_bus_amd import synthetic
    from wssdl_bus_amd.datasets.voc_eval_bus import DetectionAccumulator, evaluate_detections
    from wssdl_bus_amd.fast_rcnn import train_bus as T
    from wssdl_bus_amd.rpn_msr import anchor_target_layer_tf_bus as atl, proposal_target_layer_tf_bus as ptl
    cfg = cfg_guard
    cfg.SAMPLING_RNG = "device"
    cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = 2, 2
    cfg.TRAIN.USE_BRN = False
    torch.manual_seed(43)
    from wssdl_bus_amd.networks.factory_bus import get_network
    net = get_network("Resnet_train", 18).cuda().to(memory_format=torch.channels_last)
    net.train()
    solver = T.SolverWrapper(net)
    solver.train_step_joint(synthetic.make_batch(2, 2, 320, 480, seed=43))
    batches = [synthetic.make_batch(2, 0, 320, 480, seed=44), synthetic.make_batch(1, 0, 320, 480, seed=45)]
    gt = []
    for b in batches:
        boxes, ng, info = b["gt_boxes"].cpu().numpy(), b["num_gt_boxes"].cpu().numpy(), b["im_info"].cpu().numpy()
        for i in range(boxes.shape[0]):
            gt.append({"boxes": boxes[i, :ng[i], :4] / info[i, 2], "gt_classes": boxes[i, :ng[i], 4].astype(np.int32)})
    assert len(gt) == 3 and all(len(g["gt_classes"]) > 0 for g in gt)

    def snapshot():
        return (_tensors(net.state_dict()), _tensors(solver.optimizer.state_dict()), solver.global_step, net.training,
                int(cfg.TRAIN.IMS_PER_BATCH))

    def unchanged(s):
        now = snapshot()
        return _same_tensors(s[0], now[0]) and _same_tensors(s[1], now[1]) and s[2:] == now[2:]

    state = snapshot()
    calls = (atl._device_calls[0], ptl._device_calls[0])
    np_state = np.random.get_state()

    def rewind():
        atl._device_calls[0], ptl._device_calls[0] = calls
        np.random.set_state(np_state)

    # pass 1: the loss half alone
    plain = solver.validate(batches)
    after_calls = (atl._device_calls[0], ptl._device_calls[0])
    after_np = np.random.get_state()
    assert unchanged(state) and "corloc_list" not in plain and "detections" not in plain

    # pass 2: with the detection half; the layers of its own forwards are kept for the reference route
    from wssdl_bus_amd.fast_rcnn import val_detect
    seen = []

    def recording(layers, im_info, n_images, *args, **kw):
        R = int(layers["roi-data"][0].shape[0])
        seen.append((layers["roi-data"][0].clone(), layers["cls_prob"][:R].clone(), layers["bbox_pred"][:R].clone(),
                     im_info.clone(), int(n_images)))
        return validation_detections(layers, im_info, n_images, *args, **kw)
    validation_detections = val_detect.validation_detections
    rewind()
    monkeypatch.setattr(val_detect, "validation_detections", recording)
    full = solver.validate(batches, gt_roidb=gt)
    monkeypatch.undo()
    assert [n for _, _, _, _, n in seen] == [2, 1]
    assert (atl._device_calls[0], ptl._device_calls[0]) == after_calls and _np_state_equal(np.random.get_state(), after_np)
    assert unchanged(state) and all(p.grad is None for p in net.parameters())
    assert list(full)[:6] == list(T.VAL_TERMS) and full["n_images"] == plain["n_images"] == 3
    for name in T.VAL_TERMS:
        assert np.float64(full[name]).tobytes() == np.float64(plain[name]).tobytes(), name
    assert full["per_image"].dtype == plain["per_image"].dtype and full["per_image"].tobytes() == plain["per_image"].tobytes()
    assert isinstance(full["detections"], DetectionAccumulator) and full["detections"].num_classes == 3
    assert len(full["corloc_list"]) == 3 and len(full["aps"]) == 2 and len(full["froc_curve_pts"]) == 3
    assert full["mean_ap"] == float(np.mean(full["aps"]))

    # the reference route on those forwards: statement boxes, step-by-step post-detection, scored from the host
    K = 3
    all_boxes = [[[] for _ in range(3)] for _ in range(K)]
    first, n_dets = 0, 0
    for rois, scores, deltas, info, n in seen:
        R = int(rois.shape[0])
        deltas = deltas.cpu().numpy()
        live, _ = D.live_rows(rois.cpu().numpy(), n)
        assert bool(D.exp_is_safe(deltas.reshape(R, K, 4)[live][:, :, 2:4]).all())              # the precondition
        boxes = D.statement(rois.cpu().numpy(), deltas, info.cpu().numpy(), n)
        want = _reference_route(scores.contiguous(), _t(boxes), rois, n, K, 0.05, 300, bool(cfg.TEST.CLS_AGNOSTIC_NMS))
        for i in range(n):
            for j in range(1, K):
                all_boxes[j][first + i] = want[i][j]
                n_dets += len(want[i][j])
        first += n
    assert first == 3 and n_dets > 0
    classes = ["__background__", "class_1", "class_2"]
    ref = evaluate_detections(all_boxes, gt, classes)
    print("validate-detect: %d detections, corloc %s, aps %s" % (n_dets, ref["corloc_list"], ref["aps"]))
    assert _equal_nan(full["corloc_list"], ref["corloc_list"])
    assert _equal_nan(full["aps"], ref["aps"]) and _equal_nan(full["mean_ap"], ref["mean_ap"])
    assert _equal_nan(full["froc_curve_pts"], ref["froc_curve_pts"])
    # ... and detection by detection
    dets, counts = full["detections"].gathered(3)
    dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
    for i in range(3):
        for j in range(1, K):
            assert np.array_equal(_bits(dets[i, j - 1, :counts[i, j - 1]]), _bits(all_boxes[j][i])), (i, j)

    # im_shapes: boxes are clipped to the original image given there
    rewind()
    small = solver.validate(batches, gt_roidb=gt, im_shapes=[(200, 300)] * 3, classes=classes, feed_schedule=False)
    d, c = small["detections"].gathered(3)
    d, c = d.cpu().numpy(), c.cpu().numpy()
    kept = np.concatenate([d[i, j, :c[i, j]] for i in range(3) for j in range(K - 1)])
    assert len(kept) > 0 and kept[:, [0, 2]].max() == 299.0 and kept[:, [1, 3]].max() == 199.0 and kept[:, :4].min() >= 0
    assert small["n_images"] == 3 and unchanged(state)

    # wrong lengths
    for kw in (dict(gt_roidb=gt[:2]), dict(gt_roidb=gt + gt[:1]), dict(gt_roidb=gt, im_shapes=[(320, 480)] * 2),
               dict(gt_roidb=gt, im_shapes=[(320, 480)] * 4), dict(gt_roidb=gt, classes=classes[:2])):
        rewind()
        with pytest.raises(ValueError):
            solver.validate(batches, **kw)
        assert unchanged(state)
    solver.check_flags()


# ---------------------------------------------------------------- 4: argument validation

def test_export_rejects_invalid_arguments(L):
    from wssdl_bus_amd import _lib
    c = D.case("one_row")
    K = c["K"]
    rois, deltas, info, bounds = _t(c["rois"]), _t(c["deltas"]), _t(c["im_info"]), _t(c["bounds"])
    out = torch.full((3, 4 * K), SENTINEL, device=DEV)
    p = _lib.ptr
    null = ctypes.c_void_p(None)

    def call(rois_p=p(rois), deltas_p=p(deltas), R=1, K=K, info_p=p(info), stride=4, n=1, boxes_p=p(out)):
        return L.wssdl_decode_detections(rois_p, deltas_p, R, K, info_p, stride, n, p(bounds), boxes_p, _lib.stream())
    bad = _lib.ERR_INVALID_ARGUMENT
    assert call(R=-1) == bad
    assert call(K=1) == bad and call(K=66) == bad
    assert call(n=0) == bad and call(n=-1) == bad
    assert call(stride=2) == bad
    assert call(rois_p=null) == bad and call(deltas_p=null) == bad and call(info_p=null) == bad and call(boxes_p=null) == bad
    assert call(boxes_p=ctypes.c_void_p(out.data_ptr() + 4)) == bad           # not 16-byte aligned
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                      # nothing was launched
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out[:1]), _bits(_statement("one_row", True))) and bool((out[1:] == SENTINEL).all())
