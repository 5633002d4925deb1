"""Pin the CPU oracle (oracle/) against golden vectors produced by the reference's
own code (tests/golden/make_golden.py, make_golden_ref_cython.py) and, where oracle/_ref is
present, against the reference's own Cython kernels directly.  CPU only."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from oracle import c_oracle, np_oracle as O, ref_kernels

# the seeded inputs of the *_vs_reference_cython* tests, shared with the script that pinned the reference's outputs
_spec = importlib.util.spec_from_file_location("make_golden_ref_cython", os.path.join(GOLDEN, "make_golden_ref_cython.py"))
ref_cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_cases)
# the switch sets of make_golden_switches.py (its names of the cfg keys and values; the script only runs the reference
# when it is executed)
_spec = importlib.util.spec_from_file_location("make_golden_switches", os.path.join(GOLDEN, "make_golden_switches.py"))
switch_sets = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(switch_sets)

STRIDE = [16, ]
SCALES = [8, 16, 32]


def groups(npz):
    names = sorted({k.split("/")[0] for k in npz.files if "/" in k})
    return names


# ---------------------------------------------------------------- anchors ---

def test_generate_anchors_golden():
    g = load_golden("anchors")
    assert np.array_equal(O.generate_anchors(scales=[8, 16, 32]), g["a_8_16_32"])
    assert np.array_equal(O.generate_anchors(scales=[4, 8, 16, 32]), g["a_4_8_16_32"])
    assert np.array_equal(O.generate_anchors(scales=2 ** np.arange(3, 6)), g["a_default"])
    # live-code values, not the Matlab comment block (generate_anchors.py:10-35)
    assert O.generate_anchors()[0].tolist() == [-84.0, -40.0, 99.0, 55.0]


def test_shifted_anchor_counts():
    base = O.generate_anchors()
    for (H, W, im_h, im_w, total, inside) in ((37, 62, 600, 1000, 20646, 8151),
                                              (38, 63, 600, 1000, 21546, 8151),
                                              (63, 100, 1000, 1600, 56700, 32276)):
        a = O.shifted_anchors(H, W, 16, base)
        assert a.shape == (total, 4)
        ins = (a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 2] < im_w) & (a[:, 3] < im_h)
        assert ins.sum() == inside


# --------------------------------------------------------------------- IoU ---

def test_bbox_overlaps_golden():
    g = load_golden("bbox_overlaps")
    assert np.array_equal(O.bbox_overlaps(g["boxes"], g["query"]), g["iou"])
    assert np.array_equal(O.bbox_overlaps_ui(g["boxes"], g["query"]), g["ui"])
    assert g["iou"][5, 5] == 1.0 and np.all(g["iou"][:, 6] == 0)


def test_bbox_overlaps_vs_reference_cython():
    """The reference's own Cython IoU on random boxes: live where oracle/_ref is built, and always against its outputs
    pinned in tests/golden/ref_cython_random.npz (digests; tests/golden/make_golden_ref_cython.py)."""
    g = load_golden("ref_cython_random")
    for i, (b, q) in enumerate(ref_cases.bbox_cases()):
        assert ref_cases.digest(b, q) == str(g["bbox/%d/inputs" % i]), i
        iou, ui = O.bbox_overlaps(b, q), O.bbox_overlaps_ui(b, q)
        assert ref_cases.digest(iou) == str(g["bbox/%d/iou" % i]), i
        assert ref_cases.digest(ui) == str(g["bbox/%d/ui" % i]), i
        if ref_kernels.available():
            assert np.array_equal(iou, ref_kernels.bbox_overlaps(b, q))
            assert np.array_equal(ui, ref_kernels.bbox_overlaps_ui(b, q))
    assert O.bbox_overlaps(np.zeros((0, 4)), q).shape == (0, 20)
    assert O.bbox_overlaps(b, np.zeros((0, 4))).shape == (3000, 0)


# --------------------------------------------------------------------- NMS ---

def test_nms_golden():
    g = load_golden("nms")
    for name in groups(g):
        dets = g[name + "/dets"]
        for key in ("keep_07", "keep_03"):
            if name + "/" + key in g.files:
                th = 0.7 if key.endswith("07") else 0.3
                assert O.nms(dets, th) == g[name + "/" + key].tolist(), (name, key)
    assert O.nms(np.zeros((0, 5), np.float32), 0.7) == []     # nms_wrapper.py:16-17


def test_nms_threshold_is_double_compare():
    # IoU of these two boxes is 70/100 -> 0.7f in f32; (double)0.7f < 0.7, so the
    # reference (PyFloat compare, cpu_nms.c:2495) keeps both at thresh 0.7.
    d = np.array([[10, 10, 19, 19, 0.9], [10, 10, 19, 16, 0.8]], dtype=np.float32)
    assert O.nms(d, 0.7) == [0, 1]
    assert O.nms(d, float(np.float32(0.7))) == [0]
    if ref_kernels.available():
        assert ref_kernels.cpu_nms(d, 0.7) == [0, 1]
        assert ref_kernels.cpu_nms(d, float(np.float32(0.7))) == [0]


def test_nms_vs_reference_cython_random():
    """cpu_nms.pyx on random boxes: live where oracle/_ref is built, and always against its pinned keep lists."""
    g = load_golden("ref_cython_random")
    for n, d in ref_cases.cpu_nms_cases():
        assert np.array_equal(d, g["cpu_nms/n%d_dets" % n]), n
        for th in ref_cases.NMS_THRESH:
            got = O.nms(d, th)
            assert got == g[ref_cases.keep_key("cpu_nms", n, th)].tolist(), (n, th)
            if ref_kernels.available():
                assert got == [int(k) for k in ref_kernels.cpu_nms(d, th)]


def test_utils_nms_and_nms_new_golden():
    """f3: the test path calls utils/nms.pyx (`nms` :17-68, fast_rcnn/test_bus.py:366), not cpu_nms.pyx; the
    fixtures hold that file's own outputs (`nms` and the containment variant `nms_new` :70-123)."""
    g = load_golden("nms_utils")
    for name in groups(g):
        dets = g[name + "/dets"] if name + "/dets" in g.files else load_golden("nms")[name + "/dets"]
        for key in [k.split("/")[1] for k in g.files if k.startswith(name + "/") and "dets" not in k]:
            th = int(key[-2:]) / 10.0
            got = O.nms_new(dets, th) if key.startswith("nms_new") else O.nms(dets, th)
            assert got == g[name + "/" + key].tolist(), (name, key)
    assert O.nms_new(np.zeros((0, 5), np.float32), 0.3) == []
    # the containment terms bite: a small box inside a large one has a low IoU and inter / area_small = 1
    d = np.array([[0, 0, 199, 199, 0.9], [50, 50, 69, 69, 0.8], [0, 12, 199, 211, 0.7]], dtype=np.float32)
    assert O.nms(d, 0.99) == [0, 1, 2] and O.nms_new(d, 0.99) == [0, 2]      # box 2: 188/200 = 0.94 of either area
    d[2, 1::2] = [9, 208]                                                      # 191/200 = 0.955 > 0.95
    assert O.nms_new(d, 0.99) == [0]


def test_utils_nms_vs_reference_cython_random():
    """utils/nms.pyx (`nms`, `nms_new`) on random, often nested boxes: live where oracle/_ref/cython_nms.so is built,
    and always against its pinned keep lists."""
    g = load_golden("ref_cython_random")
    live = getattr(ref_kernels, "nms_new", None) is not None
    for n, d in ref_cases.utils_nms_cases():
        assert np.array_equal(d, g["utils_nms/n%d_dets" % n]), n
        for th in ref_cases.NMS_THRESH:
            got, got_new = O.nms(d, th), O.nms_new(d, th)
            assert got == g[ref_cases.keep_key("utils_nms", n, th)].tolist(), (n, th)
            assert got_new == g[ref_cases.keep_key("utils_nms_new", n, th)].tolist(), (n, th)
            if live:
                assert got == [int(k) for k in ref_kernels.nms(d, th)]
                assert got_new == [int(k) for k in ref_kernels.nms_new(d, th)]


# ------------------------------------------------------------ anchor target ---

@pytest.mark.parametrize("shape", ["vgg_37x62", "res_38x63", "res_63x100"])
def test_anchor_target_golden(shape):
    g = load_golden("anchor_target_" + shape)
    H, W = int(g["H"]), int(g["W"])
    score = np.zeros((1, H, W, 18), np.float32)
    for name in groups(g):
        gt = g[name + "/gt_boxes"][None]
        ng = g[name + "/num_gt"]
        ii = g[name + "/im_info"][None]
        ds = str(g[name + "/dataset"])
        pre = O.anchor_target_layer(score, gt, ng, ii, None, STRIDE, SCALES, ds,
                                    cfg=dict(RPN_BATCHSIZE=10 ** 9))
        assert np.array_equal(pre[0].astype(np.int8), g[name + "/labels_pre"]), name
        assert np.array_equal(pre[1], g[name + "/targets_pre"]), name
        rng = np.random.RandomState(int(g[name + "/seed"]))
        fin = O.anchor_target_layer(score, gt, ng, ii, None, STRIDE, SCALES, ds, rng=rng)
        assert np.array_equal(fin[0].astype(np.int8), g[name + "/labels"]), name
        assert np.array_equal(fin[1], g[name + "/targets"]), name
        assert np.array_equal(fin[2], g[name + "/inside_w"]), name
        assert np.array_equal(fin[3], g[name + "/outside_w"]), name
        lab = g[name + "/labels"]
        assert (lab == 1).sum() <= 128 and (lab >= 0).sum() <= 256


def _switch_sets(npz):
    """{switch set: [case, ...]} of a make_golden_switches.py file (keys 'set/case/array')."""
    sets = {}
    for k in npz.files:
        parts = k.split("/")
        if len(parts) == 3:
            sets.setdefault(parts[0], set()).add(parts[1])
    return {s: sorted(c) for s, c in sets.items()}


def test_anchor_target_switches_golden():
    """Non-default cfg.TRAIN switches of the anchor-target layer (make_golden_switches.py): clobbering, the two
    overlap thresholds, the positive weight, the inside weights and the fg fraction / batch size -- the
    reference's labels before and after sub-sampling and its weights, bit for bit; the targets depend on none
    of them (those of anchor_target_res_38x63.npz)."""
    ANCHOR_JOINT, ANCHOR_SWITCHES = switch_sets.ANCHOR_JOINT, switch_sets.ANCHOR_SWITCHES
    g = load_golden("anchor_target_switches")
    base = load_golden("anchor_target_res_38x63")
    H, W = int(g["H"]), int(g["W"])
    score = np.zeros((1, H, W, 18), np.float32)
    sets = _switch_sets(g)
    assert sorted(sets) == sorted(ANCHOR_SWITCHES)
    for sname, cases in sets.items():
        over = dict(ANCHOR_SWITCHES[sname])
        for name in cases:
            k = "%s/%s/" % (sname, name)
            gt, ng, ii = base[name + "/gt_boxes"][None], base[name + "/num_gt"], base[name + "/im_info"][None]
            ds = str(base[name + "/dataset"])
            pre = O.anchor_target_layer(score, gt, ng, ii, None, STRIDE, SCALES, ds,
                                        cfg=dict(over, RPN_BATCHSIZE=10 ** 9))
            assert np.array_equal(pre[0].astype(np.int8), g[k + "labels_pre"]), k
            rng = np.random.RandomState(int(g[k + "seed"]))
            with np.errstate(divide="ignore"):
                fin = O.anchor_target_layer(score, gt, ng, ii, None, STRIDE, SCALES, ds, rng=rng, cfg=over)
            assert np.array_equal(fin[0].astype(np.int8), g[k + "labels"]), k
            assert np.array_equal(fin[1], base[name + "/targets"]), k
            assert np.array_equal(fin[2], g[k + "inside_w"]), k
            assert np.array_equal(fin[3], g[k + "outside_w"]), k
    # the switches reach the fixtures: each set changes something a default run does not produce
    assert (base["FILE04254/labels_pre"] == 0).sum() > 0 and (g["clobber/FILE04254/labels_pre"] == 0).sum() == 0
    assert ((g["overlaps/twenty_fg/labels_pre"] == 1).sum() != (g["overlaps_clobber/twenty_fg/labels_pre"] == 1).sum())
    iw = g["inside_w/twenty/inside_w"].reshape(9, 4, H, W)
    lab = g["inside_w/twenty/labels"].reshape(9, H, W)
    for j, w in enumerate((0.1, 1.0, 0.0, 2.5)):
        assert np.all(iw[:, j][lab == 1] == np.float32(w)) and not iw[:, j][lab != 1].any()
    assert len(np.unique(g["posw_030/FILE04254/outside_w"])) == 3                  # 0, pos and neg weights
    # joint train batch (1 supervised + 2 weak images) with clobbering, a positive weight and inside weights
    j = load_golden("anchor_target_joint")
    score3 = np.zeros((3, H, W, 18), np.float32)
    with np.errstate(divide="ignore"):
        jt = O.anchor_target_layer_joint(score3, j["gt_boxes"], j["num_gt"], j["im_info"], None, True, STRIDE, SCALES,
                                         "SNUBH", rng=np.random.RandomState(int(g["joint/seed"])), cfg=ANCHOR_JOINT)
    assert np.array_equal(jt[0].astype(np.int8), g["joint/labels"])
    assert np.array_equal(jt[1], j["train_targets"])
    assert np.array_equal(jt[2], g["joint/inside_w"]) and np.array_equal(jt[3], g["joint/outside_w"])
    assert np.all(np.isfinite(g["joint/outside_w"])) and not (g["joint/labels"] == 0).any()


def test_rpn_positive_weight_range():
    """The reference asserts 0 < RPN_POSITIVE_WEIGHT < 1 unless it is negative (anchor_target_layer_tf_bus.py:237-238);
    the product's layer checks the same before it launches anything."""
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.rpn_msr.anchor_target_layer_tf_bus import rpn_positive_weight
    saved = cfg.TRAIN.RPN_POSITIVE_WEIGHT
    try:
        for w in (-1.0, -0.5, 1e-9, 0.3, 0.75, 0.999999):
            cfg.TRAIN.RPN_POSITIVE_WEIGHT = w
            assert rpn_positive_weight() == w
        for w in (0.0, 1.0, 1.5, float("nan"), float("inf")):
            cfg.TRAIN.RPN_POSITIVE_WEIGHT = w
            with pytest.raises(ValueError):
                rpn_positive_weight()
    finally:
        cfg.TRAIN.RPN_POSITIVE_WEIGHT = saved


def test_anchor_target_zero_overlap_quirk():
    g = load_golden("anchor_target_res_38x63")
    pre = g["outside_quirk/labels_pre"]
    # a GT box that overlaps no inside anchor turns every zero-overlap inside
    # anchor into fg (anchor_target_layer_tf_bus.py:446-449): thousands of 1s
    assert (pre == 1).sum() > 5000


def test_anchor_target_joint_and_ws_golden():
    g = load_golden("anchor_target_joint")
    gt, ng, ii = g["gt_boxes"], g["num_gt"], g["im_info"]
    score = np.zeros((3, 38, 63, 18), np.float32)
    rng = np.random.RandomState(int(g["seed"]))
    jt = O.anchor_target_layer_joint(score, gt, ng, ii, None, True, STRIDE, SCALES, "SNUBH", rng=rng)
    assert jt[0].shape == (3, 1, 342, 63)
    assert np.array_equal(jt[0].astype(np.int8), g["train_labels"])
    for k, nm in ((1, "train_targets"), (2, "train_inside"), (3, "train_outside")):
        assert np.array_equal(jt[k], g[nm])
    rng = np.random.RandomState(int(g["seed"]))
    jf = O.anchor_target_layer_joint(score[:1], gt[:1], ng[:1], ii[:1], None, False, STRIDE,
                                     SCALES, "SNUBH", rng=rng)
    assert np.array_equal(jf[0].astype(np.int8), g["test_labels"])
    assert np.array_equal(jf[1], g["test_targets"])
    ws = O.anchor_target_layer_ws(score[1:], None, None, None, None, STRIDE, SCALES)
    assert np.array_equal(ws[0].astype(np.int8), g["ws_labels"])
    assert tuple(g["ws_shape"]) == ws[1].shape and not ws[1].any() and not ws[3].any()


# ----------------------------------------------------------- proposal layer ---

@pytest.mark.parametrize("case", ["res_38x63_train", "res_38x63_test", "vgg_37x62_train",
                                  "res_63x100_test"])
def test_proposal_layer_golden(case):
    g = load_golden("proposal_layer")
    rois = O.proposal_layer(g[case + "/prob"], g[case + "/pred"], g[case + "/im_info"],
                            bool(g[case + "/is_training"]), False, STRIDE, SCALES)
    assert rois.dtype == np.float32
    assert np.array_equal(rois, g[case + "/rois"])


def test_box_transforms_golden():
    g = load_golden("bbox_transform")
    assert np.array_equal(O.bbox_transform(g["ex"], g["gt"]), g["t_f64_f32"])
    assert np.array_equal(O.bbox_transform(g["ex"].astype(np.float32), g["gt"]), g["t_f32_f32"])
    inv = O.bbox_transform_inv(g["ex"], g["deltas"])
    assert np.array_equal(inv, g["inv"])
    assert np.array_equal(O.clip_boxes(inv, np.array([400, 450], np.float32)), g["clipped"])
    assert O.bbox_transform_inv(np.zeros((0, 4)), np.zeros((0, 4), np.float32)).shape == (0, 4)


# ---------------------------------------------------------- proposal target ---

def test_proposal_target_golden():
    g = load_golden("proposal_target")
    rois, gt, ng = g["rois_in"], g["gt_boxes"], g["num_gt"]
    names = ("rois", "labels", "targets", "inside", "outside")
    for tag, args in (("alt_train", (True, False)), ("alt_ws", (True, True)),
                      ("alt_test", (False, False))):
        rng = np.random.RandomState(int(g["seed_alt"]))
        o = O.proposal_target_layer(rois, gt, ng, 3, args[0], args[1], rng=rng)
        for k, nm in enumerate(names):
            assert np.array_equal(o[k], g["%s/%s" % (tag, nm)]), (tag, nm)
    for tag, tr in (("joint_train", True), ("joint_test", False)):
        rng = np.random.RandomState(int(g["seed_joint"]))
        o = O.proposal_target_layer_joint(rois, gt, ng, 3, tr, rng=rng,
                                          cfg=dict(IMS_PER_BATCH=1, WS_IMS_PER_BATCH=1))
        for k, nm in enumerate(names):
            assert np.array_equal(o[k], g["%s/%s" % (tag, nm)]), (tag, nm)
    # joint/train: 128 sampled rows for the supervised image + every roi of the weak one
    assert g["joint_train/labels"].shape[0] == 128
    assert g["joint_train/rois"].shape[0] == 128 + int((rois[:, 0] == 1).sum())


def test_proposal_target_golden_with_precomputed_normalisation():
    """cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED = True (proposal_target_layer_tf_bus.py:221-224) with the
    reference's own means / stds (config.py:182-183): the reference's outputs, bit for bit."""
    g = load_golden("proposal_target_norm")
    rois, gt, ng = g["rois_in"], g["gt_boxes"], g["num_gt"]
    names = ("rois", "labels", "targets", "inside", "outside")
    over = dict(BBOX_NORMALIZE_TARGETS_PRECOMPUTED=True, BBOX_NORMALIZE_MEANS=tuple(g["means"]),
                BBOX_NORMALIZE_STDS=tuple(g["stds"]))
    o = O.proposal_target_layer(rois, gt, ng, 3, True, False, rng=np.random.RandomState(int(g["seed_alt"])), cfg=over)
    for k, nm in enumerate(names):
        assert np.array_equal(o[k], g["alt_train/%s" % nm]), nm
    o = O.proposal_target_layer_joint(rois, gt, ng, 3, True, rng=np.random.RandomState(int(g["seed_joint"])),
                                      cfg=dict(over, IMS_PER_BATCH=1, WS_IMS_PER_BATCH=1))
    for k, nm in enumerate(names):
        assert np.array_equal(o[k], g["joint_train/%s" % nm]), nm
    # the switch matters: the plain fixtures' targets differ, and by exactly the scaling (means are zero)
    p = load_golden("proposal_target")
    assert not np.array_equal(p["alt_train/targets"], g["alt_train/targets"])
    fg = p["alt_train/targets"] != 0
    scaled = (p["alt_train/targets"].astype(np.float64).reshape(-1, 3, 4) / g["stds"]).reshape(p["alt_train/targets"].shape)
    assert np.array_equal(scaled.astype(np.float32)[fg], g["alt_train/targets"][fg])


def test_proposal_target_switches_golden():
    """Non-default thresholds, fractions, batch sizes and inside weights of the proposal-target layer
    (make_golden_switches.py), alternating mode and joint mode (the latter with precomputed normalisation on):
    the reference's outputs bit for bit.  'overlap' has FG_THRESH < BG_THRESH_HI, where a row can be drawn
    twice, once as fg and once as bg."""
    PROPOSAL_SWITCHES, PT_NAMES = switch_sets.PROPOSAL_SWITCHES, switch_sets.PT_NAMES
    g = load_golden("proposal_target_switches")
    p = load_golden("proposal_target")
    rois, gt, ng = p["rois_in"], p["gt_boxes"], p["num_gt"]
    norm = dict(BBOX_NORMALIZE_TARGETS_PRECOMPUTED=True, BBOX_NORMALIZE_MEANS=tuple(g["means"]),
                BBOX_NORMALIZE_STDS=tuple(g["stds"]))
    sets = _switch_sets(g)
    assert sorted(sets) == sorted(PROPOSAL_SWITCHES)
    for sname in sets:
        over = dict(PROPOSAL_SWITCHES[sname])
        o = O.proposal_target_layer(rois, gt, ng, 3, True, False, rng=np.random.RandomState(int(g["seed_alt"])),
                                    cfg=over)
        for k, nm in enumerate(PT_NAMES):
            assert np.array_equal(o[k], g["%s/alt_train/%s" % (sname, nm)]), (sname, nm)
        o = O.proposal_target_layer_joint(rois, gt, ng, 3, True, rng=np.random.RandomState(int(g["seed_joint"])),
                                          cfg=dict(over, IMS_PER_BATCH=1, WS_IMS_PER_BATCH=1, **norm))
        for k, nm in enumerate(PT_NAMES):
            assert np.array_equal(o[k], g["%s/joint_train/%s" % (sname, nm)]), (sname, nm)
    # what the fixtures pin: the repeat of the overlapping bands, the one fg row per image at FG_THRESH = 1.0,
    # more rows than BATCH_SIZE 64 allows nowhere, and outside weights that follow `inside > 0` per channel
    r = g["overlap/alt_train/rois"]
    img1 = [tuple(x) for x in r[r[:, 0] == 1].tolist()]
    assert len(img1) - len(set(img1)) == 6
    lab = g["fg_one/alt_train/labels"][:, 0]
    assert (lab > 0).sum() == 2
    assert g["half_64/alt_train/labels"].shape[0] <= 2 * 64 and g["big_batch/alt_train/labels"].shape[0] > 2 * 128
    fg = g["inside_w/alt_train/labels"][:, 0] > 0
    iw = g["inside_w/alt_train/inside"][fg].reshape(-1, 3, 4)
    ow = g["inside_w/alt_train/outside"][fg].reshape(-1, 3, 4)
    cls = g["inside_w/alt_train/labels"][fg, 0].astype(int)
    for q in range(cls.size):
        assert np.array_equal(iw[q, cls[q]], np.float32([0.1, 0.0, 2.0, -0.5]))
        assert np.array_equal(ow[q, cls[q]], np.float32([1, 0, 1, 0]))


def test_oracle_roundtrip_c_binding_shapes():
    top, arg = c_oracle.roi_pool_forward(np.zeros((1, 4, 4, 2), np.float32),
                                         np.zeros((0, 5), np.float32), 7, 7, 1.0 / 16)
    assert top.shape == (0, 7, 7, 2) and arg.dtype == np.int32
