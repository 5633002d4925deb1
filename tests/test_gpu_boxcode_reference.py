"""-m gpu: the three box-coding kernels that feed training -- decode_anchor (csrc/proposal.hip), anchor_targets_kernel
(csrc/anchor_target.hip), roi_targets_kernel (csrc/roi_targets.hip) -- against the NumPy statements of their arithmetic
(tests/boxcode_reference.py), driven through the layers.

Every comparison with a statement is BIT FOR BIT.  That is derived, not measured: the library is built with
-ffp-contract=off, so each f32 / f64 multiply, add and subtract is one IEEE operation on both sides; the divisions are
correctly rounded on both sides; each exponential and logarithm is an f64 exp / log rounded once to f32, and
test_boxcode_reference_cpu.py checks that no such value of any case lies within 4 f64 ulps of an f32 rounding boundary
(a value that did was redrawn by the case's builder), so two faithful f64 implementations round alike.  Labels, sampled
rows and weights stay held to the oracle (oracle/np_oracle.py), as in test_gpu_parity.py."""
import numpy as np
import pytest
import torch

import boxcode_reference as B
from oracle import np_oracle as O
from test_gpu_parity import product_cfg  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

STRIDE = [16, ]


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from wssdl_bus_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------- 1: the proposal layer

@pytest.mark.parametrize("topk_sort", [1, 0])
@pytest.mark.parametrize("from_logits", [False, True])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("name", B.PROPOSAL_CASES)
def test_proposal_layer_equals_the_statement(L, product_cfg, name, train, from_logits, topk_sort):
    """decoded boxes bit for bit, the candidate order exact, the filter-edge anchors in or out as the statement says,
    rois and counts == the oracle's NMS on the STATEMENT's boxes and scores (nothing of the product on the expected
    side), zero padding rows, two runs the same bits.

    topk_sort = 0 decodes in proposal_decode_kernel.  topk_sort = 1 decodes in proposal_decode_runs_kernel where the
    sorted runs fit the suppression matrix they are kept in (proposal.hip, 'sortable': 16384 bytes per image and run
    against 8 * N * topn * pitch, pitch 16 words up to topn = 1024): every case but one_cell, whose topn = 9 sends
    both settings through proposal_decode_kernel; small_run (N = 1, M = 144) is the smallest launch of the runs kernel.

    over_one_run: the TRAIN runs cut the candidates at pre_nms_topN = 500 of about 1800 valid ones (post 40); the TEST
    runs cut nothing, so the order of all valid keys of both sort runs is compared.  A filter-edge anchor is DECIDED
    when the cut cannot hide it: fewer than `cut` valid anchors score above it.  The cases give the edge anchors their
    image's highest scores, so every one is decided in every run; the count printed is of decided anchors only and at
    least 8 per image are asserted."""
    from wssdl_bus_amd import _lib
    from wssdl_bus_amd.fast_rcnn.config import cfg
    from wssdl_bus_amd.rpn_msr.proposal_layer_tf_bus import proposal_layer_padded, _rpn_params
    c = B.proposal_case(name)
    assert bool(B.exp_is_safe(B.proposal_exp_arguments(c, from_logits)).all()) and c["excluded"] == 0       # the precondition
    if c["topn"] and train:
        product_cfg(RPN_PRE_NMS_TOP_N=c["topn"][0], RPN_POST_NMS_TOP_N=c["topn"][1])
    pre, post, thresh, min_size = _rpn_params(train)
    assert not cfg.USE_GPU_NMS and min_size == 16 and thresh == 0.7
    N, M = c["N"], c["M"]
    st = B.proposal_stated(name, from_logits)
    cut = pre if 0 < pre < M else 0
    order = B.candidate_order(st["scores"], st["valid"], cut)
    x = c["logits"] if from_logits else c["prob"]

    def run():
        with _lib.tuned(topk_sort=topk_sort):
            out = proposal_layer_padded(np.array(x), np.array(c["pred"]), np.array(c["im_info"]), train, STRIDE, list(B.SCALES),
                                        debug=True, from_logits=from_logits)
        torch.cuda.synchronize()
        return [_np(t) for t in out]
    rois_p, counts, dec, sidx, scnt = run()
    differ = _bits(dec) != _bits(st["boxes"])
    n_order = n_rows = n_edge = 0
    decided = [0] * N
    want_rois = []
    for i in range(N):
        n = int(scnt[i])
        n_order += int(n != len(order[i]) or not np.array_equal(sidx[i, :min(n, len(order[i]))], order[i][:n]))
        dets = np.hstack((st["boxes"][i][order[i]], st["scores"][i][order[i]][:, None])).astype(np.float32)
        keep = np.asarray(O.nms(dets, thresh), dtype=np.int64)
        keep = keep[:post] if post > 0 else keep
        want = np.hstack((np.full((len(keep), 1), i, np.float32), dets[keep, :4]))
        want_rois.append(want)
        k = int(counts[i])
        n_rows += int(k != len(want) or not np.array_equal(_bits(rois_p[i, :k]), _bits(want)))
        members = set(sidx[i, :n].tolist())
        live = st["scores"][i][st["valid"][i]]
        for e in c["edges"]:
            if e["image"] == i and (cut == 0 or int((live > st["scores"][i, e["anchor"]]).sum()) < cut):
                decided[i] += 1
                assert st["valid"][i, e["anchor"]] == (e["kind"] != "below")
                n_edge += int((e["anchor"] in members) != (e["kind"] != "below"))
    print("proposal %s train=%s from_logits=%s topk_sort=%d cut=%d: %d of %d decoded values differ from the statement, %d of %d "
          "images with another order, %d with other rois, %d of %d decided filter-edge anchors (%d planted) on the wrong side"
          % (name, train, from_logits, topk_sort, cut, int(differ.sum()), differ.size, n_order, N, n_rows, n_edge, sum(decided),
             len(c["edges"])))
    assert not differ.any(), np.argwhere(differ)[:8]
    for i in range(N):
        n = int(scnt[i])
        assert n == len(order[i]) and np.array_equal(sidx[i, :n], order[i]), (i, n, len(order[i]))
        k = int(counts[i])
        assert k == len(want_rois[i]) and np.array_equal(_bits(rois_p[i, :k]), _bits(want_rois[i])), (i, k, len(want_rois[i]))
        assert not _bits(rois_p[i, k:]).any()                                      # the padding rows: +0.0
    assert n_edge == 0
    assert not c["edges"] or min(decided) >= 8, decided
    assert bool(c["edges"]) == (name in B.EDGED_CASES)
    if c["topn"] and train:
        assert all(len(o) == c["topn"][0] for o in order) and int(st["valid"].sum(1).min()) > c["topn"][0]   # the cut cuts
    again = run()
    for a, b in zip((rois_p, counts, dec, scnt), (again[0], again[1], again[2], again[4])):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))                  # two runs, the same bits
    for i in range(N):
        assert np.array_equal(sidx[i, :int(scnt[i])], again[3][i, :int(scnt[i])])


# ---------------------------------------------------------------- 2: the anchor targets

def _anchor_args(c):
    return (c["gt_boxes"], c["num_gt"], c["im_info"], c["n_images"], c["n_out"], c["H"], c["W"], c["dataset"], 16, c["scales"])


@pytest.mark.parametrize("name", B.ANCHOR_CASES)
def test_anchor_targets_equal_the_statement(L, product_cfg, name):
    """bbox_targets of anchor_target_layer_joint (and of anchor_target_layer where every image is supervised) bit for
    bit against the statement; labels and both weight blobs against the oracle with the reference RNG.  The '*_outside'
    cases have no anchor inside any image: the reference raises there, the layer defines it (labels -1, zero targets
    and weights -- see boxcode_reference.anchor_cases) and is held to that."""
    from wssdl_bus_amd.rpn_msr.anchor_target_layer_tf_bus import anchor_target_layer, anchor_target_layer_joint
    c = B.anchor_case(name)
    n_s, n_out, H, W, scales = c["n_images"], c["n_out"], c["H"], c["W"], list(c["scales"])
    want = B.anchor_targets_statement(*_anchor_args(c))
    _, _, largs = B.anchor_targets_evaluate_f64(*_anchor_args(c))
    live = ~np.isnan(largs)
    assert bool(B.log_is_safe(largs[live]).all()) and c["excluded"] == 0                 # the precondition
    outside = name.endswith("_outside")
    assert bool(live.any()) != outside
    score = np.zeros((n_out, H, W, 18), np.float32)
    gt, ng, info = np.array(c["gt_boxes"]), np.array(c["num_gt"]), np.array(c["im_info"])
    product_cfg(SAMPLING_RNG="reference", IMS_PER_BATCH=n_s, WS_IMS_PER_BATCH=n_out - n_s)
    runs = [("joint", anchor_target_layer_joint(score, gt, ng, info, None, True, STRIDE, scales, c["dataset"],
                                                rng=np.random.RandomState(c["seed"])))]
    if n_s == n_out:
        runs.append(("alternating", anchor_target_layer(score, gt, ng, info, None, STRIDE, scales, c["dataset"],
                                                        rng=np.random.RandomState(c["seed"]))))
    for tag, got in runs:
        got = [_np(g) for g in got]
        differ = _bits(got[1]) != _bits(want)
        print("anchor-targets %s %s: %d of %d values differ from the statement (%d with a target)"
              % (name, tag, int(differ.sum()), differ.size, int(2 * live.sum())))
        assert got[1].shape == want.shape == (n_out, 36, H, W)
        assert not differ.any(), np.argwhere(differ)[:8]
        if outside:
            assert got[0].shape == (n_out, 1, 9 * H, W) and bool((got[0] == -1).all())
            assert not _bits(got[2]).any() and not _bits(got[3]).any()
            continue
        ocfg = dict(IMS_PER_BATCH=n_s, WS_IMS_PER_BATCH=n_out - n_s)
        if tag == "joint":
            ref = O.anchor_target_layer_joint(score, gt, ng, info, None, True, STRIDE, scales, c["dataset"],
                                              rng=np.random.RandomState(c["seed"]), cfg=ocfg)
        else:
            ref = O.anchor_target_layer(score, gt, ng, info, None, STRIDE, scales, c["dataset"], rng=np.random.RandomState(c["seed"]))
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), (name, tag)
        assert int((ref[0] == 1).sum()) > 0                                        # the recount has something to count


# ---------------------------------------------------------------- 3: the RoI targets

def _roi_cfg(c, norm):
    over = dict(c["cfg"])
    if norm:
        over.update(BBOX_NORMALIZE_TARGETS_PRECOMPUTED=True, BBOX_NORMALIZE_MEANS=B.ROI_NORM[0], BBOX_NORMALIZE_STDS=B.ROI_NORM[1])
    return over


def _roi_check(tag, c, norm, rows, labels, targets):
    """targets bit for bit against the statement of the returned rows; the guard on those rows' logarithms"""
    fg = labels.ravel() > 0
    nrm = B.ROI_NORM if norm else None
    want = B.roi_targets_statement(rows, fg, c["gt_boxes"], c["num_gt"], c["K"], nrm)
    _, _, largs = B.roi_targets_evaluate_f64(rows, fg, c["gt_boxes"], c["num_gt"], c["K"], nrm)
    live = ~np.isnan(largs)
    assert bool(B.log_is_safe(largs[live]).all())                                  # the precondition
    differ = _bits(targets) != _bits(want)
    print("roi-targets %s %s norm=%s: %d of %d values differ from the statement (%d rows with targets)"
          % (c["name"], tag, bool(norm), int(differ.sum()), differ.size, int(fg.sum())))
    assert targets.shape == want.shape
    assert not differ.any(), np.argwhere(differ)[:8]
    return want, fg


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("name", B.ROI_CASES)
def test_roi_targets_equal_the_statement(L, product_cfg, name, norm):
    from wssdl_bus_amd.rpn_msr.proposal_target_layer_tf_bus import proposal_target_layer, proposal_target_layer_joint
    c = B.roi_case(name)
    over = _roi_cfg(c, norm)
    rois, gt, ng, K, S = np.array(c["rois"]), np.array(c["gt_boxes"]), np.array(c["num_gt"]), c["K"], c["n_images"]
    assert c["excluded"] == 0
    # alternating, reference RNG: rows, labels and weights are the oracle's, the targets the statement's
    product_cfg(SAMPLING_RNG="reference", **over)
    got = [_np(g) for g in proposal_target_layer(rois, gt, ng, K, c["train"], False, rng=np.random.RandomState(c["seed"]))]
    ref = O.proposal_target_layer(rois, gt, ng, K, c["train"], False, rng=np.random.RandomState(c["seed"]), cfg=over)
    assert got[0].shape[0] == c["R"] == ref[0].shape[0]
    for k in (0, 1, 3, 4):
        assert np.array_equal(got[k], ref[k]), k
    want, fg = _roi_check("alternating", c, norm, ref[0], ref[1], got[2])
    assert int(fg.sum()) > 0
    # a proposal that coincides with its gt: every target +0.0, sign included (the bits are all zero)
    coincide = fg & np.array([np.array_equal(r[1:], gt[int(r[0]), j, :4]) for r, j in zip(ref[0], B.roi_assignment(ref[0], gt, ng)[0])])
    assert bool(coincide.any())
    assert not any(want.view(np.int32)[r, 4 * int(ref[1][r, 0]):4 * int(ref[1][r, 0]) + 4].any() for r in np.nonzero(coincide)[0])
    # joint: the last image weak (the only image of r1 stays supervised and a weak image without rois follows)
    n_s = max(S - 1, 1)
    jover = dict(over, IMS_PER_BATCH=n_s, WS_IMS_PER_BATCH=1)
    product_cfg(**jover)
    got = [_np(g) for g in proposal_target_layer_joint(rois, gt, ng, K, c["train"], rng=np.random.RandomState(c["seed"]))]
    ref = O.proposal_target_layer_joint(rois, gt, ng, K, c["train"], rng=np.random.RandomState(c["seed"]), cfg=jover)
    for k in (0, 1, 3, 4):
        assert np.array_equal(got[k], ref[k]), k
    n = ref[1].shape[0]
    _roi_check("joint", c, norm, ref[0][:n], ref[1], got[2])
    # the device-sampled chain, on the rows it drew
    product_cfg(SAMPLING_RNG="device", IMS_PER_BATCH=S, WS_IMS_PER_BATCH=0)
    dev = proposal_target_layer(torch.from_numpy(rois).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(ng).cuda(), K,
                                c["train"], False)
    dr, dl, dt = (_np(t) for t in dev[:3])
    arg, best = B.roi_assignment(dr, gt, ng)
    drawn = dr[:, 0] >= 0
    fg = dl.ravel() > 0
    assert int(drawn.sum()) == c["R"] and not fg[~drawn].any()
    thr = over.get("FG_THRESH", 0.5)
    assert np.array_equal(fg[drawn], best[drawn] >= thr)                           # the labels it gave: fg rows of their arg-max gt's class
    assert np.array_equal(dl.ravel()[fg], gt[dr[fg, 0].astype(int), arg[fg], 4])
    _roi_check("device", c, norm, dr, dl, dt)
