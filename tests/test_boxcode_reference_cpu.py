"""No GPU: the statements of tests/boxcode_reference.py (proposal decode, anchor targets, RoI targets) checked against
everything that is known without the device -- their own guards, the f64 evaluations' counted bounds, the NumPy oracle
and the committed goldens within the budgets of the oracle's f32 np.exp / np.log, the filter-edge anchors, and the
mutants of the proposal statement that the cases must be able to tell from it (> for >=, the filter before the clip,
NumPy's f32 exp, and a faithful exponential one ulp off)."""
import numpy as np
import pytest

import boxcode_reference as B
from conftest import load_golden
from oracle import np_oracle as O

U = B.U


def ulp_diff_f32(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, np.int64(-2 ** 31) - a, a)
    b = np.where(b < 0, np.int64(-2 ** 31) - b, b)
    return np.abs(a - b)


def _anchor_args(c):
    return (c["gt_boxes"], c["num_gt"], c["im_info"], c["n_images"], c["n_out"], c["H"], c["W"], c["dataset"], 16, c["scales"])


def _roi_rows(c, norm):
    """the rows the reference returns for a RoI case (all of its candidates), with its labels and targets"""
    over = dict(c["cfg"])
    if norm:
        over.update(BBOX_NORMALIZE_TARGETS_PRECOMPUTED=True, BBOX_NORMALIZE_MEANS=B.ROI_NORM[0], BBOX_NORMALIZE_STDS=B.ROI_NORM[1])
    return O.proposal_target_layer(c["rois"], c["gt_boxes"], c["num_gt"], c["K"], c["train"], False,
                                   rng=np.random.RandomState(c["seed"]), cfg=over)


# ---------------------------------------------------------------- the guards

def test_base_anchors_are_the_oracles():
    for scales in (B.SCALES, B.SMALL_SCALES):
        assert np.array_equal(B.generate_anchors(scales=scales), O.generate_anchors(scales=np.array(scales)))
    assert np.array_equal(B.shifted_anchors(5, 7), O.shifted_anchors(5, 7, 16, O.generate_anchors()))
    assert np.array_equal(B.generate_anchors(), load_golden("anchors")["a_8_16_32"])


def test_log_guard_rejects_a_rounding_midpoint():
    f = np.float32(-0.3712)
    mid = (np.float64(f) + np.float64(np.nextafter(f, np.float32(0)))) / 2.0
    assert not B.log_value_is_safe(mid) and not B.log_value_is_safe(mid + 3 * np.spacing(mid))
    assert B.log_value_is_safe(np.float64(f)) and B.log_value_is_safe(0.0) and B.log_value_is_safe(mid + 6 * np.spacing(mid))
    pos = -mid                                                         # the same on the positive side
    assert not B.log_value_is_safe(pos) and B.log_value_is_safe(pos - 6 * np.spacing(pos)) and bool(B.log_is_safe(1.0))


@pytest.mark.parametrize("name", B.PROPOSAL_CASES)
def test_proposal_cases_pass_their_guards_with_nothing_excluded(name):
    c = B.proposal_case(name)
    assert c["excluded"] == 0 and c["M"] == c["H"] * c["W"] * 9
    sizes = c["pred"].reshape(-1, 4)[:, 2:4]
    assert float(np.abs(sizes[sizes < 80]).max()) <= 8.0
    assert int((sizes > 88.73).sum()) >= 2                             # exp overflows f32 to inf
    for from_logits in (False, True):
        args = B.proposal_exp_arguments(c, from_logits)
        assert args.size == 2 * c["N"] * c["M"] * (2 if from_logits else 1)
        assert bool(B.exp_is_safe(args).all())                         # every argument, none left out
        st = B.proposal_stated(name, from_logits)
        for n in range(c["N"]):
            assert len(np.unique(st["scores"][n])) == c["M"]           # pairwise distinct: the order is defined
            both = st["boxes"][n][(sizes.reshape(c["N"], -1, 2)[n] > 88.73).all(1)]
            assert (both[:, 0] == 0).all() and (both[:, 2] == c["im_info"][n, 1] - 1).all()     # the clip brings both corners back
        assert np.isfinite(st["boxes"]).all()
    if c["topn"]:
        assert int(B.proposal_stated(name, False)["valid"].sum(1).min()) > c["topn"][0] > c["topn"][1]
    assert (c["M"] < 2048) == (name != "over_one_run") and (name != "over_one_run" or c["M"] - 2048 == 112)


@pytest.mark.parametrize("name", B.ANCHOR_CASES)
def test_anchor_cases_pass_their_guards_with_nothing_excluded(name):
    c = B.anchor_case(name)
    _, _, largs = B.anchor_targets_evaluate_f64(*_anchor_args(c))
    inside, arg = B.anchor_assignment(c["gt_boxes"], c["num_gt"], c["im_info"], c["n_images"], c["H"], c["W"], c["dataset"], 16, c["scales"])
    live = ~np.isnan(largs)
    assert c["excluded"] == 0 and np.array_equal(live.all(2), inside) and np.array_equal(live.any(2), arg >= 0)
    assert bool(B.log_is_safe(largs[live]).all())
    assert bool(inside.any(1).all()) != name.endswith("_outside")      # at least one inside anchor per supervised image
    used = [{int(k) for k in arg[n][inside[n]]} for n in range(c["n_images"])]
    for n, u in enumerate(used):                                       # the arg-max runs over the admitted rows only
        assert not u or max(u) < B.admitted_rows(c["gt_boxes"][n], c["num_gt"][n], c["dataset"])
    if c["special"]:
        # the special rows are still what they are called (a redraw's jitter would have undone two of them) ...
        thin, big, dup = c["special"]
        for n in range(c["n_images"]):
            g, (h, w) = c["gt_boxes"][n], c["im_info"][n, :2]
            assert g[thin, 0] == g[thin, 2] and np.array_equal(g[dup, :4], g[0, :4]) and g[dup, 4] != 0
            assert g[big, 0] < 0 and g[big, 1] < 0 and g[big, 2] > w and g[big, 3] > h
        # ... and which of them give targets: the larger-than-image gt does in every image of the 14 x 17 maps; row 0
        # does where the case has three supervised images, its copy never (equal IoU: the first maximum wins); the
        # 1-px-wide row is no inside anchor's arg-max next to these (that is what the case 14x17_thin is for)
        if name.startswith("14x17"):
            assert all(big in u for u in used) and not any(dup in u or thin in u for u in used)
            assert c["n_images"] == 1 or sum(0 in u for u in used) >= 2
    if name == "14x17_thin":                                           # the 1-px-wide gt, the only admitted row
        g = c["gt_boxes"][0]
        assert g[0, 0] == g[0, 2] and used == [{0}] and int(inside.sum()) > 100
        assert float(np.nanmax(largs[..., 0])) <= 1.0 / 88.0           # gw / ew: 1 px against the narrowest anchor
    print("anchor case %s: %d gt rows redrawn" % (name, c["redrawn"]))


@pytest.mark.parametrize("name", B.ROI_CASES)
def test_roi_cases_pass_their_guards_with_nothing_excluded(name):
    c = B.roi_case(name)
    ref = _roi_rows(c, False)
    assert ref[0].shape[0] == c["R"] and c["excluded"] == 0             # the layer returns every candidate
    fg = ref[1].ravel() > 0
    _, _, largs = B.roi_targets_evaluate_f64(ref[0], fg, c["gt_boxes"], c["num_gt"], c["K"])
    assert np.array_equal(~np.isnan(largs).any(1), fg) and int(fg.sum()) > 0
    assert bool(B.log_is_safe(largs[fg]).all())
    if name == "r70":
        assert float(largs[fg].min()) < 0.15 and float(largs[fg].max()) > 7.0        # gw / ew far from 1, both ways
    assert bool((largs[fg] == 1.0).all(1).any())                      # a proposal that coincides with its gt


# ---------------------------------------------------------------- the statements inside the counted bounds

@pytest.mark.parametrize("from_logits", [False, True])
@pytest.mark.parametrize("name", B.PROPOSAL_CASES)
def test_proposal_statement_lies_inside_the_f64_bound(name, from_logits):
    c = B.proposal_case(name)
    st = B.proposal_stated(name, from_logits)
    b64, bound, s64, sbound = B.proposal_evaluate_f64(c["logits"] if from_logits else c["prob"], c["pred"], c["im_info"],
                                                      from_logits=from_logits)
    err = np.abs(st["boxes"].astype(np.float64) - b64)
    assert bool((err <= bound).all()), float((err - bound).max())
    assert bool((np.abs(st["scores"].astype(np.float64) - s64) <= sbound).all())
    # a bound that binds: the widest box is exp(4) * 736 px, its corner's count about 2.5 U of that
    assert float(bound.max()) < 2.5 * U * np.exp(4.0) * 736 + 1e-4 and (not from_logits or 0 < float(sbound.max()) < 1e-6)


@pytest.mark.parametrize("name", B.ANCHOR_CASES)
def test_anchor_statement_lies_inside_the_f64_bound(name):
    c = B.anchor_case(name)
    st = B.anchor_targets_statement(*_anchor_args(c))
    t64, bound, _ = B.anchor_targets_evaluate_f64(*_anchor_args(c))
    assert st.shape == (c["n_out"], 36, c["H"], c["W"]) and st.dtype == np.float32
    assert bool((np.abs(st.astype(np.float64) - t64) <= bound).all())
    assert float(bound.max()) < 1e-5 and not st[c["n_images"]:].any()


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("name", B.ROI_CASES)
def test_roi_statement_lies_inside_the_f64_bound(name, norm):
    c = B.roi_case(name)
    ref = _roi_rows(c, norm)
    fg = ref[1].ravel() > 0
    nrm = B.ROI_NORM if norm else None
    st = B.roi_targets_statement(ref[0], fg, c["gt_boxes"], c["num_gt"], c["K"], nrm)
    t64, bound, _ = B.roi_targets_evaluate_f64(ref[0], fg, c["gt_boxes"], c["num_gt"], c["K"], nrm)
    assert bool((np.abs(st.astype(np.float64) - t64) <= bound).all())
    assert float(bound.max()) < 1e-4 and not st[~fg].any()


# ---------------------------------------------------------------- the statements against the oracle and the goldens

def _decode_budget(pred, im_info, H, W):
    """|statement - oracle| per corner: the oracle's f32 np.exp is about 2.5 ulp accurate, the statement's exp half an
    ulp: their quotient is within 3 ulp = 6 U, the product with aw rounds once on each side, so pw differs by at most
    8 U pw, half of which reaches a corner, whose own rounding on each side adds 2 U |x|: 4 U pw + 2 U |x|"""
    anc = B.shifted_anchors(H, W)
    d = np.asarray(pred, np.float32).reshape(pred.shape[0], -1, 4).astype(np.float64)
    out = np.zeros(d.shape)
    with np.errstate(all="ignore"):
        for a in (0, 1):
            aw = (anc[:, a + 2] - anc[:, a] + 1.0)[None]
            pw = np.exp(d[:, :, a + 2]) * aw
            pc = d[:, :, a] * aw + anc[None, :, a] + 0.5 * aw
            over = np.isinf(pw.astype(np.float32))
            for col, sign in ((a, -1.0), (a + 2, 1.0)):
                out[:, :, col] = np.where(over, 0.0, 1.001 * (4 * U * pw + 2 * U * np.abs(pc + sign * 0.5 * pw)))
    return out


@pytest.mark.parametrize("name", B.PROPOSAL_CASES)
def test_proposal_statement_agrees_with_the_oracle(name):
    c = B.proposal_case(name)
    st = B.proposal_stated(name, False)
    anchors = O.shifted_anchors(c["H"], c["W"], 16, O.generate_anchors())
    budget = _decode_budget(c["pred"], c["im_info"], c["H"], c["W"])
    for n in range(c["N"]):
        with np.errstate(all="ignore"):
            ref = O.clip_boxes(O.bbox_transform_inv(anchors, c["pred"][n].reshape(-1, 4)), c["im_info"][n, :2])
        assert bool((np.abs(st["boxes"][n].astype(np.float64) - ref) <= budget[n]).all())
    # the fused softmax against the oracle's reshape -> softmax -> reshape
    # The oracle evaluates it in f64 on the exact differences x - max: that is the evaluation proposal_evaluate_f64
    # counts its score bound against (the rounding of t = fl32(x - max) is the bound's term E U |t|), so the same
    # counted bound holds here; two f64 evaluations of it differ by a few 2^-53 relative, far inside the factor 1.001.
    s = O.rpn_cls_prob_reshape(np.array(c["logits"]))[..., 9:].reshape(c["N"], -1)
    assert s.dtype == np.float64
    sbound = B.proposal_evaluate_f64(c["logits"], c["pred"], c["im_info"], from_logits=True)[3]
    assert bool((np.abs(B.proposal_stated(name, True)["scores"].astype(np.float64) - s) <= sbound).all())



def test_proposal_statement_on_the_goldens_has_the_oracles_order():
    g = load_golden("proposal_layer")
    for case in ("res_38x63_train", "res_38x63_test", "vgg_37x62_train", "res_63x100_test"):
        prob, pred, info = g[case + "/prob"], g[case + "/pred"], g[case + "/im_info"]
        N, H, W = prob.shape[:3]
        pre, post = (12000, 2000) if bool(g[case + "/is_training"]) else (6000, 300)
        st = B.proposal_statement(prob, pred, info)
        assert bool(B.exp_is_safe(pred.reshape(-1, 4)[:, 2:4]).all())
        order = B.candidate_order(st["scores"], st["valid"], pre)
        anchors = O.shifted_anchors(H, W, 16, O.generate_anchors())
        budget = _decode_budget(pred, info, H, W)
        for i in range(N):
            ref = O.proposal_stages_one_image(prob[i], pred[i], info[i], anchors, 9, pre, post, 0.7, 16)
            assert np.array_equal(order[i], ref["order"]) and np.array_equal(st["order"][i][:pre], order[i]), (case, i)
            assert bool((np.abs(st["boxes"][i].astype(np.float64) - ref["decoded"]) <= budget[i]).all())


def test_candidate_order_tie_rule():
    s = np.array([[0.5, 0.25, 0.5, 0.75, 0.5]], np.float32)
    v = np.array([[True, True, True, True, False]])
    assert B.candidate_order(s, v)[0].tolist() == [3, 2, 0, 1]         # equal scores: the higher index first
    assert B.candidate_order(s, v, 2)[0].tolist() == [3, 2]


@pytest.mark.parametrize("name", [n for n in B.ANCHOR_CASES if not n.endswith("_outside")])
def test_anchor_statement_agrees_with_the_oracle(name):
    c = B.anchor_case(name)
    st = B.anchor_targets_statement(*_anchor_args(c))
    score = np.zeros((c["n_out"], c["H"], c["W"], 18), np.float32)
    ref = O.anchor_target_layer_joint(score, c["gt_boxes"], c["num_gt"], c["im_info"], None, True, [16], list(c["scales"]),
                                      c["dataset"], rng=np.random.RandomState(c["seed"]),
                                      cfg=dict(IMS_PER_BATCH=c["n_images"], WS_IMS_PER_BATCH=c["n_out"] - c["n_images"]))
    assert ref[1].shape == st.shape and ulp_diff_f32(st, ref[1]).max() <= 1
    t, e = st.reshape(c["n_out"], 9, 4, -1), ref[1].reshape(c["n_out"], 9, 4, -1)
    assert np.array_equal(t[:, :, :2], e[:, :, :2])


@pytest.mark.parametrize("shape", ["vgg_37x62", "res_38x63", "res_63x100"])
def test_anchor_statement_on_the_goldens(shape):
    g = load_golden("anchor_target_" + shape)
    H, W = int(g["H"]), int(g["W"])
    names = sorted({k.split("/")[0] for k in g.files if "/" in k})
    assert names
    for name in names:
        st = B.anchor_targets_statement(g[name + "/gt_boxes"][None], g[name + "/num_gt"], g[name + "/im_info"][None], 1, 1, H, W,
                                        str(g[name + "/dataset"]))
        e = g[name + "/targets"]
        assert ulp_diff_f32(st, e).max() <= 1, name
        assert np.array_equal(st.reshape(9, 4, H, W)[:, :2], e.reshape(9, 4, H, W)[:, :2]), name
        assert np.array_equal(st, g[name + "/targets_pre"]) or ulp_diff_f32(st, g[name + "/targets_pre"]).max() <= 1


def test_roi_statement_agrees_with_the_oracle_and_the_goldens():
    for name in B.ROI_CASES:
        c = B.roi_case(name)
        for norm in (False, True):
            ref = _roi_rows(c, norm)
            st = B.roi_targets_statement(ref[0], ref[1].ravel() > 0, c["gt_boxes"], c["num_gt"], c["K"], B.ROI_NORM if norm else None)
            assert ulp_diff_f32(st, ref[2]).max() <= 4, (name, norm)                  # np.log f32: about 4 ulp
            if not norm:
                cols = np.arange(12) % 4 < 2
                assert np.array_equal(st[:, cols], ref[2][:, cols]), name              # dx, dy: IEEE operations only
    for file, norm in (("proposal_target", None), ("proposal_target_norm", True)):
        g = load_golden(file)
        nrm = (g["means"], g["stds"]) if norm else None
        for tag in ("alt_train", "joint_train") + (() if norm else ("alt_test", "joint_test")):
            labels = g[tag + "/labels"].ravel()
            rows = g[tag + "/rois"][:labels.size]
            st = B.roi_targets_statement(rows, labels > 0, g["gt_boxes"], g["num_gt"], 3, nrm)
            e = g[tag + "/targets"]
            assert st.shape == e.shape and ulp_diff_f32(st, e).max() <= 4, (file, tag)
            if not norm:
                cols = np.arange(12) % 4 < 2
                assert np.array_equal(st[:, cols], e[:, cols]), (file, tag)


# ---------------------------------------------------------------- the filter-edge anchors and the mutants

EDGED = list(B.EDGED_CASES)


@pytest.mark.parametrize("from_logits", [False, True])
@pytest.mark.parametrize("name", EDGED)
def test_filter_edge_anchors_hold_the_highest_scores(name, from_logits):
    """the k filter-edge anchors of an image hold its k largest scores, so each of them is inside any pre-NMS cut of
    at least k: the device's sorted_index then says of every one whether it was kept"""
    c = B.proposal_case(name)
    st = B.proposal_stated(name, from_logits)
    for n in range(c["N"]):
        mine = {e["anchor"] for e in c["edges"] if e["image"] == n}
        top = np.argsort(-st["scores"][n].astype(np.float64))[:len(mine)]
        assert len(mine) >= 8 and set(top.tolist()) == mine
        kept = [i for i in mine if st["valid"][n, i]]
        assert set(st["order"][n][:len(kept)].tolist()) == set(kept)   # the kept ones head the candidate order


@pytest.mark.parametrize("name", EDGED)
def test_filter_edge_anchors_sit_at_and_one_step_either_side_of_the_edge(name):
    c = B.proposal_case(name)
    assert c["M"] >= 315
    st = B.proposal_stated(name, False)
    loose = B.proposal_statement(c["prob"], c["pred"], c["im_info"], mutant="filter_first")      # the unclipped sizes
    anc32 = B.shifted_anchors(c["H"], c["W"]).astype(np.float32)
    pred = c["pred"].reshape(c["N"], -1, 4)
    after_clip = 0
    for n in range(c["N"]):
        mine = [e for e in c["edges"] if e["image"] == n]
        assert len(mine) >= 8 and {e["kind"] for e in mine} == set(B.EDGE_KINDS), (n, len(mine))
        assert len({e["anchor"] for e in mine}) == len(mine)
    for e in c["edges"]:
        n, i, ax = e["image"], e["anchor"], e["axis"]
        size = (st["bw"], st["bh"])[ax][n, i]
        other = (st["bh"], st["bw"])[ax][n, i]
        ms = st["ms"][n]
        assert other >= ms + 1                                         # the other axis decides nothing

        def stepped(by):
            d = pred[n, i].copy()
            d[2 + ax] = B._unordered(B._ordered(d[2 + ax]) + by)
            return B._one_anchor(anc32, i, d, c["im_info"][n], 16.0)
        if e["kind"] == "at":
            assert size == ms and st["valid"][n, i] and not stepped(-1)[3]
        elif e["kind"] == "below":
            assert size < ms and not st["valid"][n, i] and stepped(+1)[3]
        else:
            assert size > ms and st["valid"][n, i] and stepped(-1)[ax] <= ms
        if e["place"] == "border":
            lim = c["im_info"][n, 1 - ax] - 1
            assert st["boxes"][n, i, 2 + ax] == lim                    # the far corner is clipped ...
            assert (loose["bw"], loose["bh"])[ax][n, i] > size          # ... and only then does the size reach the edge
            after_clip += 1
    assert after_clip >= 2 * c["N"]


def _rejected(c, from_logits, mutant):
    """(values beyond the f64 bound, filter-edge anchors on the wrong side) of a mutant of the statement"""
    x = c["logits"] if from_logits else c["prob"]
    st = B.proposal_stated(c["name"], from_logits)
    mu = B.proposal_statement(x, c["pred"], c["im_info"], from_logits=from_logits, mutant=mutant)
    b64, bound, _, _ = B.proposal_evaluate_f64(x, c["pred"], c["im_info"], from_logits=from_logits)
    beyond = int((np.abs(mu["boxes"].astype(np.float64) - b64) > bound).sum())
    flips = sum(int(mu["valid"][e["image"], e["anchor"]] != st["valid"][e["image"], e["anchor"]]) for e in c["edges"])
    return beyond, flips


@pytest.mark.parametrize("name", EDGED)
def test_mutant_strict_filter_is_rejected(name):
    """> for >=: every 'at' anchor falls out"""
    c = B.proposal_case(name)
    beyond, flips = _rejected(c, False, "gt")
    assert flips == sum(e["kind"] == "at" for e in c["edges"]) > 0 and beyond == 0


@pytest.mark.parametrize("name", EDGED)
def test_mutant_filter_before_clip_is_rejected(name):
    """the filter on the unclipped box: the 'below' anchors at the right / lower border come back in"""
    c = B.proposal_case(name)
    beyond, flips = _rejected(c, False, "filter_first")
    assert flips >= sum(e["kind"] == "below" and e["place"] == "border" for e in c["edges"]) > 0 and beyond == 0


def test_mutant_f32_exp_is_rejected():
    """NumPy's f32 exp for the f64 exp rounded once: over the cases with filter-edge anchors, a decoded value leaves the
    f64 bound or a filter-edge anchor changes sides.  Summed over the cases: which of its values NumPy's f32 exp
    rounds differently depends on the SIMD path NumPy takes on the machine, and an exponential that is off by one ulp
    mostly stays inside the f64 bound (about 1.5 U pw at a corner against the 1 U pw it moves), so this sum rests on
    few values (where this was written: 1 value beyond the bound, 4 edge anchors on the other side, all in
    over_one_run).  test_mutant_faithful_exp_is_rejected below is its companion that no machine changes."""
    beyond = flips = 0
    for name in EDGED:
        for from_logits in (False, True):
            b, f = _rejected(B.proposal_case(name), from_logits, "exp_f32")
            beyond, flips = beyond + b, flips + f
    print("f32 np.exp mutant: %d values beyond the f64 bound, %d filter-edge anchors on the other side" % (beyond, flips))
    assert beyond + flips > 0


@pytest.mark.parametrize("from_logits", [False, True])
@pytest.mark.parametrize("name", EDGED)
def test_mutant_faithful_exp_is_rejected(name, from_logits):
    """the correctly rounded exponential moved one f32 ulp up -- a faithful expf -- is told from the statement by the
    filter-edge anchors of EVERY case: some anchor one delta step below the edge comes back in.  Nothing here depends
    on the machine: the mutant is defined from the f64 exp, whose rounding the guard makes unambiguous."""
    c = B.proposal_case(name)
    beyond, flips = _rejected(c, from_logits, "exp_ulp")
    st = B.proposal_stated(name, from_logits)
    mu = B.proposal_statement(c["logits"] if from_logits else c["prob"], c["pred"], c["im_info"], from_logits=from_logits, mutant="exp_ulp")
    back = [e for e in c["edges"] if e["kind"] == "below" and mu["valid"][e["image"], e["anchor"]]]
    assert flips == len(back) > 0 and not st["valid"][back[0]["image"], back[0]["anchor"]]
