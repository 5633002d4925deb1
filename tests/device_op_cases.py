"""The one table of device-op cases: CASES, name -> (builder, min_allocations).

Every case is a small callable built from inputs the suite already has.  builder() returns dict(fn=, inputs=, ...):
fn(inputs) runs the op through its Python wrapper on the tensors of `inputs` (a dict or a sequence) and returns a nested
result of tensors, arrays and plain values.  Two harnesses run every case:

  test_gpu_memory_contracts.py   guard bands and poison (guarded_alloc.py); min_allocations is its vacuity floor
  test_gpu_stream_order.py       the stream-order contract (stream_order.py)

Regions a contract leaves undefined are excluded through the one table UNDEFINED below and nowhere else; each entry
quotes the sentence of include/wssdl_bus_hip.h or of the wrapper's docstring that leaves the region undefined.

Importing this module needs no GPU and builds nothing: builders touch the device, the table does not."""
import contextlib

import numpy as np
import torch

import boxcode_reference as B
import decode_reference as DR
import eval_cases as EC
import groupnorm_reference as GR
import headconv_reference as HC
import guarded_alloc as ga
import loss_reference as LR
import mil_pool_reference as MP
import network_reference as NR
import recall_cases as RC
import renorm_reference as RN
import roi_align_reference as RA
import rowbn_reference as RB
import validation_cases as V
from conftest import load_golden

DEV = "cuda"
CASES = {}                     # name -> (builder, min_allocations)
STRIDE = [16, ]


def _dets_up_to_counts(result):
    """(dets [..., P, 5], counts [...]) -> (every class's rows below its count, counts); a negative count (the overflow flag
    of the batched ops) has no rows"""
    dets, counts = result
    n = counts.reshape(-1).cpu().tolist()
    d = dets.reshape(len(n), dets.shape[-2], 5)
    return [d[k, :max(c, 0)] for k, c in enumerate(n)], counts


# (case prefixes, region, the contract's sentence, result -> its defined part)
UNDEFINED = (
    (("post-detect-", "val-detect-"), "dets[..., counts:, :]",
     "Rows of dets at and beyond a class's count are not written: they keep what the caller's buffer held.", _dets_up_to_counts),
    (("rowbn-join-identity-",), "stats_s (the fourth result) of a join without a second norm",
     "stats_s unwritten without bns", lambda r: r[:3] + (None,) + r[4:]),
)


def _defined_for(name):
    cuts = [cut for prefixes, _region, _sentence, cut in UNDEFINED if name.startswith(prefixes)]
    if not cuts:
        return None

    def apply(result):
        for cut in cuts:
            result = cut(result)
        return result
    return apply


def case(name, min_allocations):
    def deco(builder):
        assert name not in CASES, name
        CASES[name] = (builder, min_allocations)
        return builder
    return deco


def _t(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared cases are read-only arrays)
    return t if dtype is None else t.to(dtype)


@contextlib.contextmanager
def _cfg(**kw):
    """Keys of cfg.TRAIN (or the top-level keys named below) for one case; everything is restored."""
    from wssdl_bus_amd.fast_rcnn.config import cfg
    saved_top, saved_train, saved_test = dict(cfg), dict(cfg.TRAIN), dict(cfg.TEST)
    try:
        for k, v in kw.items():
            if k in cfg.TRAIN:
                cfg.TRAIN[k] = v
            else:
                cfg[k] = v
        yield cfg
    finally:
        cfg.TRAIN.clear()
        cfg.TRAIN.update(saved_train)
        cfg.TEST.clear()
        cfg.TEST.update(saved_test)
        for k in list(cfg):
            if k not in saved_top:
                del cfg[k]
        for k, v in saved_top.items():
            if k not in ("TRAIN", "TEST"):
                cfg[k] = v


def _flags():
    from wssdl_bus_amd.roi_pooling_layer import roi_pooling_op
    return roi_pooling_op.flags_raised


# ------------------------------------------------------------------------------------------------------------ NMS ---
# n: 1, one under and one over a 64-wide mask word, one sorted run of 2048 plus one.  thresh 1.0001 suppresses nothing:
# keep is then the ranking.  max_keep 64 / 65: the sweep's kept list is written in chunks of 64 next to a keep output of
# exactly max_keep entries.

def _nms_dets(n):
    rs = np.random.RandomState(7000 + n)
    xy = rs.uniform(0, 200, size=(n, 2))
    wh = rs.uniform(8, 120, size=(n, 2))
    score = (rs.permutation(n) + 1.0) / (n + 1.0)
    if n > 8:
        score[5] = score[3]                             # a tie: the higher input index goes first
        xy[7], wh[7] = xy[2], wh[2]                     # a duplicate box
    return np.hstack((xy, xy + wh, score[:, None])).astype(np.float32)


def _nms_case(n, thresh, max_keep, rule, topk_sort):
    def build():
        from wssdl_bus_amd import _lib
        from wssdl_bus_amd.nms.hip_nms import hip_nms

        def fn(inp):
            with _lib.tuned(topk_sort=topk_sort):
                return hip_nms(inp["dets"], thresh, max_keep, rule)
        return dict(fn=fn, inputs={"dets": _t(_nms_dets(n))})
    return build


for _n in (1, 63, 65, 2049):
    for _th in (0.7, 1.0001):
        for _mk in (None, 1, 64, 65):
            for _rule in ("nms", "nms_new"):
                for _ts in (1, 0):
                    case("nms-%s-n%d-t%s-k%s-sort%d" % (_rule, _n, _th, _mk, _ts), 3)(_nms_case(_n, _th, _mk, _rule, _ts))


# ------------------------------------------------------------------------------------------------- proposal layer ---

def _proposal_inputs(name, empty_image):
    c = B.proposal_case(name)
    info = np.array(c["im_info"])
    if empty_image:
        info[-1, :2] = 8.0                              # every box of the last image fails the min-size filter
    return c, {"prob": _t(c["prob"]), "logits": _t(c["logits"]), "pred": _t(c["pred"]), "info": _t(info)}


def _proposal_case(name, train, padded, from_logits, tuning, empty_image):
    def build():
        from wssdl_bus_amd import _lib
        from wssdl_bus_amd.rpn_msr.proposal_layer_tf_bus import proposal_layer, proposal_layer_from_score
        c, inputs = _proposal_inputs(name, empty_image)
        over = dict(PADDED_ROIS=bool(padded))
        if c["topn"] and train:
            over.update(RPN_PRE_NMS_TOP_N=c["topn"][0], RPN_POST_NMS_TOP_N=c["topn"][1])

        def fn(inp):
            with _cfg(**over), _lib.tuned(**tuning):
                layer = proposal_layer_from_score if from_logits else proposal_layer
                rois = layer(inp["logits" if from_logits else "prob"], inp["pred"], inp["info"], train, False,
                             STRIDE, list(B.SCALES))
                counts = getattr(rois, "_wssdl_counts_dev", None)
                return rois, counts, getattr(rois, "_wssdl_counts", None)
        return dict(fn=fn, inputs=inputs, flags=True)
    return build


_PROPOSAL_TUNINGS = (("sort1-fused1", dict(topk_sort=1, nms_fused=1)), ("sort0-fused1", dict(topk_sort=0, nms_fused=1)),
                     ("sort1-fused0", dict(topk_sort=1, nms_fused=0)), ("sort0-fused0", dict(topk_sort=0, nms_fused=0)),
                     ("sort1-onepass", dict(topk_sort=1, nms_one_pass=1)))
for _name, _empty in (("one_cell", False), ("below_one_run", False), ("below_one_run", True), ("over_one_run", False)):
    for _train in (True, False):
        for _padded in (False, True):
            for _tag, _tu in _PROPOSAL_TUNINGS:
                _logits = _tag in ("sort0-fused0", "sort1-onepass")         # the fused softmax in front of the decode
                case("proposal-%s%s-%s-%s-%s%s" % (_name, "-empty" if _empty else "", "train" if _train else "test",
                                                     "padded" if _padded else "compact", _tag, "-logits" if _logits else ""), 3)(
                    _proposal_case(_name, _train, _padded, _logits, _tu, _empty))


# ------------------------------------------------------------------------------------------------- anchor targets ---

def _anchor_case(name, joint, device_rng):
    def build():
        from wssdl_bus_amd.rpn_msr import anchor_target_layer_tf_bus as atl
        c = B.anchor_case(name)
        n_s, n_out = c["n_images"], c["n_out"]
        assert joint or n_s == n_out               # the single-mode layer: every image supervised
        shape = (n_out, c["H"], c["W"])
        over = dict(SAMPLING_RNG="device" if device_rng else "reference", IMS_PER_BATCH=n_s, WS_IMS_PER_BATCH=n_out - n_s,
                    RPN_BATCHSIZE=16)              # 16 of up to 2142 anchors: both draws have something to drop

        def fn(inp):
            with _cfg(**over):
                atl._device_calls[0] = 0           # the device draw's seed folds the call count in
                rng = None if device_rng else np.random.RandomState(c["seed"])
                if joint:
                    return atl.anchor_target_layer_joint(shape, inp["gt"], inp["ng"], inp["info"], None, True, STRIDE,
                                                         list(c["scales"]), c["dataset"], rng=rng)
                return atl.anchor_target_layer(shape, inp["gt"], inp["ng"], inp["info"], None, STRIDE, list(c["scales"]),
                                               c["dataset"], rng=rng)
        return dict(fn=fn, inputs={"gt": _t(c["gt_boxes"]), "ng": _t(c["num_gt"]), "info": _t(c["im_info"])})
    return build


for _name, _joint in (("1x1_small", False), ("1x1_small", True), ("1x1_outside", True), ("3x4_small_fg", False),
                      ("3x4_small_joint", True), ("14x17_fg", False), ("14x17_joint", True), ("14x17_all", False)):
    for _dev in (False, True):
        case("anchor-%s-%s-%s" % (_name, "joint" if _joint else "single", "device" if _dev else "reference"), 5)(
            _anchor_case(_name, _joint, _dev))


# ----------------------------------------------------------------------------------------------- proposal targets ---

def _roi_target_case(name, joint, no_gt_image):
    def build():
        from wssdl_bus_amd.rpn_msr import proposal_target_layer_tf_bus as ptl
        c = B.roi_case(name)
        S = c["n_images"]
        gt, ng = np.array(c["gt_boxes"]), np.array(c["num_gt"])
        if no_gt_image:
            gt[-1], ng[-1] = 0.0, 0                # the last image: no ground truth at all
        # 24 rows per image: r70 and r257 give an image more candidates than that (the draw drops some), r1 fewer (padding)
        over = dict(c["cfg"], SAMPLING_RNG="device", BATCH_SIZE=24, IMS_PER_BATCH=max(S - 1, 1) if joint else S,
                    WS_IMS_PER_BATCH=1 if joint else 0)

        def fn(inp):
            with _cfg(**over):
                ptl._device_calls[0] = 0
                if joint:
                    return ptl.proposal_target_layer_joint(inp["rois"], inp["gt"], inp["ng"], c["K"], True)
                return ptl.proposal_target_layer(inp["rois"], inp["gt"], inp["ng"], c["K"], c["train"], False)
        return dict(fn=fn, inputs={"rois": _t(c["rois"]), "gt": _t(gt), "ng": _t(ng)})
    return build


for _name in B.ROI_CASES:
    for _joint in (False, True):
        case("roi-targets-%s-%s" % (_name, "joint" if _joint else "single"), 4)(_roi_target_case(_name, _joint, False))
case("roi-targets-r70-single-no-gt-image", 4)(_roi_target_case("r70", False, True))
case("roi-targets-r257-single-no-gt-image", 4)(_roi_target_case("r257", False, True))


# ------------------------------------------------------------------------------------------------------- RoIAlign ---

def _align_case(name, op):
    def build():
        from wssdl_bus_amd.roi_pooling_layer import roi_align_op as ra
        c = RA.make_case(name)
        aligned = name != "axes"
        args = (c["PH"], c["PW"], c["scale"], c["S"], aligned)

        def fn(inp):
            if op == "tables":
                return ra.roi_align_tables(inp["rois"], c["shape"], *args)
            if op == "forward":
                return ra.roi_align(inp["data"], inp["rois"], *args)
            if op == "grad":
                return ra.roi_align_grad(c["shape"], inp["rois"], inp["grad"], *args)
            data = inp["data"].detach().clone().requires_grad_(True)
            top = ra.roi_align_autograd(data, inp["rois"], *args)
            top.backward(inp["grad"])
            return top.detach(), data.grad
        return dict(fn=fn, inputs={"data": _t(c["data"]), "rois": _t(c["rois"]), "grad": _t(c["grad"])})
    return build


for _name in ("mixed", "axes", "empty"):
    for _op, _floor in (("tables", 1), ("forward", 2), ("grad", 3), ("autograd", 4)):
        if _name == "empty" and _op in ("forward",):
            _floor = 1                      # R = 0: top has no bytes, the table buffer is the one allocation
        if _name == "empty" and _op in ("grad", "autograd"):
            _floor = 3
        case("roi-align-%s-%s" % (_name, _op), _floor)(_align_case(_name, _op))



# ------------------------------------------------------------------------------------------------ RoI max pooling ---
# Every RoI list holds dead rows (batch index -1), an index >= N, a RoI smaller than a cell and one covering the map,
# and no RoI that reaches outside the image (none raises the overflow flag).

def _pool_rois(seed, R, N, H, W):
    rs = np.random.RandomState(seed)
    im_h, im_w = 16.0 * H - 8, 16.0 * W - 8
    x = np.sort(rs.uniform(0, im_w - 1, size=(R, 2)), axis=1)
    y = np.sort(rs.uniform(0, im_h - 1, size=(R, 2)), axis=1)
    rois = np.stack([rs.randint(0, N, size=R).astype(np.float64), x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1)
    special = [(-1, 4, 4, 40, 40), (N, 4, 4, 40, 40), (0, 20, 20, 24, 23), (N - 1, 0, 0, im_w - 1, im_h - 1),
               (-1, 0, 0, 0, 0), (0, 30, 10, 12, 5)]                  # (the last: end < start)
    at = rs.permutation(R)[:len(special)]
    for k, row in zip(at, special[:R]):
        rois[k] = row
    if R == 1:
        rois[0] = special[3]
    return rois.astype(np.float32)


def _pool_data(seed, shape):
    rs = np.random.RandomState(seed)
    return np.maximum(rs.normal(size=shape), 0).astype(np.float32)                 # ReLU plateaus: ties at 0


def _pool_forward_case(form, shape, R, pair):
    def build():
        from wssdl_bus_amd.roi_pooling_layer import roi_pooling_op as op
        N, H, W, C = shape
        inputs = {"data": _t(_pool_data(60 + C + R, shape)), "rois": _t(_pool_rois(61 + R, R, N, H, W))}
        over = dict(ROI_POOL_FWD_BLOCKS=(form == "blocks"))
        if pair == "compact":
            assert op.compact_supported(H, W, C, 7, 7)
            with _cfg(**over):
                g = op._Geom(shape, inputs["rois"], 7, 7, 1.0 / 16)
                assert op._forward_form(g)[0] == form, (op._forward_form(g), form)
        diff = _t(np.random.RandomState(62).normal(size=(R, 7, 7, C)).astype(np.float32))
        inputs["diff"] = diff

        def fn(inp):
            with _cfg(**over):
                if pair == "i32":
                    top, arg = op.roi_pool(inp["data"], inp["rois"], 7, 7, 1.0 / 16)
                    grad = op.roi_pool_grad(inp["data"], inp["rois"], arg, inp["diff"], 7, 7, 1.0 / 16)
                    return top, arg, grad
                top, arg8 = op.roi_pool_compact(inp["data"], inp["rois"], 7, 7, 1.0 / 16)
                return top, arg8, op.expand_argmax(arg8, inp["rois"], shape, 7, 7, 1.0 / 16)
        return dict(fn=fn, inputs=inputs)
    return build


# i32 pair: C = 3 is no power of two (the backward that filters the RoIs itself), C = 64 takes the list-driven one
case("roi-pool-i32-c3", 3)(_pool_forward_case("small", (2, 5, 6, 3), 37, "i32"))
case("roi-pool-i32-c64", 4)(_pool_forward_case("small", (2, 13, 17, 64), 70, "i32"))
case("roi-pool-i32-r1", 3)(_pool_forward_case("small", (1, 4, 5, 32), 1, "i32"))
# compact pair: C % 32 == 0 for the small form; the table forms need 7 x 7 bins, C % 256 == 0 and R >= 1024, the block
# tables H, W >= 4 on top of that
case("roi-pool-compact-small-c32", 3)(_pool_forward_case("small", (2, 5, 6, 32), 37, "compact"))
case("roi-pool-compact-small-c256", 3)(_pool_forward_case("small", (2, 5, 6, 256), 1023, "compact"))
case("roi-pool-compact-windows", 4)(_pool_forward_case("windows", (2, 4, 5, 256), 1025, "compact"))
case("roi-pool-compact-blocks", 5)(_pool_forward_case("blocks", (2, 4, 5, 256), 1025, "compact"))

_BWD_SHAPE, _BWD_R = (2, 13, 17, 128), 301


def _pool_backward_case(kind, plan_id=-1, segments=1, owner=-1, waves=1):
    def build():
        from wssdl_bus_amd import _lib
        from wssdl_bus_amd.roi_pooling_layer import roi_pooling_op as op
        N, H, W, C = _BWD_SHAPE
        R = _BWD_R
        data, rois = _t(_pool_data(70, _BWD_SHAPE)), _t(_pool_rois(71, R, N, H, W))
        top, arg8 = op.roi_pool_compact(data, rois, 7, 7, 1.0 / 16)
        arg = op.expand_argmax(arg8, rois, _BWD_SHAPE, 7, 7, 1.0 / 16)
        diff = _t(np.random.RandomState(72).normal(size=(R, 7, 7, C)).astype(np.float32))
        inputs = {"rois": rois, "arg8": arg8, "arg": arg, "diff": diff}
        L = _lib.lib()

        def fn(inp):
            if kind == "no-lists":
                return op.roi_pool_grad_compact(_BWD_SHAPE, inp["rois"], inp["arg8"], inp["diff"], 7, 7, 1.0 / 16,
                                                use_workspace=False)
            if kind == "walk":
                with _lib.tuned(roi_bwd_plan=plan_id):
                    plan = op.roi_pool_grad_prepare(_BWD_SHAPE, inp["rois"], 7, 7, 1.0 / 16)
                assert plan.plan >= 0
                return op.roi_pool_grad_compact(_BWD_SHAPE, inp["rois"], inp["arg8"], inp["diff"], 7, 7, 1.0 / 16, plan=plan,
                                                segments=segments)
            if kind == "owner":
                plan = op.roi_pool_grad_prepare_owner(_BWD_SHAPE, inp["rois"], 7, 7, 1.0 / 16, owner)
                plan.owner_segments = waves
                return op.roi_pool_grad_compact(_BWD_SHAPE, inp["rois"], inp["arg8"], inp["diff"], 7, 7, 1.0 / 16, plan=plan)
            assert kind == "owner-i32"
            nws = L.wssdl_roi_pool_backward_workspace_bytes(R, N, H, W, 7, 7)
            nscr = L.wssdl_roi_pool_backward_owner_scratch_bytes(N, H, W, C, owner)
            ws = torch.empty((nws,), dtype=torch.uint8, device=DEV)
            scr = torch.empty((nscr,), dtype=torch.uint8, device=DEV)
            out = torch.empty(_BWD_SHAPE, dtype=torch.float32, device=DEV)
            _lib.check(L.wssdl_roi_pool_backward_owner_i32(
                _lib.ptr(inp["diff"]), _lib.ptr(inp["arg"]), _lib.ptr(inp["rois"]), R, N, H, W, C, 7, 7, 1.0 / 16, _lib.ptr(out),
                _lib.ptr(ws), nws, owner, _lib.ptr(scr), nscr, _lib.stream()), "wssdl_roi_pool_backward_owner_i32")
            return out
        return dict(fn=fn, inputs=inputs)
    return build


case("roi-pool-bwd-no-lists", 1)(_pool_backward_case("no-lists"))
for _plan in (-1, 11, 23, 21):                                       # the exact-walk plans test_split_walk... names
    for _k in (1, 2, 7):
        case("roi-pool-bwd-walk-plan%d-k%d" % (_plan, _k), 2 if _k == 1 else 3)(_pool_backward_case("walk", _plan, _k))


OWNER_PLANS = 12                # wssdl_roi_pool_backward_owner_plan_count(); test_every_owner_plan_has_its_cases holds it to that
for _owner in range(OWNER_PLANS):
    for _waves in (1, 2, 3):                                         # C = 128: C % 4 == 0, every plan takes 2 and 3 waves
        case("roi-pool-bwd-owner%d-waves%d" % (_owner, _waves), 3)(_pool_backward_case("owner", owner=_owner, waves=_waves))
for _owner in (0, 1):                                                # the plans the i32 form is built for
    case("roi-pool-bwd-owner-i32-plan%d" % _owner, 3)(_pool_backward_case("owner-i32", owner=_owner))


# --------------------------------------------------------------------------------------------------- fused losses ---

def _mt_case(name):
    def build():
        from wssdl_bus_amd.fast_rcnn.loss_op import multi_task_loss
        c = LR.make_mt_case(name, DEV)
        keys = ("rpn_cls", "rpn_box", "cls", "box", "rpn_labels", "rpn_tg", "rpn_inw", "rpn_outw", "labels", "tg", "inw", "outw",
                "gl")
        inputs = {k: c[k] for k in keys}
        inputs["rois"] = torch.zeros((c["n_rows"], 5), device=DEV)

        def fn(inp):
            leaves = [inp[k].detach().clone().requires_grad_(True) for k in ("rpn_cls", "rpn_box", "cls", "box")]
            rpn_data = (inp["rpn_labels"], inp["rpn_tg"], inp["rpn_inw"], inp["rpn_outw"])
            roi_data = (inp["rois"], inp["labels"], inp["tg"], inp["inw"], inp["outw"])
            terms = multi_task_loss(*leaves, rpn_data, roi_data, c["dims"][4])
            (terms * inp["gl"]).sum().backward()
            return terms.detach(), [x.grad for x in leaves]
        return dict(fn=fn, inputs=inputs)
    return build


for _name in ("one_anchor", "below_block", "no_rows", "no_rows_pad", "wrong_k2", "partial_nb1"):
    case("loss-multi-task-%s" % _name, 2)(_mt_case(_name))


def _per_image_case(name, spec):
    def build():
        from wssdl_bus_amd.fast_rcnn.loss_op import multi_task_loss_per_image
        seed, N, H, W, A, K, rows, regimes, nan_images = spec
        c = V.make_val_case(seed, N, H, W, A, K, rows, regimes, shuffle=True, nan_images=nan_images, junk=True, device=DEV)
        args = V.layer_args(c)
        flat = list(args[:4]) + list(args[4]) + list(args[5])

        def fn(inp):
            with torch.no_grad():
                return multi_task_loss_per_image(inp[0], inp[1], inp[2], inp[3], tuple(inp[4:4 + len(args[4])]),
                                                 tuple(inp[4 + len(args[4]):]), N)
        return dict(fn=fn, inputs=flat)
    return build


case("loss-per-image-one_cell", 3)(_per_image_case("one_cell", (32, 1, 1, 1, 1, 3, [1], ["normal"], ())))
case("loss-per-image-four_images", 3)(_per_image_case(
    "four_images", (31, 4, 16, 15, 9, 3, [0, 1, 128, 300], ["normal", "correct", "shift12", "wrong"], (1,))))


# ------------------------------------------------------------------------------------------------------------ MIL ---

def _mil_case(op_name):
    def build():
        from wssdl_bus_amd.mil import core as M
        sel = (3, 4)
        c = MP.make_case("mixed_k3", sel, DEV)
        funcs = [M.MIL_FUNCS[MP.NAMES[sel[0]]], M.MIL_FUNCS[MP.NAMES[sel[1]]]]
        cw = c["cw"].cpu().numpy()
        inputs = {"logits": c["logits"], "col": c["col"], "bag_labels": c["bag_labels"], "gl": c["gl"]}

        def fn(inp):
            if op_name == "pool-forward":
                return M.mil_bag_losses_device(inp["logits"], inp["col"], c["offset"], inp["bag_labels"], c["n_bags"], funcs, cw)
            x = inp["logits"].detach().clone().requires_grad_(True)
            if op_name == "pool-backward":
                loss = M.mil_loss_device(x, inp["col"], c["offset"], inp["bag_labels"], c["n_bags"], funcs, cw, c["scale"])
                (loss * inp["gl"]).backward()
                return loss.detach(), x.grad
            assert op_name == "select"
            bag_logits, scale, valid = M.get_bag_logit_device(x, inp["col"], c["offset"], inp["bag_labels"], c["n_bags"], funcs,
                                                             return_valid=True)
            bag_logits.sum().backward()
            return bag_logits.detach(), scale.detach(), valid, x.grad
        return dict(fn=fn, inputs=inputs)
    return build


for _op in ("pool-forward", "pool-backward", "select"):
    case("mil-%s-mixed_k3-disc_max-mean_ben" % _op, 2)(_mil_case(_op))



# ----------------------------------------------------------------------------------------------------- image path ---

def _plane(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w)).astype(np.uint8)


def _image_case(op, *a):
    def build():
        from wssdl_bus_amd.utils import blob as BL
        rs = np.random.RandomState(90)
        if op == "prep":
            h, w, flipped, delta, factor = a
            inputs = {"gray": _t(_plane(91, h, w))}
            fn = lambda inp: BL.prep_im_pre_resize(inp["gray"], flipped, delta, factor)              # noqa: E731
        elif op == "adjust-f64":
            h, w, flipped, factor = a
            inputs = {"gray": _t(_plane(92, h, w))}
            fn = lambda inp: BL.prep_im_pre_resize_rotated(inp["gray"], flipped, 3.5, 0.1, factor,   # noqa: E731
                                                           crop=(1, 2, 0, 1))
        elif op == "resize":
            shape, out, dtype = a
            inputs = {"im": _t(rs.uniform(0, 1, size=shape).astype(dtype))}
            fn = lambda inp: BL.skimage_resize(inp["im"], out)                                       # noqa: E731
        elif op == "rotate":
            shape, angle = a
            inputs = {"im": _t(rs.uniform(0, 1, size=shape).astype(np.float32))}
            fn = lambda inp: BL.skimage_rotate(inp["im"], angle, cval=0.25)                          # noqa: E731
        elif op == "warp":
            shape, out, mode, clip = a
            inputs = {"im": _t(rs.uniform(-0.2, 1.2, size=shape))}
            M = np.array([[0.9, 0.2, -3.0], [-0.1, 1.1, 2.5], [0.0, 0.0, 1.0]])
            fn = lambda inp: BL.skimage_warp(inp["im"], M, out, mode=mode, cval=0.1, clip=clip)      # noqa: E731
        elif op == "to-blob":
            inputs = {"a": _t(rs.uniform(0, 1, size=(3, 257, 3)).astype(np.float32)), "b": _t(rs.uniform(0, 1, size=(1, 1, 3))),
                      "c": _t(rs.uniform(0, 1, size=(7, 5, 3)))}
            fn = lambda inp: BL.im_list_to_blob([inp["a"], inp["b"], inp["c"]], scale=52.802 / 255.0, divide=True)  # noqa: E731
        else:
            assert op == "flip-boxes"
            from wssdl_bus_amd import _lib
            boxes = rs.uniform(0, 400, size=(a[0], 5)).astype(np.float32)
            inputs = {"boxes": _t(boxes)}

            def fn(inp):
                # wssdl_flip_boxes works IN PLACE ("datasets/imdb.py:106-121 on a GPU tensor [n, >=4] f32 (returns a mirrored
                # copy)": blob.flip_boxes hands it a clone, which no patched call allocates); here the copy is a guarded
                # buffer, so that the kernel's writes have guard bands around them, and the wrapper runs next to it
                b = torch.empty_like(inp["boxes"])
                b.copy_(inp["boxes"])
                _lib.check(_lib.lib().wssdl_flip_boxes(_lib.ptr(b), b.shape[0], b.stride(0), 498.0, _lib.stream()),
                           "wssdl_flip_boxes")
                return b, BL.flip_boxes(inp["boxes"], 498)
        return dict(fn=fn, inputs=inputs)
    return build


for _h, _w in ((1, 1), (3, 257)):
    for _flip in (False, True):
        case("image-prep-%dx%d%s-plain" % (_h, _w, "-flipped" if _flip else ""), 2)(_image_case("prep", _h, _w, _flip, None, None))
        case("image-prep-%dx%d%s-contrast" % (_h, _w, "-flipped" if _flip else ""), 2)(_image_case("prep", _h, _w, _flip, 0.15, 0.4))
case("image-adjust-f64-9x23-contrast", 6)(_image_case("adjust-f64", 9, 23, True, 0.4))
case("image-adjust-f64-9x23-plain", 6)(_image_case("adjust-f64", 9, 23, False, None))
case("image-resize-3x257-to-7x19-f32", 2)(_image_case("resize", (3, 257, 3), (7, 19), np.float32))
case("image-resize-1x1-to-5x3-f64", 2)(_image_case("resize", (1, 1), (5, 3), np.float64))
case("image-resize-23x31-to-1x1-f64", 2)(_image_case("resize", (23, 31, 3), (1, 1), np.float64))
case("image-rotate-23x31", 2)(_image_case("rotate", (23, 31, 3), -4.5))
case("image-rotate-1x1", 2)(_image_case("rotate", (1, 1), 5.0))
case("image-warp-edge-noclip", 2)(_image_case("warp", (23, 31), (17, 40), "edge", False))
case("image-warp-constant-clip", 2)(_image_case("warp", (9, 33, 3), (1, 1), "constant", True))
case("image-list-to-blob", 1)(_image_case("to-blob"))
case("image-flip-boxes-1", 1)(_image_case("flip-boxes", 1))
case("image-flip-boxes-257", 1)(_image_case("flip-boxes", 257))


def _entry(seed, h, w, flipped):
    """one roidb entry with a decoded plane, two boxes inside it and their classes"""
    rs = np.random.RandomState(1000 + seed)
    x1, y1 = rs.randint(0, max(w // 2, 1), size=2), rs.randint(0, max(h // 2, 1), size=2)
    boxes = np.stack([x1, y1, x1 + rs.randint(1, max(w // 2, 2), size=2), y1 + rs.randint(1, max(h // 2, 2), size=2)],
                     axis=1).astype(np.uint16)
    return dict(plane=_plane(seed, h, w), flipped=flipped, boxes=boxes, gt_classes=rs.randint(0, 3, size=2).astype(np.int32),
                birads_diag=1)


def small_joint():
    """the batch of test_gpu_data_layer.small_joint: 2 supervised + 3 weak entries of mixed shapes and flips (9 x 300 hits
    MAX_SIZE; a weak image needs int(0.05 * min(h, w)) >= 1 for the crop draw)"""
    sup = [_entry(1, 23, 31, True), _entry(2, 9, 300, False)]
    weak = [_entry(3, 40, 57, False), _entry(4, 57, 40, True), _entry(5, 23, 31, False)]
    return sup, weak


def _batch_blob_case(net, train):
    def build():
        from wssdl_bus_amd.roi_data_layer import minibatch_bus as M
        from wssdl_bus_amd.utils import blob as BL
        sup, weak = small_joint()

        def fn(inp):
            with _cfg(SCALES=(48,), MAX_SIZE=80):
                plan = M.plan_minibatch_joint(sup, weak, net, 3, train, rng=np.random.RandomState(7))
                return BL.image_batch_blob(plan, plan.planes), BL.image_blob_per_image(plan, plan.planes)
        return dict(fn=fn, inputs={})
    return build


case("image-batch-blob-small_joint-resnet-train", 2)(_batch_blob_case("Resnet_train", True))
case("image-batch-blob-small_joint-vgg-eval", 2)(_batch_blob_case("VGGnet_train", False))        # the VGG scaling, is_training False


# -------------------------------------------------------------------------------------------------- test-time ops ---

def _image_rows(rs, n, K):
    """n rows of one image: scores [n,K] in [0,1), class-wise boxes [n,4K] that share a centre per row (the union pass has
    a lot to suppress); from nine rows on the first eight rows of class 1 share one score and sit far apart (ties)"""
    ctr = rs.uniform(50, 900, size=(n, 1, 2)) * [1.0, 0.6] + rs.normal(0, 6, size=(n, K, 2))
    wh = rs.uniform(30, 220, size=(n, K, 2))
    boxes = np.concatenate((ctr - wh / 2, ctr + wh / 2), axis=2).reshape(n, 4 * K).astype(np.float32)
    scores = rs.uniform(0, 1, size=(n, K)).astype(np.float32)
    if n > 8:
        scores[:8, 1] = np.float32(0.625)
        boxes[:8, 4:8] = boxes[:8, 4:8] + np.arange(8, dtype=np.float32)[:, None] * 1500
    return scores, boxes


def _post_rows(R, K, n_images):
    rs = np.random.RandomState(300 + R)
    per = [R // n_images + (1 if i < R % n_images else 0) for i in range(n_images)]
    parts = [_image_rows(rs, n, K) for n in per if n > 0]
    scores = np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, K), np.float32)
    boxes = np.concatenate([p[1] for p in parts]) if parts else np.zeros((0, 4 * K), np.float32)
    assert scores.shape == (R, K) and boxes.shape == (R, 4 * K)
    rois = np.zeros((R, 5), np.float32)
    rois[:, 0] = np.repeat(np.arange(n_images), per)
    return scores, boxes, rois


def _post_case(form, R):
    def build():
        from wssdl_bus_amd.fast_rcnn import detect_batch, post_detections
        K = 4
        batched = form.endswith("batched")
        agnostic = form.startswith("agnostic")
        scores, boxes, rois = _post_rows(R, K, 3 if batched else 1)                # the batched forms: image 2 of 3 is short
        if batched and R:
            rois[-1, 0] = -1                                                        # and one row belongs to no image
        inputs = {"scores": _t(scores), "boxes": _t(boxes), "rois": _t(rois)}

        def fn(inp):
            if batched:
                return detect_batch.post_detections_batched_device(inp["scores"], inp["boxes"], inp["rois"], 3, K, 0.05, 20,
                                                                   max_rows_per_image=max(R, 1), agnostic=agnostic)
            return post_detections.post_detections_device(inp["scores"], inp["boxes"], K, 0.05, 20, agnostic=agnostic)
        return dict(fn=fn, inputs=inputs)
    return build


for _form in ("per-class", "per-class-batched", "agnostic", "agnostic-batched"):
    for _r in (0, 1, 70):
        case("post-detect-%s-r%d" % (_form, _r), 3)(_post_case(_form, _r))


def _val_detect_case(name, given):
    def build():
        from wssdl_bus_amd.fast_rcnn.val_detect import validation_detections
        c = DR.case(name)
        inputs = {"rois": _t(c["rois"]), "deltas": _t(c["deltas"]), "scores": _t(c["scores"]), "info": _t(c["im_info"])}

        def fn(inp):
            with _cfg(BATCH_SIZE=int(c["span"])):
                layers = {"roi-data": [inp["rois"]], "cls_prob": inp["scores"], "bbox_pred": inp["deltas"]}
                return validation_detections(layers, inp["info"], c["n_images"], im_shapes=c["im_shapes"] if given else None,
                                             agnostic=False)
        return dict(fn=fn, inputs=inputs)
    return build


for _name, _given in DR.RUNS:
    case("val-detect-%s-%s" % (_name, "bounds" if _given else "im_info"), 4)(_val_detect_case(_name, _given))


def _eval_case():
    from wssdl_bus_amd.datasets import eval_detections
    dets, gt, thr = EC.case("small")
    inputs = [_t(a) for a in dets]
    return dict(fn=lambda inp: eval_detections(tuple(inp), gt, EC.K, score_thresh=[thr[10]] + list(thr)), inputs=inputs)


case("eval-detections-small", 2)(_eval_case)


def _recall_case(name):
    def build():
        from wssdl_bus_amd.datasets import recall
        c = RC.cases()[name]
        gt = recall.pack_recall_gt(RC.roidb_of(c))

        def fn(inp):
            with np.errstate(all="ignore"):
                return recall.evaluate_recall_table(c["candidates"], gt, c["areas"], c["limits"], return_matches=True)
        return dict(fn=fn, inputs={})
    return build


for _name in ("tie_box", "zero_overlap", "mixed", "sizes", "random200"):
    case("proposal-recall-%s" % _name, 2)(_recall_case(_name))


def _draw_case():
    CLASSES = ['__background__', 'benign', 'malignant']
    from wssdl_bus_amd.datasets.voc_eval_bus import DetectionAccumulator
    from wssdl_bus_amd.fast_rcnn import vis
    from wssdl_bus_amd.fast_rcnn.detect_batch import post_detections_batched_device
    K, N, R = len(CLASSES), 3, 90
    rng = np.random.RandomState(12)
    planes = [rng.randint(0, 256, shape).astype(np.uint8) for shape in ((60, 80), (45, 70), (50, 50))]
    rois = np.zeros((R, 5), np.float32)
    rois[:, 0] = np.repeat(np.arange(N), R // N)
    scores = rng.rand(R, K).astype(np.float32)
    xy = rng.rand(R, K, 2) * 40
    boxes = np.concatenate([xy, xy + 5 + rng.rand(R, K, 2) * 30], 2).reshape(R, 4 * K).astype(np.float32)
    gt_roidb = [dict(boxes=np.asarray([[4, 4, 30, 30]]), gt_classes=np.asarray([1])),
                dict(boxes=np.zeros((0, 4)), gt_classes=np.zeros(0, np.int32)),
                dict(boxes=np.asarray([[10, 10, 45, 45], [0, 0, 9, 9]]), gt_classes=np.asarray([2, 1]))]

    def fn(inp):
        acc = DetectionAccumulator(K)
        d, c = post_detections_batched_device(inp["scores"], inp["boxes"], inp["rois"], N, K, 0.05, 300, max_rows_per_image=30)
        acc.add(d, c, 0)
        return vis.draw_detections(planes, gt_roidb, acc, CLASSES)
    return dict(fn=fn, inputs={"scores": _t(scores), "boxes": _t(boxes), "rois": _t(rois)})


case("draw-detections-three-images", 4)(_draw_case)



# ----------------------------------------------------------------------------------------------- plumbing library ---
# Through the Python wrappers, at the reference modules' smallest odd cases.  What a call updates in place by contract
# (running statistics, the renorm state, optimiser state, parameters) is cloned inside the case and returned as a result.

EPS = 1e-3


def _plumbing():
    from wssdl_bus_amd.networks import _plumbing as P
    assert P.lib() is not None, "plumbing library not built"
    return P


def _running(c, mom):
    # (torch.full, not torch.tensor([5], device=DEV): that one uploads from the host and synchronises it, and these
    # cases run under the synchronisation debugger of the stream-order test)
    return c["rm"].clone(), c["rv"].clone(), mom, torch.full((1,), 5, dtype=torch.int64, device=DEV)


def _rowbn_case(M, C, relu, mask_kind=None, n_rois=None, per=1, pm=False, renorm=False):
    def build():
        P = _plumbing()
        c = RB.make_case(21, M, C, DEV)
        inputs = dict(c)
        if mask_kind is not None:
            inputs["mask"] = RB.make_mask(mask_kind, n_rois, n_rois, DEV)
        state = RN.warm_state(C, 0.875, 3, DEV) if renorm else None

        def fn(inp):
            run = _running(inp, 0.01)
            ren = (state["mean"].clone(), state["stddev"].clone(), state["weight"].clone(), RN.RHO) if renorm else None
            mask = inp.get("mask")
            y, stats, count = P.rowbn_forward(inp["x"], inp["w"], inp["b"], EPS, relu, mask, pm, running=run, renorm=ren)
            grads = P.rowbn_backward(inp["x"], inp["dy"], inp["w"], stats, relu, mask, pm)
            ya = P.rowbn_apply(inp["x"], stats[3], stats[4], relu) if (mask is None and not renorm) else None
            return y, stats, count, grads, ya, run[:2], run[3], ren[:3] if renorm else None
        return dict(fn=fn, inputs=inputs)
    return build


case("rowbn-plain-1x4", 3)(_rowbn_case(1, 4, False))
case("rowbn-plain-7x256-relu", 3)(_rowbn_case(7, 256, True))
case("rowbn-plain-259x16-relu", 3)(_rowbn_case(259, 16, True))
case("rowbn-plain-1041x512", 3)(_rowbn_case(1041, 512, False))
case("rowbn-masked-1x16-one_live", 3)(_rowbn_case(16, 256, True, "one_live", 1, 16))
case("rowbn-masked-37x49-random", 3)(_rowbn_case(37 * 49, 256, True, "random", 37, 49))
case("rowbn-masked-37x49-random-pm", 3)(_rowbn_case(37 * 49, 256, True, "random", 37, 49, pm=True))
case("rowbn-masked-37x49-all_dead", 3)(_rowbn_case(37 * 49, 256, True, "all_dead", 37, 49))
case("renorm-plain-1x4", 3)(_rowbn_case(1, 4, False, renorm=True))
case("renorm-plain-259x16-relu", 3)(_rowbn_case(259, 16, True, renorm=True))
case("renorm-masked-37x49-random-pm", 3)(_rowbn_case(37 * 49, 256, True, "random", 37, 49, pm=True, renorm=True))


def _join_case(n_rois, per, C, dual, with_dres, kind):
    def build():
        P = _plumbing()
        M = n_rois * per
        c3, co, cn = (RB.make_case(25 + k, M, C, DEV) for k in range(3))
        inputs = {"x3": c3["x"], "other": co["x"], "dy": cn["dy"], "dres": cn["dres"], "w3": c3["w"], "b3": c3["b"], "ws": co["w"],
                  "bs": co["b"], "wn": cn["w"], "bn": cn["b"]}
        if kind != "none":
            inputs["mask"] = RB.make_mask(kind, n_rois, n_rois, DEV)

        def fn(inp):
            mask = inp.get("mask")
            bn3, bnn = (inp["w3"], inp["b3"], EPS), (inp["wn"], inp["bn"], EPS)
            bns = (inp["ws"], inp["bs"], 1e-5) if dual else None
            runs = [_running(c3, 0.01), _running(co, 1.0) if dual else None, _running(cn, 1.0)]
            out, y, s3, ss, sn, count = P.rowbn_join_forward(inp["x3"], bn3, inp["other"], bns, bnn, mask, running=runs)
            xs, ws = (inp["other"], inp["ws"]) if dual else (None, None)
            back = P.rowbn_join_backward(out, inp["dy"], inp["dres"] if with_dres else None, inp["x3"], xs, inp["wn"], sn,
                                         inp["w3"], s3, ws, ss if dual else None, mask)
            return out, y, s3, ss, sn, count, back, [(r[0], r[1], r[3]) for r in runs if r is not None]
        return dict(fn=fn, inputs=inputs)
    return build


for _dual in (False, True):
    case("rowbn-join-%s-37x16-c512-random" % ("dual" if _dual else "identity"), 6)(_join_case(37, 16, 512, _dual, _dual, "random"))
    case("rowbn-join-%s-1x16-c512-none" % ("dual" if _dual else "identity"), 6)(_join_case(1, 16, 512, _dual, not _dual, "none"))


def _groupnorm_case(S, Pn, C, pm, kind, relu):
    def build():
        P = _plumbing()
        c = GR.make_case(1, S, Pn, C, DEV)
        inputs = dict(c)
        if kind != "none":
            inputs["mask"] = GR.make_mask(kind, S, 3, DEV)
        assert P.groupnorm_usable(c["x"], Pn, GR.G)

        def fn(inp):
            mask = inp.get("mask")
            y, mean, rstd = P.groupnorm_forward(inp["x"], Pn, inp["w"], inp["b"], GR.EPS, GR.G, relu, mask, pm)
            return y, mean, rstd, P.groupnorm_backward(inp["x"], inp["dy"], Pn, inp["w"], inp["b"], mean, rstd, relu, mask, pm)
        return dict(fn=fn, inputs=inputs)
    return build


case("groupnorm-1x1x8", 3)(_groupnorm_case(1, 1, 8, False, "none", False))
case("groupnorm-3x49x64-relu-random", 3)(_groupnorm_case(3, 49, 64, False, "random", True))
case("groupnorm-4x7x72-pm-relu", 3)(_groupnorm_case(4, 7, 72, True, "none", True))
case("groupnorm-2x65x1024-large-first_last_dead", 3)(_groupnorm_case(2, 65, 1024, False, "first_last_dead", True))
case("groupnorm-1x300x264-large-pm", 3)(_groupnorm_case(1, 300, 264, True, "none", False))


def to_pm(t, slots):
    """roi-major [R, hh, ww, ch] -> position-major rows slot * R + roi, in the plan's slot order"""
    R_, hh, ww, ch = t.shape
    assert sorted(slots) == [(y, x) for y in range(hh) for x in range(ww)]
    idx = torch.tensor([y * ww + x for y, x in slots], dtype=torch.long, device=t.device)
    return t.reshape(R_, hh * ww, ch)[:, idx].transpose(0, 1).reshape(-1, ch).contiguous()


def _tap_case(name, geom, bias, in_pm=False, normed=False, masked=False):
    """TapConv3x3Fn forward and backward: roi-major or position-major source; normed: the source is the raw rows in front
    of a row batch norm + ReLU, which the patch gather applies while it copies (rowbn_stats, tap_gather_norm, and
    rowbn_backward behind the patches' adjoint), with running statistics and, masked, dead RoIs"""
    def build():
        P = _plumbing()
        c = HC.make_case(name, geom)
        R, C = c["R"], c["C"]
        plan = P.tap_plan(c["h"], c["w"], c["s"])
        assert not in_pm or plan.h == plan.oh
        x = _t(c["x"])
        src = to_pm(x, plan.slots) if in_pm else (x.reshape(-1, C).contiguous() if normed else x)
        nc = RB.make_case(31, 8, C, DEV)
        inputs = {"x": src, "W": _t(c["W"]), "b": _t(c["b"]), "dy": to_pm(c["dy"].to(DEV), plan.slots), "wn": nc["w"],
                  "bn": nc["b"]}
        if normed:
            assert P.tapnorm_usable(src)
        if masked:
            m = torch.ones((R,), device=DEV)
            m[R // 2], m[R - 1] = 0.0, 0.0
            inputs["mask"] = m

        def fn(inp):
            xx, W = (inp[k].detach().clone().requires_grad_(True) for k in ("x", "W"))
            b = inp["b"].detach().clone().requires_grad_(True) if bias else None
            if not normed:
                y = P.TapConv3x3Fn.apply(xx, W, b, plan, in_pm, R)
                y.backward(inp["dy"])
                return y.detach(), xx.grad, W.grad, b.grad if bias else None
            wn, bn = (inp[k].detach().clone().requires_grad_(True) for k in ("wn", "bn"))
            run = _running(nc, 0.01)
            y, mean, var, count = P.TapConv3x3Fn.apply(xx, W, b, plan, in_pm, R, wn, bn, EPS, inp.get("mask"), run)
            y.backward(inp["dy"])
            return (y.detach(), mean, var, count if masked else None, xx.grad, W.grad, b.grad if bias else None, wn.grad,
                    bn.grad, run[:2], run[3])
        return dict(fn=fn, inputs=inputs)
    return build


case("tap-conv-r1-7x7s2", 2)(_tap_case("one", (7, 7, 2), True))
case("tap-conv-r37-7x7s2", 2)(_tap_case("sharp", (7, 7, 2), True))
case("tap-conv-r37-4x4s1-no-bias", 2)(_tap_case("sharp", (4, 4, 1), False))
case("tap-conv-r37-6x5s2", 2)(_tap_case("sharp", (6, 5, 2), True))
case("tap-conv-r37-4x4s1-pos-major", 2)(_tap_case("sharp", (4, 4, 1), True, in_pm=True))
case("tap-conv-r70-4x4s1-pos-major", 2)(_tap_case("flight", (4, 4, 1), False, in_pm=True))
case("tap-conv-normed-r70-7x7s2", 5)(_tap_case("flight", (7, 7, 2), False, normed=True))
case("tap-conv-normed-r70-4x4s1-pos-major-masked", 5)(_tap_case("flight", (4, 4, 1), False, in_pm=True, normed=True, masked=True))
case("tap-conv-normed-r37-7x7s2-masked", 5)(_tap_case("sharp", (7, 7, 2), True, normed=True, masked=True))


# the head's entry norm: block 1's pre-activation norm, which also hands out the stride-2 positions position-major
# (rowbn_forward_entry) and takes its output's gradient in two parts (rowbn_backward_entry)

def _entry_norm_case(n_rois, C, masked, renorm=False):
    def build():
        P = _plumbing()
        plan = P.tap_plan(7, 7, 2)
        per, ns = 49, len(plan.slots)
        c = RB.make_case(23, n_rois * per, C, DEV)
        inputs = {"x": c["x"], "w": c["w"], "b": c["b"], "dy": c["dy"], "dys": RB.make_case(24, ns * n_rois, C, DEV)["dy"],
                  "possel": plan.subsample_slots(7, 7, 2, c["x"].device)}
        assert P.entry_usable(c["x"]) and int((inputs["possel"] >= 0).sum()) == ns
        if masked:
            inputs["mask"] = RB.make_mask("random", n_rois, n_rois, DEV)
        state = RN.warm_state(C, 0.875, 3, DEV) if renorm else None

        def fn(inp):
            run = _running(c, 0.01)
            ren = (state["mean"].clone(), state["stddev"].clone(), state["weight"].clone(), RN.RHO) if renorm else None
            mask = inp.get("mask")
            y, ys, stats, count = P.rowbn_forward_entry(inp["x"], inp["w"], inp["b"], EPS, inp["possel"], ns, mask, running=run,
                                                        renorm=ren)
            grads = P.rowbn_backward_entry(inp["x"], inp["dy"], inp["dys"], inp["possel"], ns, inp["w"], stats, mask)
            return y, ys, stats, count, grads, run[:2], run[3], ren[:3] if renorm else None
        return dict(fn=fn, inputs=inputs)
    return build


case("entry-norm-r1-c256", 5)(_entry_norm_case(1, 256, False))
case("entry-norm-r37-c256-masked", 5)(_entry_norm_case(37, 256, True))
case("entry-norm-r37-c1024", 5)(_entry_norm_case(37, 1024, False))
case("entry-norm-r37-c256-masked-renorm", 5)(_entry_norm_case(37, 256, True, renorm=True))


# the head's exit: the last join writes feat [R, C] = the mean of y over the slots instead of y, and its backward takes dfeat

def _exit_join_case(n_rois, n_slots, C, dual, kind):
    def build():
        P = _plumbing()
        M = n_rois * n_slots
        c3, co, cn = (RB.make_case(35 + k, M, C, DEV) for k in range(3))
        inputs = {"x3": c3["x"], "other": co["x"], "dfeat": cn["dy"][:n_rois].contiguous(), "w3": c3["w"], "b3": c3["b"],
                  "ws": co["w"], "bs": co["b"], "wn": cn["w"], "bn": cn["b"]}
        assert P.exit_usable(c3["x"])
        if kind != "none":
            inputs["mask"] = RB.make_mask(kind, n_rois, n_rois, DEV)

        def fn(inp):
            mask = inp.get("mask")
            bn3, bnn = (inp["w3"], inp["b3"], EPS), (inp["wn"], inp["bn"], EPS)
            bns = (inp["ws"], inp["bs"], 1e-5) if dual else None
            runs = [_running(c3, 0.01), _running(co, 1.0) if dual else None, _running(cn, 1.0)]
            out, feat, s3, ss, sn, count = P.rowbn_join_forward(inp["x3"], bn3, inp["other"], bns, bnn, mask, running=runs,
                                                                exit_slots=n_slots)
            assert feat.shape == (n_rois, C)
            xs, ws = (inp["other"], inp["ws"]) if dual else (None, None)
            back = P.rowbn_join_backward(out, inp["dfeat"], None, inp["x3"], xs, inp["wn"], sn, inp["w3"], s3, ws,
                                         ss if dual else None, mask, exit_slots=n_slots)
            return out, feat, s3, ss, sn, count, back, [(r[0], r[1], r[3]) for r in runs if r is not None], \
                P.slot_mean(inp["x3"], n_slots)
        return dict(fn=fn, inputs=inputs)
    return build


case("rowbn-join-identity-exit-r1-16-slots-c64", 6)(_exit_join_case(1, 16, 64, False, "none"))
case("rowbn-join-identity-exit-r37-16-slots-c2048-random", 6)(_exit_join_case(37, 16, 2048, False, "random"))
case("rowbn-join-identity-exit-r37-4-slots-c64-dead_run", 6)(_exit_join_case(37, 4, 64, False, "dead_run"))
case("rowbn-join-dual-exit-r37-16-slots-c256-random", 6)(_exit_join_case(37, 16, 256, True, "random"))


def _im2col_case(R, h, w, C, stride):
    def build():
        P = _plumbing()
        rs = np.random.RandomState(40 + R)
        plan = P.tap_plan(h, w, stride)
        x = _t(rs.normal(size=(R, h, w, C)).astype(np.float32))
        assert P.im2col_usable(x)
        dcols = _t(rs.normal(size=(R * plan.oh * plan.ow, 9 * C)).astype(np.float32))

        def fn(inp):
            xa = inp["x"].detach().clone().requires_grad_(True)
            cols = P.Im2Col3x3Fn.apply(xa, plan.s, plan.oh, plan.ow, plan.pt, plan.pl)
            cols.backward(inp["dcols"].view_as(cols))
            return cols.detach(), xa.grad
        return dict(fn=fn, inputs={"x": x, "dcols": dcols})
    return build


case("im2col3x3-r1-7x7s2", 2)(_im2col_case(1, 7, 7, 8, 2))
case("im2col3x3-r37-6x5s2", 2)(_im2col_case(37, 6, 5, 40, 2))


def _decay_params():
    """numel 1, 3, one chunk of 4096, one chunk + 1, a channels_last conv weight (dense, permuted), a [512, 4608] weight (576
    chunks) and a contiguous slice that starts one float into its storage (not float4-aligned: the scalar form)"""
    g = torch.Generator(device=DEV).manual_seed(11)
    rn = lambda *shape: torch.randn(*shape, generator=g, device=DEV) * 0.05                      # noqa: E731
    ps = [rn(1), rn(3), rn(4096), rn(4097), rn(64, 3, 7, 7).contiguous(memory_format=torch.channels_last), rn(512, 4608),
          rn(4100)[1:4098].detach()]
    assert not ps[4].is_contiguous() and ps[6].data_ptr() % 16 == 4
    return [p.requires_grad_() for p in ps]


def _l2_case():
    P = _plumbing()
    params, L2K = _decay_params(), 0.5 * 0.0005
    assert P.l2decay_usable(params)

    def fn(inp):
        for p in params:
            p.grad = None
        loss = P.l2_decay(params, L2K)
        loss.backward()
        return loss.detach(), [p.grad for p in params]
    return dict(fn=fn, inputs=[p.detach() for p in params])


case("l2-decay", 1)(_l2_case)


def _optim_case(kind):
    """three steps (t = 1, 2, 1000) of the one-launch optimiser from an injected state: m / accum of mixed signs, v >= 0,
    vhat on both sides of v; parameters of 1, 3, 33, one chunk, one chunk + 1 elements, a channels_last weight, a [512, 4608]
    weight; one parameter without a gradient, one with a zero gradient"""
    def build():
        from wssdl_bus_amd.fast_rcnn import optim as O
        g = torch.Generator().manual_seed(11)
        rn = lambda *shape: (torch.randn(*shape, generator=g) * 0.05).to(DEV)                    # noqa: E731
        start = [rn(1), rn(3), rn(4096), rn(4097), rn(64, 3, 7, 7).contiguous(memory_format=torch.channels_last), rn(512, 4608),
                 rn(33), rn(1000), rn(7)]
        grads = [[(torch.randn(p.shape, generator=g) * 0.01).to(DEV).contiguous(memory_format=torch.preserve_format)
                  for p in start] for _ in range(3)]
        r = [[torch.randn(p.shape, generator=g).to(DEV) for _ in range(3)] for p in start]

        def fn(inp):
            params = [p.detach().clone().requires_grad_(True) for p in inp]
            opt = O.ReferenceOptimizer(params, kind, 5e-4, eps=0.1, momentum=0.9)
            assert O.hip_usable(params)
            full = [dict(m=a * 0.02, accum=a * 0.02, v=b * b * 1e-3, vhat=b * b * 1e-3 * (1.0 + 0.5 * torch.sign(c)))
                    for a, b, c in r]
            opt.load_state_dict(dict(kind=kind, step=0, lr=5e-4, state={i: {k: full[i][k] for k in opt.views}
                                                                        for i in range(len(params))}))
            for step, t in enumerate((1, 2, 1000)):
                opt.t = t - 1
                for i, p in enumerate(params):
                    p.grad = None if i == 7 else torch.zeros_like(p) if i == 8 else grads[step][i].clone()
                opt.step()
                opt.zero_grad()
            return [p.detach() for p in params], [v for k in sorted(opt.views) for v in opt.views[k]]
        return dict(fn=fn, inputs=start)
    return build


for _kind in ("adam", "amsgrad", "sgd"):
    case("optimiser-%s" % _kind, 1)(_optim_case(_kind))


# ----------------------------------------------------------------------------------------------- the hot-path chain ---
# proposal -> padded blob -> proposal targets (device sampling) -> RoI pool forward -> prepare -> backward, eager: the
# workspace one op frees is the next op's torch.empty.

def _chain_case(fwd_blocks):
    def build():
        from wssdl_bus_amd import _lib
        from wssdl_bus_amd.roi_pooling_layer import roi_pooling_op as op
        from wssdl_bus_amd.rpn_msr import proposal_target_layer_tf_bus as ptl
        from wssdl_bus_amd.rpn_msr.proposal_layer_tf_bus import proposal_layer
        g = load_golden("proposal_layer")                             # the 38 x 63 training map of the parity tests
        prob, pred, info = (torch.from_numpy(g["res_38x63_train/" + k]).to(DEV) for k in ("prob", "pred", "im_info"))
        N, H, W = prob.shape[:3]
        gt = torch.zeros((N, 20, 5), device=DEV)
        gt[0, 0] = torch.tensor([100.0, 80.0, 380.0, 300.0, 1.0])
        gt[0, 1] = torch.tensor([500.0, 60.0, 900.0, 420.0, 0.0])
        ng = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
        feat = torch.relu(torch.randn((N, H, W, 256), device=DEV, generator=torch.Generator(DEV).manual_seed(4)))
        diff = torch.randn((128 + 2000, 7, 7, 256), device=DEV, generator=torch.Generator(DEV).manual_seed(5))

        def fn(inp):
            with _cfg(IMS_PER_BATCH=1, WS_IMS_PER_BATCH=1, SAMPLING_RNG="device", PADDED_ROIS=True), \
                    _lib.tuned(roi_fwd_blocks=fwd_blocks):
                ptl._device_calls[0] = 41                            # same sampler seed on every run
                rois = proposal_layer(inp["prob"], inp["pred"], inp["info"], True, False)
                out = ptl.proposal_target_layer_joint(rois, inp["gt"], inp["ng"], 3, True)
                r = out[0].contiguous()
                top, arg8 = op.roi_pool_compact(inp["feat"], r, 7, 7, 1.0 / 16)
                plan = op.roi_pool_grad_prepare(tuple(inp["feat"].shape), r, 7, 7, 1.0 / 16)
                g = op.roi_pool_grad_compact(tuple(inp["feat"].shape), r, arg8, inp["diff"] * top, 7, 7, 1.0 / 16, plan=plan)
                return r, out[1], top, arg8, g
        return dict(fn=fn, inputs={"prob": prob, "pred": pred, "info": info, "gt": gt, "ng": ng, "feat": feat, "diff": diff})
    return build


case("hot-path-chain-eager-fwd_blocks0", 8)(_chain_case(0))
case("hot-path-chain-eager-fwd_blocks1", 8)(_chain_case(1))


# ----------------------------------------------------------------------------------------- whole head and trunk steps ---
# One training step (forward, backward, every parameter gradient and buffer) of the seeded small cases of
# test_gpu_network_reference / network_reference: every fused route in its place in the network.

def _network_case(kind, depth, R=None, live=None):
    def build():
        import copy
        from wssdl_bus_amd.networks import _plumbing as P, backbones, roi_head
        torch.manual_seed(depth + (R or 0))
        g = torch.Generator(device=DEV).manual_seed(R or 7)
        mask = None
        if kind == "head":
            module = NR.prepare(roi_head.ResNetHeadNHWC(depth)).cuda()
            c = {18: 256, 50: 1024}[depth]
            x = torch.relu(torch.randn((R, 7, 7, c), device=DEV, generator=g))
            dy = torch.randn((R, 2 * c), device=DEV, generator=g)
            if live is not None:
                mask = torch.zeros(R, device=DEV)
                mask[torch.tensor(live, device=DEV)] = 1.0
                x = torch.where(mask.view(R, 1, 1, 1) > 0, x, 1e3 * torch.randn(x.shape, device=DEV, generator=g))
            x = x.contiguous()
        else:
            module = NR.prepare(backbones.ResNetTrunk(depth)).cuda().to(memory_format=torch.channels_last)
            x = torch.randn((2, 3, 70, 102), device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
            dy = torch.randn((2, module.out_channels, 5, 7), device=DEV, generator=g)
        state = copy.deepcopy(module.state_dict())
        inputs = {"x": x, "dy": dy}
        if mask is not None:
            inputs["mask"] = mask

        def fn(inp):
            module.load_state_dict(state)
            module.zero_grad(set_to_none=True)
            xx = inp["x"].detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
            old, P.TAPS_MIN_ROIS = P.TAPS_MIN_ROIS, 1             # the class-packed route at every R
            det, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
            roi_head.set_roi_mask(inp.get("mask"))
            try:
                y = module(xx)
                (y * inp["dy"]).sum().backward()
            finally:
                roi_head.set_roi_mask(None)
                P.TAPS_MIN_ROIS, torch.backends.cudnn.deterministic = old, det
            return NR.module_outputs(module, y, xx)
        return dict(fn=fn, inputs=inputs)
    return build


case("network-head-d50-r1", 8)(_network_case("head", 50, 1))
case("network-head-d50-r37-masked", 8)(_network_case("head", 50, 37, list(range(1, 29))))
case("network-head-d18-r5-one-live", 8)(_network_case("head", 18, 5, [3]))
case("network-trunk-d18", 8)(_network_case("trunk", 18))


N_MEMORY_CONTRACT_CASES = len(CASES)          # the table as the memory-contract work left it: 407


# --------------------------------------------------------------- exports no case above reaches through its wrapper ---
# Found by looking, for every export of include/wssdl_bus_hip.h that takes a stream, for a wrapper that names it and a case
# above that takes the wrapper down that branch.  None did for: wssdl_bbox_overlaps, wssdl_bbox_overlaps_ui,
# wssdl_shifted_anchors (no case), wssdl_roi_gt_assign and wssdl_roi_targets (the proposal-target cases all draw on the
# device), wssdl_mil_loss_forward / _backward (the MIL cases all pick the mean-ben pair), wssdl_roi_pool_backward,
# wssdl_roi_candidates and wssdl_loss_libm_probe (no wrapper names them: called directly here, as the i32 owner form is above).

def _overlap_boxes(seed, n):
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 60, size=(n, 2))                     # corners within 60 of each other, sides of 61 and more:
    boxes = np.hstack((xy, xy + rs.uniform(61, 200, size=(n, 2))))          # every box overlaps every query
    if n > 2:
        boxes[2] = boxes[0]                                 # an identical pair
    return boxes                                            # f64


def _overlaps_case(ui, n, k):
    def build():
        from wssdl_bus_amd.utils import cython_bbox, cython_bbox_ui
        fn_ = cython_bbox_ui.bbox_overlaps_ui if ui else cython_bbox.bbox_overlaps
        inputs = {"boxes": _t(_overlap_boxes(500 + n, n)), "query": _t(_overlap_boxes(600 + k, k))}
        return dict(fn=lambda inp: fn_(inp["boxes"], inp["query"]), inputs=inputs)
    return build


for _n, _k in ((1, 1), (70, 3), (257, 20)):
    case("bbox-overlaps-%dx%d" % (_n, _k), 1)(_overlaps_case(False, _n, _k))
    case("bbox-overlaps-ui-%dx%d" % (_n, _k), 1)(_overlaps_case(True, _n, _k))


def _shifted_anchors_case(H, W):
    def build():
        from wssdl_bus_amd.rpn_msr import generate_anchors as GA
        base = GA.generate_anchors(scales=np.array(B.SCALES))
        # the base anchors are a host array that the launch takes by value: the op has no device input
        return dict(fn=lambda inp: GA.shifted_anchors(H, W, STRIDE, base), inputs={})
    return build


case("shifted-anchors-1x1", 1)(_shifted_anchors_case(1, 1))
case("shifted-anchors-14x17", 1)(_shifted_anchors_case(14, 17))


def _roi_target_reference_case(name):
    """proposal_target_layer with the reference's host draw: wssdl_roi_gt_assign, the NumPy sampling, wssdl_roi_targets"""
    def build():
        from wssdl_bus_amd.rpn_msr import proposal_target_layer_tf_bus as ptl
        c = B.roi_case(name)
        over = dict(c["cfg"], SAMPLING_RNG="reference", BATCH_SIZE=24, IMS_PER_BATCH=c["n_images"], WS_IMS_PER_BATCH=0)

        def fn(inp):
            with _cfg(**over):
                return ptl.proposal_target_layer(inp["rois"], inp["gt"], inp["ng"], c["K"], c["train"], False,
                                                 rng=np.random.RandomState(5))
        return dict(fn=fn, inputs={"rois": _t(c["rois"]), "gt": _t(c["gt_boxes"]), "ng": _t(c["num_gt"])})
    return build


for _name in B.ROI_CASES:
    case("roi-targets-%s-single-reference" % _name, 2)(_roi_target_reference_case(_name))


def _mil_loss_case():
    """the pair without mean-ben: mil_loss_device goes through wssdl_mil_loss_forward / _backward"""
    from wssdl_bus_amd.mil import core as M
    sel = (0, 1)
    c = MP.make_case("mixed_k3", sel, DEV)
    funcs = [M.MIL_FUNCS[MP.NAMES[sel[0]]], M.MIL_FUNCS[MP.NAMES[sel[1]]]]
    cw = c["cw"].cpu().numpy()

    def fn(inp):
        x = inp["logits"].detach().clone().requires_grad_(True)
        loss = M.mil_loss_device(x, inp["col"], c["offset"], inp["bag_labels"], c["n_bags"], funcs, cw, c["scale"])
        (loss * inp["gl"]).backward()
        return loss.detach(), x.grad
    return dict(fn=fn, inputs={"logits": c["logits"], "col": c["col"], "bag_labels": c["bag_labels"], "gl": c["gl"]})


case("mil-loss-mixed_k3-%s-%s" % (MP.NAMES[0], MP.NAMES[1]), 2)(_mil_loss_case)


def _pool_backward_i32_case():
    """wssdl_roi_pool_backward, the form without a workspace, on the arg-max of the i32 forward"""
    from wssdl_bus_amd import _lib
    from wssdl_bus_amd.roi_pooling_layer import roi_pooling_op as op
    shape, R = (2, 5, 6, 3), 37
    N, H, W, C = shape
    data, rois = _t(_pool_data(63, shape)), _t(_pool_rois(64, R, N, H, W))
    _top, arg = op.roi_pool(data, rois, 7, 7, 1.0 / 16)
    diff = _t(np.random.RandomState(65).normal(size=(R, 7, 7, C)).astype(np.float32))

    def fn(inp):
        out = torch.empty(shape, dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().wssdl_roi_pool_backward(_lib.ptr(inp["diff"]), _lib.ptr(inp["arg"]), _lib.ptr(inp["rois"]), R, N, H, W,
                                                      C, 7, 7, 1.0 / 16, _lib.ptr(out), _lib.stream()), "wssdl_roi_pool_backward")
        return out
    return dict(fn=fn, inputs={"diff": diff, "arg": arg, "rois": rois})


case("roi-pool-bwd-i32-no-workspace", 1)(_pool_backward_i32_case)


def _roi_candidates_case(name, append_gt):
    """wssdl_roi_candidates, stage 0 of the device-sampled layer as an export of its own"""
    def build():
        from wssdl_bus_amd import _lib
        c = B.roi_case(name)
        rois, gt = _t(c["rois"], torch.float32).contiguous(), _t(c["gt_boxes"], torch.float32).contiguous()
        ng = _t(c["num_gt"], torch.int32).contiguous()
        n_img, max_gt, R = gt.shape[0], gt.shape[1], rois.shape[0]
        images = torch.arange(n_img, dtype=torch.int32, device=DEV)

        def fn(inp):
            cand = torch.empty((R + (n_img * max_gt if append_gt else 0), 5), dtype=torch.float32, device=DEV)
            num_pos = torch.empty((n_img,), dtype=torch.int32, device=DEV)
            _lib.check(_lib.lib().wssdl_roi_candidates(_lib.ptr(inp["rois"]), R, _lib.ptr(inp["gt"]), max_gt, _lib.ptr(inp["ng"]),
                                                       n_img, _lib.ptr(inp["images"]), n_img, int(append_gt), _lib.ptr(cand),
                                                       _lib.ptr(num_pos), _lib.stream()), "wssdl_roi_candidates")
            return cand, num_pos
        return dict(fn=fn, inputs={"rois": rois, "gt": gt, "ng": ng, "images": images})
    return build


case("roi-candidates-r70-append", 2)(_roi_candidates_case("r70", True))
case("roi-candidates-r1-plain", 2)(_roi_candidates_case("r1", False))


def _libm_probe_case(which):
    def build():
        from wssdl_bus_amd import _lib
        x = _t(np.random.RandomState(66).uniform(-20, 20, size=1025).astype(np.float32))

        def fn(inp):
            y = torch.empty_like(inp["x"])
            _lib.check(_lib.lib().wssdl_loss_libm_probe(_lib.ptr(inp["x"]), inp["x"].numel(), which, _lib.ptr(y), _lib.stream()),
                       "wssdl_loss_libm_probe")
            return y
        return dict(fn=fn, inputs={"x": x})
    return build


case("loss-libm-probe-0", 1)(_libm_probe_case(0))
case("loss-libm-probe-1", 1)(_libm_probe_case(1))

N_STREAM_ORDER_ADDED = len(CASES) - N_MEMORY_CONTRACT_CASES
