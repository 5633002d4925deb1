#!/usr/bin/env python3
"""Generate tests/golden/anchor_target_switches.npz and proposal_target_switches.npz: the reference's own anchor-target
and proposal-target layers (imported through oracle/ref_python_stage.py) with non-default cfg.TRAIN switches.

Run in the build container only:  python tests/golden/make_golden_switches.py
Data only: the inputs are those of make_golden.py (same helpers; its .npz files are read here, never
written), the outputs are the reference's.  Each switch set is applied to the reference's cfg for
one call and restored afterwards.  Re-running reproduces the files bit-for-bit.

Bounding the size: the regression targets of both anchor-target files do not depend on any switch here (the
generator asserts it), so they are not stored again -- the tests compare them with anchor_target_res_38x63.npz
and anchor_target_joint.npz.
"""
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import ref_python_stage as stage  # noqa: E402
from make_golden import labels_i8, sample_gt, save, synth_gt_sets  # noqa: E402

# anchor target (a5), cfg.TRAIN keys per set
ANCHOR_SWITCHES = {
    "clobber": dict(RPN_CLOBBER_POSITIVES=True),
    "overlaps": dict(RPN_POSITIVE_OVERLAP=0.5, RPN_NEGATIVE_OVERLAP=0.6),
    "overlaps_clobber": dict(RPN_POSITIVE_OVERLAP=0.5, RPN_NEGATIVE_OVERLAP=0.6, RPN_CLOBBER_POSITIVES=True),
    "posw_030": dict(RPN_POSITIVE_WEIGHT=0.3),
    "posw_075": dict(RPN_POSITIVE_WEIGHT=0.75),
    "posw_clobber": dict(RPN_POSITIVE_WEIGHT=0.75, RPN_CLOBBER_POSITIVES=True),
    "inside_w": dict(RPN_BBOX_INSIDE_WEIGHTS=(0.1, 1.0, 0.0, 2.5)),
    "fg_quarter_64": dict(RPN_FG_FRACTION=0.25, RPN_BATCHSIZE=64),
}
ANCHOR_CASES = ("FILE04254", "on_anchor", "twenty", "twenty_fg", "pos_only_udiat")
ANCHOR_JOINT = dict(RPN_CLOBBER_POSITIVES=True, RPN_POSITIVE_WEIGHT=0.75, RPN_BBOX_INSIDE_WEIGHTS=(0.1, 1.0, 0.0, 2.5))

# proposal target (a10); joint_train runs with BBOX_NORMALIZE_TARGETS_PRECOMPUTED on, alt_train with it off
PROPOSAL_SWITCHES = {
    "overlap": dict(FG_THRESH=0.4, BG_THRESH_HI=0.6, BG_THRESH_LO=0.1),
    "gap": dict(FG_THRESH=0.6, BG_THRESH_HI=0.3, BG_THRESH_LO=0.1),
    "fg_one": dict(FG_THRESH=1.0),
    "half_64": dict(FG_FRACTION=0.5, BATCH_SIZE=64),
    "big_batch": dict(BATCH_SIZE=4096),
    "inside_w": dict(BBOX_INSIDE_WEIGHTS=(0.1, 0.0, 2.0, -0.5)),
}
PT_NAMES = ("rois", "labels", "targets", "inside", "outside")


@contextlib.contextmanager
def switched(cfg, **keys):
    saved = {k: cfg.TRAIN[k] for k in keys}
    try:
        cfg.TRAIN.update(keys)
        yield
    finally:
        cfg.TRAIN.update(saved)


def anchor_cases():
    """The res_38x63 inputs of make_golden.py for ANCHOR_CASES."""
    im_h, im_w = 600, 1000
    synth = synth_gt_sets(im_h, im_w)
    info = np.array([im_h, im_w, 1.0, 1], np.float32)
    gt, n, ii = sample_gt("FILE04254", 600, 1000)
    return {"FILE04254": (gt, n, ii, "SNUBH"),
            "on_anchor": synth["on_anchor"] + (info, "SNUBH"),
            "twenty": synth["twenty"] + (info, "SNUBH"),
            "twenty_fg": synth["twenty"] + (info, "SNUBH_FG"),
            "pos_only_udiat": synth["pos_only"] + (info, "UDIAT")}


def main():
    R = stage.load()
    cfg = R.cfg
    scales, stride = [8, 16, 32], [16, ]
    H, W = 38, 63
    defaults = dict(cfg.TRAIN)
    base = np.load(os.path.join(HERE, "anchor_target_res_38x63.npz"))

    # ---- a5 ------------------------------------------------------------------------------------------------
    out = {}
    cases = anchor_cases()
    for sname, keys in ANCHOR_SWITCHES.items():
        for cname in ANCHOR_CASES:
            gt, n, info, dataset = cases[cname]
            assert np.array_equal(gt, base[cname + "/gt_boxes"]) and np.array_equal(info, base[cname + "/im_info"])
            score = np.zeros((1, H, W, 18), np.float32)
            gtb, ng, ii = gt[None], np.array([n], np.int32), info[None]
            with switched(cfg, **dict(keys, RPN_BATCHSIZE=10 ** 9)):
                pre = R.anchor_target_layer(score, gtb, ng, ii, None, stride, scales, dataset)
            seed = 100 + len(out) // 5                 # one seed per (switch set, case)
            np.random.seed(seed)
            with switched(cfg, **keys), np.errstate(divide="ignore"):
                fin = R.anchor_target_layer(score, gtb, ng, ii, None, stride, scales, dataset)
            # the targets depend on no switch here: stored once, in anchor_target_res_38x63.npz
            assert np.array_equal(pre[1], base[cname + "/targets_pre"]) and np.array_equal(fin[1], base[cname + "/targets"])
            k = "%s/%s/" % (sname, cname)
            out[k + "seed"] = np.array(seed)
            out[k + "labels_pre"] = labels_i8(pre[0])
            out[k + "labels"] = labels_i8(fin[0])
            out[k + "inside_w"] = fin[2]
            out[k + "outside_w"] = fin[3]
            assert np.all(np.isfinite(fin[3])), (sname, cname)
    # joint train batch: 1 supervised + 2 weak images, as anchor_target_joint.npz
    joint = np.load(os.path.join(HERE, "anchor_target_joint.npz"))
    gtb, ng, ii = joint["gt_boxes"], joint["num_gt"], joint["im_info"]
    score = np.zeros((3, H, W, 18), np.float32)
    np.random.seed(7)
    with switched(cfg, **ANCHOR_JOINT), np.errstate(divide="ignore"):
        jt = R.anchor_target_layer_joint(score, gtb, ng, ii, None, True, stride, scales, "SNUBH")
    assert np.array_equal(jt[1], joint["train_targets"])
    out["joint/seed"] = np.array(7)
    out["joint/labels"] = labels_i8(jt[0])
    out["joint/inside_w"] = jt[2]
    out["joint/outside_w"] = jt[3]
    save("anchor_target_switches", H=np.array(H), W=np.array(W), **out)

    # ---- a10 -----------------------------------------------------------------------------------------------
    pt = np.load(os.path.join(HERE, "proposal_target.npz"))
    rois, gtb, ng = pt["rois_in"], pt["gt_boxes"], pt["num_gt"]
    out = {}
    for sname, keys in PROPOSAL_SWITCHES.items():
        np.random.seed(13)
        with switched(cfg, **keys):
            o = R.proposal_target_layer(rois, gtb, ng, 3, True, False)
        for k, nm in enumerate(PT_NAMES):
            out["%s/alt_train/%s" % (sname, nm)] = o[k]
        np.random.seed(17)
        with switched(cfg, IMS_PER_BATCH=1, WS_IMS_PER_BATCH=1, BBOX_NORMALIZE_TARGETS_PRECOMPUTED=True, **keys):
            o = R.proposal_target_layer_joint(rois, gtb, ng, 3, True)
        for k, nm in enumerate(PT_NAMES):
            out["%s/joint_train/%s" % (sname, nm)] = o[k]
    out["seed_alt"] = np.array(13)
    out["seed_joint"] = np.array(17)
    out["means"] = np.asarray(cfg.TRAIN.BBOX_NORMALIZE_MEANS, np.float64)
    out["stds"] = np.asarray(cfg.TRAIN.BBOX_NORMALIZE_STDS, np.float64)
    save("proposal_target_switches", **out)
    assert dict(cfg.TRAIN) == defaults


if __name__ == "__main__":
    if not stage.reference_present():
        sys.exit("reference tree not present: golden vectors can only be generated in the build container")
    main()
