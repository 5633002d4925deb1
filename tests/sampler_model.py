"""NumPy restatement of the two device samplers (cfg.SAMPLING_RNG = 'device'), exact to the row.

Both draw by counter-based keys: a SplitMix64-style hash per (seed, image, [phase,] row) in the high word and
the row index in the low word (unique keys), and keep the `quota` smallest keys of a class.

  anchor side  : csrc/anchor_target.hip  sample_key / subsample_one / anchor_subsample_kernel
  RoI side     : csrc/roi_targets.hip    rs_key / roi_sample_kernel (fg rows first, then bg rows, each
                 in candidate order, then -1 padding)

The seeds the layers pass are those of rpn_msr/anchor_target_layer_tf_bus.py (_run_device) and
rpn_msr/proposal_target_layer_tf_bus.py (_supervised_device)."""
import numpy as np

M64 = 0xFFFFFFFFFFFFFFFF
BG_SEED_XOR = 0x5bd1e995


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def mix64(z):
    z = _u64(z)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _key(seed, lo_word_in, i):
    h = mix64(np.uint64(seed & M64) ^ mix64(lo_word_in))
    return (h & np.uint64(0xFFFFFFFF00000000)) | _u64(i)


def sample_key(seed, img, phase, i):
    """anchor_target.hip sample_key, for an array of anchor indices i."""
    i = _u64(np.asarray(i, dtype=np.int64))
    return _key(seed, (np.uint64(img) << np.uint64(34)) ^ (np.uint64(phase) << np.uint64(32)) ^ i, i)


def rs_key(seed, img, i):
    """roi_targets.hip rs_key, for an array of candidate indices i."""
    i = _u64(np.asarray(i, dtype=np.int64))
    return _key(seed, (np.uint64(img & 0xFFFFFFFF) << np.uint64(34)) ^ i, i)


def smallest(members, keys, quota):
    """The members with the `quota` smallest keys, in member order (all of them when there are no more)."""
    if members.size <= quota:
        return members
    if quota <= 0:
        return members[:0]
    cut = np.sort(keys)[quota - 1]
    return members[keys <= cut]


# ------------------------------------------------------------------ anchors ---

def anchor_seed(device_rng_seed, call):
    return (int(device_rng_seed) * 0x9E3779B1 + call) & M64


def anchor_subsample(labels, batchsize, fg_fraction, seed):
    """wssdl_anchor_subsample_device on int8 labels [n_images, total]: the labels after both draws."""
    lab = np.array(labels, dtype=np.int8, copy=True)
    num_fg = int(fg_fraction * float(batchsize))
    for img in range(lab.shape[0]):
        row = lab[img]
        fg_left = 0
        for phase, which in ((0, 1), (1, 0)):
            quota = num_fg if which == 1 else batchsize - fg_left
            members = np.flatnonzero(row == which)
            kept = smallest(members, sample_key(seed, img, phase, members), quota)
            row[np.setdiff1d(members, kept)] = -1
            if which == 1:
                fg_left = kept.size
    return lab


# --------------------------------------------------------------------- RoIs ---

def roi_seed(device_rng_seed, call):
    return (int(device_rng_seed) * 0x9E3779B1 + 0x51ED27 * call) & M64


def roi_sample(cand_batch, max_overlap, images, rois_per_image, fg_rois_per_image, fg_thresh, bg_hi, bg_lo,
               seed):
    """wssdl_roi_sample_device: (keep [S*rpi] i32, is_fg [S*rpi] u8, counts [S, 2] i32).

    fg and bg are classified independently, as in proposal_target_layer_tf_bus.py:241,253-254: with
    FG_THRESH < BG_THRESH_HI a row can be drawn once as fg and once as bg."""
    cand_batch = np.asarray(cand_batch).astype(np.int64)
    ov = np.asarray(max_overlap, dtype=np.float64)
    S = len(images)
    keep = np.full(S * rois_per_image, -1, np.int32)
    is_fg = np.zeros(S * rois_per_image, np.uint8)
    counts = np.zeros((S, 2), np.int32)
    for s, img in enumerate(images):
        mine = cand_batch == img
        fg = np.flatnonzero(mine & (ov >= fg_thresh))
        bg = np.flatnonzero(mine & (ov < bg_hi) & (ov >= bg_lo))
        n_fg = min(fg_rois_per_image, fg.size)
        n_bg = min(rois_per_image - n_fg, bg.size)
        kf = smallest(fg, rs_key(seed, img, fg), n_fg)
        kb = smallest(bg, rs_key(seed ^ BG_SEED_XOR, img, bg), n_bg)
        o = s * rois_per_image
        keep[o:o + n_fg] = kf
        is_fg[o:o + n_fg] = 1
        keep[o + n_fg:o + n_fg + n_bg] = kb
        counts[s] = (n_fg, n_bg)
    return keep, is_fg, counts


def proposal_candidates(rois, gt_boxes, num_gt, images, append_gt):
    """The candidate rows of wssdl_proposal_target_device (include/wssdl_bus_hip.h, Stage 0): the rois, then per
    sampled image all max_gt slots of its gt array, batch index = the image for its positive boxes and -1 for
    the other slots."""
    rois = np.asarray(rois, np.float32)
    gt_boxes = np.asarray(gt_boxes, np.float32)
    max_gt = gt_boxes.shape[1]
    parts = [rois]
    if append_gt:
        for img in images:
            ng = min(max(int(num_gt[img]), 0), max_gt)
            npos = int(np.sum(gt_boxes[img, :ng, 4] != 0))
            c = np.empty((max_gt, 5), np.float32)
            c[:, 0] = -1.0
            c[:npos, 0] = img
            c[:, 1:] = gt_boxes[img, :, :4]
            parts.append(c)
    return np.concatenate(parts, axis=0)
