"""The device samplers (cfg.SAMPLING_RNG = 'device') draw exactly the rows of their NumPy restatement
(tests/sampler_model.py): same keys, same cuts, same output order.  The structural tests of test_gpu_edges.py
(quotas, bands, reproducibility) would pass a selection that is off by one rank; these would not.

The switch sets are those of tests/golden/make_golden_switches.py; the default-threshold cases guard that a
change to a sampler moves no default draw."""
import numpy as np
import pytest

import sampler_model as SM
from conftest import load_golden
from oracle import np_oracle as O
from test_gpu_parity import product_cfg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

STRIDE = [16, ]
SCALES = [8, 16, 32]

# (FG_THRESH, BG_THRESH_HI, BG_THRESH_LO, FG_FRACTION, BATCH_SIZE)
ROI_SWITCHES = {
    "default": (0.5, 0.5, 0.0, 0.25, 128),
    "overlap": (0.4, 0.6, 0.1, 0.25, 128),       # FG_THRESH < BG_THRESH_HI: a row can be fg and bg
    "gap": (0.6, 0.3, 0.1, 0.25, 128),
    "fg_one": (1.0, 0.5, 0.0, 0.25, 128),        # only the appended gt rows reach it
    "half_64": (0.5, 0.5, 0.0, 0.5, 64),
    "big_batch": (0.4, 0.6, 0.1, 0.25, 4096),    # more than an image's candidates: padding rows
}
# (RPN_FG_FRACTION, RPN_BATCHSIZE)
ANCHOR_DRAWS = ((0.5, 256), (0.25, 64), (0.0, 256), (0.5, 40), (1.0, 256))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd import _lib
    _lib.lib()
    return torch


def _max_overlaps(cand, gt, num_gt):
    """f64 IoU maximum of every candidate row against the positive gt boxes of its image (0 for other rows)."""
    ov = np.zeros(cand.shape[0], np.float64)
    assign = np.full(cand.shape[0], -1, np.int64)
    for img in range(gt.shape[0]):
        rows = np.flatnonzero(cand[:, 0] == img)
        npos = int(np.sum(gt[img, :num_gt[img], 4] != 0))
        if rows.size == 0 or npos == 0:
            continue
        o = O.bbox_overlaps(cand[rows, 1:5].astype(np.float64), gt[img, :npos, :4].astype(np.float64))
        ov[rows] = o.max(axis=1)
        assign[rows] = o.argmax(axis=1)
    return ov, assign


def _roi_sample_device(torch, cand_batch, ov, images, rpi, fg_rpi, th, seed):
    from wssdl_bus_amd import _lib
    Rc = cand_batch.shape[0]
    cand = np.zeros((Rc, 5), np.float32)
    cand[:, 0] = cand_batch
    cand_d = torch.from_numpy(cand).cuda()
    ov_d = torch.from_numpy(np.ascontiguousarray(ov, np.float64)).cuda()
    img_d = torch.tensor(list(images), dtype=torch.int32, device="cuda")
    S = len(images)
    keep = torch.full((S * rpi,), -7, dtype=torch.int32, device="cuda")
    is_fg = torch.full((S * rpi,), 7, dtype=torch.uint8, device="cuda")
    counts = torch.full((S, 2), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().wssdl_roi_sample_device(
        _lib.ptr(cand_d), _lib.ptr(ov_d), Rc, _lib.ptr(img_d), S, rpi, fg_rpi, th[0], th[1], th[2], seed,
        _lib.ptr(keep), _lib.ptr(is_fg), _lib.ptr(counts), _lib.stream()), "wssdl_roi_sample_device")
    return keep.cpu().numpy(), is_fg.cpu().numpy(), counts.cpu().numpy()


def _check_roi_draw(torch, cand_batch, ov, images, rpi, fg_rpi, th, seed, tag):
    got = _roi_sample_device(torch, cand_batch, ov, images, rpi, fg_rpi, th, seed)
    want = SM.roi_sample(cand_batch, ov, images, rpi, fg_rpi, th[0], th[1], th[2], seed)
    for k in (2, 0, 1):                           # counts first: the clearest message
        nm = ("keep", "is_fg", "counts")[k]
        g, w = got[k], want[k]
        bad = np.flatnonzero(g.ravel() != w.ravel())[:8]
        assert np.array_equal(g, w), (tag, nm, "at", bad.tolist(), "got", g.ravel()[bad].tolist(),
                                      "want", w.ravel()[bad].tolist())
    return want


# ------------------------------------------------------------------ RoI sampler ---

@pytest.mark.parametrize("switch", sorted(ROI_SWITCHES))
def test_roi_sample_device_exact(torch_cuda, switch):
    """wssdl_roi_sample_device on the proposal_target golden's candidates (rois + appended gt rows), given the
    f64 max overlaps: keep, is_fg and counts equal the restatement's, for three seeds."""
    g = load_golden("proposal_target")
    rois, gt, ng = g["rois_in"], g["gt_boxes"], g["num_gt"]
    fg_t, bg_hi, bg_lo, frac, rpi = ROI_SWITCHES[switch]
    fg_rpi = int(np.round(frac * rpi))
    cand = SM.proposal_candidates(rois, gt, ng, [0, 1], True)
    ov, _ = _max_overlaps(cand, gt, ng)
    for seed in (1, 0x9E3779B1 * 3 + 0x51ED27, 0xFFFFFFFFFFFFFFFF):
        for images in ([0, 1], [1]):
            w = _check_roi_draw(torch_cuda, cand[:, 0], ov, images, rpi, fg_rpi, (fg_t, bg_hi, bg_lo), seed,
                                (switch, seed, images))
    if switch == "overlap":
        # the case this pins: some row is drawn twice, once as fg and once as bg (as the reference may)
        keep, is_fg, _ = w
        assert np.intersect1d(keep[(is_fg == 1) & (keep >= 0)], keep[(is_fg == 0) & (keep >= 0)]).size > 0
    if switch == "fg_one":
        keep, is_fg, counts = w
        assert counts[0, 0] == 1                   # the one positive gt row of the image, nothing else
    if switch == "big_batch":
        assert (w[0] == -1).any()


def test_roi_sample_device_exact_long_and_interleaved_spans(torch_cuda):
    """Spans longer than 32 rows per thread (the sampler's class masks give way to re-reads), images whose rows
    interleave, rows of images that are not sampled, and overlaps exactly on the thresholds."""
    rs = np.random.RandomState(41)
    levels = np.array([0.0, 0.1, 0.3, 0.4, 0.5, 0.6, 1.0])
    for Rc, n_img, interleave in ((40000, 1, False), (70001, 3, True), (5000, 4, False), (33, 2, True)):
        if interleave:
            batch = rs.randint(-1, n_img, size=Rc)
        else:
            batch = np.sort(rs.randint(0, n_img, size=Rc))
        ov = np.where(rs.rand(Rc) < 0.2, levels[rs.randint(0, levels.size, size=Rc)], rs.rand(Rc))
        images = list(range(n_img))[::-1] if n_img > 1 else [0]
        for th in ((0.5, 0.5, 0.0), (0.4, 0.6, 0.1), (0.6, 0.3, 0.1)):
            for rpi, fg_rpi in ((128, 32), (512, 256), (64, 0), (64, 64)):
                _check_roi_draw(torch_cuda, batch, ov, images, rpi, fg_rpi, th, 0x1234567 + Rc,
                                (Rc, th, rpi, fg_rpi))


@pytest.mark.parametrize("switch", sorted(ROI_SWITCHES))
def test_proposal_target_device_exact_rows(torch_cuda, switch, product_cfg):
    """wssdl_proposal_target_device through the layer (its seed formula, _device_calls reset): the sampled rows,
    their labels and weights are those of the restatement on the Stage-0 candidate layout."""
    torch = torch_cuda
    from wssdl_bus_amd.rpn_msr import proposal_target_layer_tf_bus as ptl
    g = load_golden("proposal_target")
    rois, gt, ng = g["rois_in"], g["gt_boxes"], g["num_gt"]
    fg_t, bg_hi, bg_lo, frac, rpi = ROI_SWITCHES[switch]
    iw = (0.1, 0.0, 2.0, -0.5)
    product_cfg(SAMPLING_RNG="device", DEVICE_RNG_SEED=29, FG_THRESH=fg_t, BG_THRESH_HI=bg_hi, BG_THRESH_LO=bg_lo,
                FG_FRACTION=frac, BATCH_SIZE=rpi, BBOX_INSIDE_WEIGHTS=iw, IMS_PER_BATCH=1, WS_IMS_PER_BATCH=1)
    fg_rpi = int(np.round(frac * rpi))
    args = [torch.from_numpy(x).cuda() for x in (rois, gt, ng.astype(np.int32))]
    for mode in ("alt", "joint"):
        ptl._device_calls[0] = 0
        if mode == "alt":
            o = ptl.proposal_target_layer(*args, 3, True, False)
            images = [0, 1]
        else:
            o = ptl.proposal_target_layer_joint(*args, 3, True)
            images = [0]
        out_rois, labels, _, inw, outw = (t.cpu().numpy() for t in o)
        cand = SM.proposal_candidates(rois, gt, ng, images, True)
        ov, assign = _max_overlaps(cand, gt, ng)
        keep, is_fg, counts = SM.roi_sample(cand[:, 0], ov, images, rpi, fg_rpi, fg_t, bg_hi, bg_lo,
                                            SM.roi_seed(29, 1))
        n = keep.size
        want_rois = np.zeros((n, 5), np.float32)
        want_rois[:, 0] = -1
        want_rois[keep >= 0] = cand[keep[keep >= 0]]
        want_lab = np.full(n, -1, np.float32)
        want_lab[keep >= 0] = 0
        fg = np.flatnonzero(is_fg == 1)
        for p in fg:
            img = int(cand[keep[p], 0])
            want_lab[p] = gt[img, assign[keep[p]], 4]
        want_iw = np.zeros((n, 12), np.float32)
        want_ow = np.zeros((n, 12), np.float32)
        for p in fg:
            c = int(want_lab[p])
            want_iw[p, 4 * c:4 * c + 4] = iw
            want_ow[p, 4 * c:4 * c + 4] = np.asarray(iw) > 0
        assert np.array_equal(out_rois[:n], want_rois), (switch, mode)
        assert np.array_equal(labels[:n, 0], want_lab), (switch, mode)
        assert np.array_equal(inw, want_iw) and np.array_equal(outw, want_ow), (switch, mode)
        if mode == "joint":
            assert np.array_equal(out_rois[n:], rois[rois[:, 0] == 1])


# --------------------------------------------------------------- anchor sampler ---

def _flat_hwa(labels, A=9):
    """[1, 1, A*H, W] layer output -> the label stage's flat (h, w, a) order"""
    H, W = labels.shape[-2] // A, labels.shape[-1]
    return np.ascontiguousarray(labels.reshape(A, H, W).transpose(1, 2, 0).reshape(-1))


def _anchor_pre_sets():
    g = load_golden("anchor_target_res_38x63")
    sets = {k: _flat_hwa(g[k + "/labels_pre"])
            for k in ("FILE04254", "outside_quirk", "big_pos", "twenty", "twenty_fg")}
    s = load_golden("anchor_target_switches")
    for k in ("clobber/FILE04254", "overlaps_clobber/twenty_fg", "overlaps/twenty_fg"):
        sets[k] = _flat_hwa(s[k + "/labels_pre"])
    return sets


def test_anchor_subsample_device_exact(torch_cuda):
    """wssdl_anchor_subsample_device in both launch forms -- counts passed (fg and bg drawn by two workgroups per
    image) and counts = NULL (one workgroup draws both) -- leaves exactly the restatement's labels."""
    torch = torch_cuda
    from wssdl_bus_amd import _lib
    for name, pre in _anchor_pre_sets().items():
        two = np.stack([pre, pre[::-1].copy()])                              # two "images"
        assert two.shape == (2, 38 * 63 * 9)
        cnt = torch.tensor([[0, int((x == 1).sum()), int((x == 0).sum()), 0] for x in two], dtype=torch.int32,
                           device="cuda")
        for frac, batch in ANCHOR_DRAWS:
            seed = 0x9E3779B1 * 3 + batch
            want = SM.anchor_subsample(two, batch, frac, seed)
            for counts in (cnt, None):
                a = torch.from_numpy(two).cuda()
                _lib.check(_lib.lib().wssdl_anchor_subsample_device(
                    _lib.ptr(a), 2, a.shape[1], batch, frac, seed, _lib.ptr(counts) if counts is not None else None,
                    _lib.stream()), "wssdl_anchor_subsample_device")
                assert np.array_equal(a.cpu().numpy(), want), (name, frac, batch, counts is None)


# (RPN_CLOBBER_POSITIVES, RPN_POSITIVE_OVERLAP, RPN_NEGATIVE_OVERLAP, RPN_FG_FRACTION, RPN_BATCHSIZE)
ANCHOR_SWITCHES = {
    "default": (False, 0.7, 0.3, 0.5, 256),
    "clobber": (True, 0.7, 0.3, 0.5, 256),
    "overlaps": (False, 0.5, 0.6, 0.5, 256),
    "overlaps_clobber": (True, 0.5, 0.6, 0.5, 256),
    "fg_quarter_64": (False, 0.7, 0.3, 0.25, 64),
}


@pytest.mark.parametrize("switch", sorted(ANCHOR_SWITCHES))
def test_anchor_target_layer_device_draw_exact(torch_cuda, switch, product_cfg):
    """The layer with cfg.SAMPLING_RNG = 'device' (its seed formula, _device_calls reset): the final labels are the
    restatement's draw on the label stage's own labels."""
    torch = torch_cuda
    from wssdl_bus_amd.rpn_msr import anchor_target_layer_tf_bus as atl
    clob, pos, neg, frac, batch = ANCHOR_SWITCHES[switch]
    product_cfg(SAMPLING_RNG="device", DEVICE_RNG_SEED=5, RPN_CLOBBER_POSITIVES=clob, RPN_POSITIVE_OVERLAP=pos,
                RPN_NEGATIVE_OVERLAP=neg, RPN_FG_FRACTION=frac, RPN_BATCHSIZE=batch)
    g = load_golden("anchor_target_res_38x63")
    H, W, A = 38, 63, 9
    score = torch.zeros((1, H, W, 18), device="cuda")
    for name in ("FILE04254", "twenty", "twenty_fg", "big_pos"):
        gt = torch.from_numpy(g[name + "/gt_boxes"][None]).cuda()
        ng = torch.from_numpy(g[name + "/num_gt"]).cuda()
        ii = torch.from_numpy(g[name + "/im_info"][None]).cuda()
        ds = str(g[name + "/dataset"])
        pre = atl.anchor_labels(gt, ng, ii, 1, H, W, STRIDE, SCALES, ds)[0].cpu().numpy()
        atl._device_calls[0] = 0
        lab = atl.anchor_target_layer(score, gt, ng, ii, None, STRIDE, SCALES, ds)[0].cpu().numpy()
        want = SM.anchor_subsample(pre, batch, frac, SM.anchor_seed(5, 1))
        want = want.reshape(H, W, A).transpose(2, 0, 1).reshape(1, 1, A * H, W)
        assert np.array_equal(lab.astype(np.int8), want), (switch, name)
