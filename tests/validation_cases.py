"""Shared by test_validation_cpu.py and test_gpu_validation.py: multi-image cases for the per-image loss op
(loss_op.multi_task_loss_per_image) in the format of loss_reference.make_mt_case, their single-image slices (what
loss_reference.mt_reference is evaluated on), and the count-weighted combination that the batch op must agree with.
torch only, any device, no import of the package.

A case is built image by image with the recipe of loss_reference.make_mt_case -- anchor labels -1 / 0 / 1, in_w in
{0, 0.5, 1}, out_w = 1 / n_examples, the box specials (d = +-1 exactly and one ulp on either side, |d| >= 1 under
in_w = 0) on the first labelled elements of every image, make_logits under that image's regime -- and the RoI rows of
all images are then put into one list with their image index in column 0 of a [R, 5] blob."""
import torch

import loss_reference as R


def make_val_case(seed, N, H, W, A, K, rows, regimes, shuffle=False, nan_images=(), junk=False, device="cpu"):
    """rows[i] labelled rows of image i (labels in [0, K), box weights on the label's columns when it is > 0);
    regimes[i] the make_logits regime of image i's anchors and rows.  shuffle: the row list is permuted, so that the
    images interleave.  nan_images: every anchor label of these images is -1.  junk: three rows per non-empty image
    with label -1 and NON-ZERO box weights, one row with image index -1 and one with index N (both with a valid
    label and weights), all inside the list: none of them belongs to any image's terms."""
    g = torch.Generator().manual_seed(seed)
    rpn = {k: [] for k in ("rpn_cls", "rpn_labels", "rpn_box", "rpn_tg", "rpn_inw", "rpn_outw")}
    n_anchor = H * W * A
    for i in range(N):
        pick = torch.rand((n_anchor,), generator=g)
        lab = torch.where(pick < 0.55, -1, torch.where(pick < 0.85, 0, 1))
        lab[0] = 1
        s2 = R.make_logits(g, n_anchor, 2, lab.clamp_min(0), regimes[i])
        n_ex = R._not_pow2(int((lab >= 0).sum()))
        lab4 = lab.repeat_interleave(4)
        n_el = lab4.numel()
        pred = torch.randn((n_el,), generator=g) * 0.7
        tg = torch.randn((n_el,), generator=g) * 0.7
        half = torch.rand((n_el,), generator=g) < 0.5
        iw = torch.where(lab4 == 1, torch.where(half, 0.5, 1.0), 0.0)
        ow = torch.where(lab4 >= 0, 1.0 / n_ex, 0.0)
        far = (lab4 == 1) & (torch.rand((n_el,), generator=g) < 0.3)
        tg = tg + far * torch.where(half, 3.0, -2.5)
        spots = (lab4 >= 0).nonzero().squeeze(1)[:len(R._BOX_SPECIALS)]
        for e, (p_, t_, w_) in zip(spots.tolist(), R._BOX_SPECIALS):
            pred[e], tg[e], iw[e] = p_, t_, w_
        if i in nan_images:
            lab = torch.full_like(lab, -1)                           # (box weights stay: the box term does not read labels)
        nchw = lambda t: t.float().view(1, H, W, 4 * A).permute(0, 3, 1, 2).contiguous()
        rpn["rpn_cls"].append(R._scatter_scores(s2, (1, H, W, A, 1)))
        rpn["rpn_labels"].append(lab.view(1, H, W, A).permute(0, 3, 1, 2).reshape(1, 1, A * H, W).to(torch.int32))
        rpn["rpn_box"].append(pred.float().view(1, H, W, 4 * A))
        rpn["rpn_tg"].append(nchw(tg))
        rpn["rpn_inw"].append(nchw(iw))
        rpn["rpn_outw"].append(nchw(ow))
    c = {k: torch.cat(v, 0).contiguous() for k, v in rpn.items()}

    img, labr, cls, rinw, routw, rtg, box = [], [], [], [], [], [], []
    cols = torch.arange(4 * K).unsqueeze(0) // 4
    for i in range(N):
        n = rows[i]
        extra = 3 if (junk and n > 0) else 0
        m = n + extra
        l = torch.randint(0, K, (m,), generator=g)
        cls.append(R.make_logits(g, m, K, l, regimes[i]))
        b = (torch.randn((m, 4 * K), generator=g) * 0.5).float()
        t = torch.randn((m, 4 * K), generator=g) * 0.5
        rhalf = torch.rand((m, 4 * K), generator=g) < 0.5
        fg = (cols == l.unsqueeze(1)) & (l.unsqueeze(1) > 0)
        if extra:
            l[n:] = -1
            fg[n:, 4:8] = True                                       # padding rows WITH weights
        t = t + (fg & rhalf) * 2.0
        spots = fg.reshape(-1).nonzero().squeeze(1)[:3]
        for e, dd in zip(spots.tolist(), (0.0, 1.0, -1.0)):          # sgn(0) = 0; |d| = 1 exactly
            t.view(-1)[e] = 0.5
            b.view(-1)[e] = 0.5 + dd
        img.append(torch.full((m,), float(i)))
        labr.append(l)
        rinw.append(torch.where(fg, torch.where(rhalf, 0.5, 1.0), 0.0))
        routw.append(fg * (1.0 / 3.0))
        rtg.append(t)
        box.append(b)
    if junk:
        for bad in (-1.0, float(N)):
            l = torch.ones((1,), dtype=torch.int64)
            cls.append(R.make_logits(g, 1, K, l, "normal"))
            box.append((torch.randn((1, 4 * K), generator=g) * 0.5).float())
            rtg.append(torch.randn((1, 4 * K), generator=g) * 0.5)
            fg = cols == 1
            rinw.append(torch.where(fg, 1.0, 0.0))
            routw.append(fg * (1.0 / 3.0))
            img.append(torch.full((1,), bad))
            labr.append(l)
    img, labr = torch.cat(img), torch.cat(labr)
    Rn = img.numel()
    order = torch.randperm(Rn, generator=g) if shuffle else torch.arange(Rn)
    rois = torch.zeros((Rn, 5))
    rois[:, 0] = img[order]
    rois[:, 1:] = torch.rand((Rn, 4), generator=g) * 100.0
    take = lambda parts: torch.cat(parts, 0)[order].float().contiguous()
    c.update(rois=rois, labels=labr[order].to(torch.int32).view(Rn, 1), cls=take(cls), box=take(box), tg=take(rtg),
             inw=take(rinw), outw=take(routw), dims=(N, H, W, A, N), n_rows=Rn, rows_total=Rn, K=K,
             gl=torch.ones((4,), dtype=torch.float32), name="val%d" % seed)
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}


def slice_case(c, i):
    """Image i of a case as a single-image case for mt_reference: rpn_* sliced on dimension 0; the rows whose image
    column is i, in list order.  Rows with a label outside [0, K) stay in the slice with their box weights zeroed:
    that is the per-image rule for loss_box (such a row contributes to nothing), stated in the reference's own terms
    (it sums the box term over every row of the case)."""
    N, H, W, A, _ = c["dims"]
    rows = (c["rois"][:, 0] == i).nonzero().squeeze(1)
    lab = c["labels"][rows]
    live = ((lab >= 0) & (lab < c["K"])).to(torch.float32)
    s = {k: c[k][i:i + 1].contiguous() for k in ("rpn_cls", "rpn_labels", "rpn_box", "rpn_tg", "rpn_inw", "rpn_outw")}
    s.update(cls=c["cls"][rows], box=c["box"][rows], tg=c["tg"][rows], inw=c["inw"][rows], outw=c["outw"][rows] * live,
             labels=lab, dims=(1, H, W, A, 1), n_rows=int(rows.numel()), rows_total=int(rows.numel()), K=c["K"],
             gl=c["gl"], name="%s[%d]" % (c["name"], i))
    return s


def layer_args(c):
    """(rpn_cls_score, rpn_bbox_pred, cls_score, bbox_pred, rpn_data, roi_data) as the ops take them"""
    return (c["rpn_cls"], c["rpn_box"], c["cls"], c["box"], (c["rpn_labels"], c["rpn_tg"], c["rpn_inw"], c["rpn_outw"]),
            (c["rois"], c["labels"], c["tg"], c["inw"], c["outw"]))


def per_image_ratios(c, losses, log=None):
    """checks every image's four values against mt_reference of its slice with the bounds counted there (mt_ratios;
    the gradients are not part of this op); -> the references, for further use"""
    refs = []
    for i in range(c["dims"][0]):
        s = slice_case(c, i)
        ref = R.mt_reference(s)
        refs.append(ref)
        r = R.mt_ratios(ref, losses[i], ref["grads"])
        R.check_ratios(s["name"], {k: v for k, v in r.items() if k.startswith("v_")}, log)
    return refs
