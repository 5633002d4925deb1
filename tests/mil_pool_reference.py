"""Shared by test_mil_pool_cpu.py and test_gpu_mil_pool.py (and tools/mil_fuzz.py): a plain float64 statement of the
MIL term under any pair of the five bag functions of mil/core.py -- mal-max, ben-max, mass-max, disc-max (they select
a row) and mean-ben (it pools) --, of the weighted cross-entropy, of the mean over the bags and of the gradient,
written from the reference's formulas (mil/core.py:49-96, fast_rcnn/train_bus.py:239-260), with elementwise error
bounds counted from the roundings of csrc/mil.hip.  torch only, any device, no import of the package.

The bounds of the cross-entropy itself are loss_reference's (bound_ce_term, bound_ce_grad, bound_value, SLACK, the
rule for bounds and the measured allowance of expf / log1pf stated there); this module adds only what the mean
introduces.  With u = 2^-24, e = 2^-53, x the class-1 logits of the bag's cnt rows and m their mean:

  delta (bound_mean)  the error of the kernel's f32 m against the exact mean:
                        the f64 sum's reassociation (per-thread partials, then a tree: some order), cnt e sum|x| on
                        the sum, e sum|x| on the mean (the conversions of x to f64 are exact);
                        the f64 division by cnt, e |m|;
                        the one rounding of m to f32, u |m|.
  through the CE      t(m) = lse([0, m, 0, ...]) - row[label] has dt/dm = p_1 - [label == 1], which is p_1 or
                      -(1 - p_1); d(m) = p_1 - [label == 1], the class-1 component of the CE gradient, has dd/dm =
                      p_1 (1 - p_1).  The logarithmic derivatives of p_1 and of 1 - p_1 with respect to m are 1 - p_1
                      and -p_1, inside [-1, 1], so over |h| <= delta each of p_1, 1 - p_1 and their product grows by
                      at most the factor e^delta, and by the mean value theorem
                        |t(m + h) - t(m)| <= delta e^delta |p_1 - [label == 1]|        (prop_term)
                        |d(m + h) - d(m)| <= delta e^delta p_1 (1 - p_1)               (prop_grad)
                      with 1 - p_1 taken as the sum of the other probabilities, which stays accurate as p_1 -> 1.
  the gradient        g = fl(fl(c d) / cnt): fl(c d) is the CE gradient's component (bound_ce_grad with three scale
                      roundings, as for a selected row); (float)cnt is exact; the f32 division, u |g|.
  subnormal results   p_1 near e^-80 is a normal number, but c d and c d / cnt may fall below 2^-126, where a result
                      is rounded to the grid of 2^-149 or flushed to zero: 2^-126 / cnt where |c d| < 2^-126, 2^-126
                      where |g| < 2^-126 (loss_reference's rule for subnormal results, at the output itself).

No constant was chosen by looking at what a GPU produced.

DECISIONS ARE DATA.  The selected row is decided on the f32 keys exactly as the kernel does: first row with the
largest key, keys compared as f32 values.  For mean-ben the reported row is the bag's first row.  An empty bag: row
-1, zeros as its logit row, term 0, no gradient, and it counts in the mean over the bags."""
import math

import torch

import loss_reference as R

MAL_MAX, BEN_MAX, MASS_MAX, DISC_MAX, MEAN_BEN = range(5)
NAMES = ("mal_max", "ben_max", "mass_max", "disc_max", "mean_ben")
ALL_PAIRS = [(a, b) for a in range(5) for b in range(5)]
OLD_PAIRS = [(a, b) for a in range(3) for b in range(3)]


def keys(logits, sel):
    """f32 [n]: what a selecting function takes the arg-max of"""
    if sel == MAL_MAX:
        return logits[:, 2]
    if sel == BEN_MAX:
        return logits[:, 1]
    if sel == MASS_MAX:
        return -logits[:, 0]
    assert sel == DISC_MAX, sel
    return logits[:, 1:].max(1).values


def bag_selectors(c):
    """list [n_bags]: label 1 takes sel[0], any other label sel[1]"""
    return [c["sel"][0] if l == 1 else c["sel"][1] for l in c["bag_labels"].tolist()]


def select(c):
    """-> (rows int64 [n_bags], counts int64 [n_bags], members: per bag the int64 row indices)"""
    bag = R.mil_bag_of_row(c)
    nb = c["n_bags"]
    rows = torch.full((nb,), -1, dtype=torch.int64, device=bag.device)
    counts = torch.zeros((nb,), dtype=torch.int64, device=bag.device)
    members = []
    for b, sel in enumerate(bag_selectors(c)):
        idx = (bag == b).nonzero().squeeze(1)
        members.append(idx)
        counts[b] = idx.numel()
        if idx.numel() == 0:
            continue
        if sel == MEAN_BEN:
            rows[b] = idx[0]
        else:
            k = keys(c["logits"][idx], sel)
            rows[b] = idx[(k == k.max()).nonzero().squeeze(1)[0]]
    return rows, counts, members


def exact_mean(x):
    """(mean, sum|x|) of f32 values, the sums exact (math.fsum), the division in f64"""
    v = x.double().tolist()
    return math.fsum(v) / len(v), math.fsum(abs(a) for a in v)


def bound_mean(cnt, sum_abs, m):
    """delta: f64 reassociation cnt e sum|x| / cnt, the f64 division e|m|, the rounding to f32 u|m| (module docstring)"""
    return R.SLACK * (R.E * sum_abs + (R.E + R.U) * abs(m))


def _p1_q1(ce):
    """(p_1, 1 - p_1 as the sum of the other probabilities)"""
    p1 = ce["p"][:, 1]
    return p1, ce["p"].sum(1) - p1


def prop_term(ce, delta):
    """[n_bags]: |t(m + h) - t(m)| for |h| <= delta"""
    p1, q1 = _p1_q1(ce)
    return delta * torch.exp(delta) * torch.where(ce["onehot"][:, 1], q1, p1)


def prop_grad(ce, delta):
    """[n_bags]: |d(m + h) - d(m)| for |h| <= delta, d the class-1 component of softmax - onehot"""
    p1, q1 = _p1_q1(ce)
    return delta * torch.exp(delta) * p1 * q1


def reference(c):
    """One case (a dict as loss_reference.make_mil_case makes them, `sel` a pair of 0..4) in f64 with bounds.
    -> dict: rows, counts (exact); bag_logits [n_bags, K] / b_logits; bag_loss / b_bag; loss / b_loss; grad [R, K] /
    b_grad; zero: bool [R, K], the gradient elements that must be exactly 0; pooled: bool [n_bags]; args, z1: what the
    case hands to expf / log1pf (for the allowance)."""
    logits, K, nb = c["logits"], c["K"], c["n_bags"]
    dev = logits.device
    rows, counts, members = select(c)
    sels = bag_selectors(c)
    valid = rows >= 0
    pooled = torch.tensor([s == MEAN_BEN for s in sels], dtype=torch.bool, device=dev) & valid
    lab = c["bag_labels"].long()
    live = valid & (lab >= 0) & (lab < K)

    row64 = logits[rows.clamp_min(0)].double() * valid.unsqueeze(1)
    delta = torch.zeros((nb,), dtype=torch.float64, device=dev)
    for b in range(nb):
        if bool(pooled[b]):
            m, sum_abs = exact_mean(logits[members[b], 1])
            row64[b] = 0.0
            row64[b, 1] = m
            delta[b] = bound_mean(int(counts[b]), sum_abs, m)
    b_logits = torch.zeros_like(row64)
    b_logits[:, 1] = delta

    ce = R.ce_parts(row64, lab.clamp(0, K - 1))
    w = c["cw"].double()[lab.clamp(0, K - 1)] * live
    bag_loss = w * ce["t"]
    b_bag = R.bound_mil_bag_loss(ce, w) + R.SLACK * w.abs() * prop_term(ce, delta)
    scale = float(torch.tensor(c["scale"], dtype=torch.float32).double())
    wt = scale / nb
    loss = wt * float(bag_loss.sum())
    b_loss = R.bound_value(b_bag, bag_loss.abs(), wt, loss, nb)

    gl = float(c["gl"].double())
    cs = gl * scale * w / nb
    g_rows = R.ce_grad(ce, cs)                                     # [n_bags, K]: c (softmax - onehot) of the bag's row
    b_rows = R.bound_ce_grad(ce, cs, 3) * (cs != 0).unsqueeze(1)
    grad = torch.zeros((logits.shape[0], K), dtype=torch.float64, device=dev)
    b_grad = torch.zeros_like(grad)
    zero = torch.ones((logits.shape[0], K), dtype=torch.bool, device=dev)
    for b in range(nb):
        if not bool(valid[b]) or float(cs[b]) == 0.0:
            continue
        if bool(pooled[b]):
            cnt = float(counts[b])
            cd = float(g_rows[b, 1])
            g = cd / cnt
            bound = (float(b_rows[b, 1]) + R.SLACK * abs(float(cs[b])) * float(prop_grad(ce, delta)[b])) / cnt \
                + R.SLACK * R.U * abs(g)
            if abs(cd) < R.TINY:
                bound += R.TINY / cnt
            if abs(g) < R.TINY:
                bound += R.TINY
            grad[members[b], 1] = g
            b_grad[members[b], 1] = bound
            zero[members[b], 1] = False
        else:
            grad[rows[b]] = g_rows[b]
            b_grad[rows[b]] = b_rows[b]
            zero[rows[b]] = False
    pick = live & (w != 0)
    return dict(rows=rows, counts=counts, pooled=pooled, bag_logits=row64, b_logits=b_logits, bag_loss=bag_loss,
                b_bag=b_bag, loss=loss, b_loss=b_loss, grad=grad, b_grad=b_grad, zero=zero,
                args=ce["arg32"][pick].reshape(-1).float(), z1=ce["z1"][pick].float())


def ratios(ref, loss=None, bag_loss=None, grad=None, bag_logits=None):
    """worst |error| / bound of whichever outputs are given"""
    r = {}
    if loss is not None:
        r["pool_loss"] = R.ratio(loss, ref["loss"], ref["b_loss"])
    if bag_loss is not None:
        r["pool_bag_loss"] = R.ratio(bag_loss, ref["bag_loss"], ref["b_bag"])
    if grad is not None:
        r["pool_grad"] = R.ratio(grad, ref["grad"], ref["b_grad"])
    if bag_logits is not None:
        r["pool_bag_logits"] = R.ratio(bag_logits, ref["bag_logits"], ref["b_logits"])
    return r


def host_tolerance(c, ref):
    """-> (tolerance of the loss, tolerance [R, K] of the gradient) for the UNFUSED routes of train_bus.mil_loss: the
    host restatement on CPU tensors, and on the device the selection op followed by torch's own mean and
    cross-entropy.  That is torch's f32 arithmetic (a mean, log_softmax, a few products), whose kernels are not this
    project's to count rounding by rounding.  The tolerance therefore comes from the number format, u = 2^-24:
      m of a mean-ben bag   at worst an f32 sum of cnt terms in some order and one division: u (sum|x| + |m|), carried
                            through the cross-entropy by prop_term / prop_grad;
      a bag's term          16 roundings of the largest magnitude it is made of: 16 u (max|row| + t + 1);
      the loss              the weighted mean of those, and 8 u |loss| for the products and the mean (the scale factor
                            taken as f32 or as f64 included);
      a gradient element    |c| (16 u + the carried error of m) / cnt + 16 u |g|."""
    U = R.U
    nb, K = c["n_bags"], c["K"]
    lab = c["bag_labels"].long().clamp(0, K - 1)
    w = c["cw"].double()[lab] * (ref["rows"] >= 0)
    wt = float(torch.tensor(c["scale"], dtype=torch.float32)) / nb
    _, counts, members = select(c)
    delta = torch.zeros((nb,), dtype=torch.float64, device=w.device)
    for b in range(nb):
        if bool(ref["pooled"][b]):
            m, sum_abs = exact_mean(c["logits"][members[b], 1])
            delta[b] = U * (sum_abs + abs(m))
    ce = R.ce_parts(ref["bag_logits"], lab)
    tol_t = 16 * U * (ref["bag_logits"].abs().max(1).values + ce["t"] + 1.0) + prop_term(ce, delta)
    tol_loss = wt * float((w * tol_t).sum()) + 8 * U * abs(ref["loss"])
    cs = (abs(float(c["gl"])) * wt * w).abs()
    tol_g = torch.zeros_like(ref["grad"])
    for b in range(nb):
        if bool(ref["pooled"][b]):
            tol_g[members[b], 1] = float(cs[b]) * (16 * U + float(prop_grad(ce, delta)[b])) / float(counts[b])
        elif int(ref["rows"][b]) >= 0:
            tol_g[ref["rows"][b]] = float(cs[b]) * 16 * U
    return tol_loss, tol_g + 16 * U * ref["grad"].abs()


# ---------------------------------------------------------------- kernel model (torch f32 on the CPU)

def model(c):
    """csrc/mil.hip's arithmetic with torch's exp / log1p standing in for the device's -> (rows, counts, bag_logits
    f32, bag_loss f32, loss f32, grad f32).  The mean: an f64 sum (torch's order, not the kernel's), the f64 division,
    one rounding to f32."""
    logits, K, nb = c["logits"], c["K"], c["n_bags"]
    rows, counts, members = select(c)
    sels = bag_selectors(c)
    valid = rows >= 0
    lab = c["bag_labels"].long()
    bag_logits = logits[rows.clamp_min(0)] * valid.unsqueeze(1)
    for b in range(nb):
        if sels[b] == MEAN_BEN and bool(valid[b]):
            bag_logits[b] = 0.0
            bag_logits[b, 1] = (logits[members[b], 1].double().sum() / float(counts[b])).float()
    w = c["cw"][lab.clamp(0, K - 1)] * valid
    t, p, others, onehot = R.model_ce(bag_logits.contiguous(), lab.clamp(0, K - 1))
    bag_loss = torch.where(valid, w * t, torch.zeros_like(t))
    scale = torch.tensor(c["scale"], dtype=torch.float64).float()
    loss = (scale.double() * bag_loss.double().sum() / float(nb)).float()
    cs = ((c["gl"] * scale) * w) / torch.tensor(float(nb))
    g = torch.where(onehot, (-others).unsqueeze(1) * cs.unsqueeze(1), p * cs.unsqueeze(1))
    grad = torch.zeros((logits.shape[0], K))
    for b in range(nb):
        if not bool(valid[b]):
            continue
        if sels[b] == MEAN_BEN:
            grad[members[b], 1] = g[b, 1] / counts[b].float()
        else:
            grad[rows[b]] = g[b]
    return rows, counts, bag_logits, bag_loss, loss, grad


# ---------------------------------------------------------------- cases

FRONT, BACK = 3, 4          # rows of no bag in front (negative bag index) and behind (>= n_bags)

# name: (K, bag sizes, bag labels, bag_offset (4: strided column 0 of an [R, 5] blob), regime)
CASES = {
    # one and two strides of the 256-thread scan, a single-row bag next to an empty one in the middle
    "mixed_k3": (3, [1, 0, 257, 300], [1, 2, 1, 2], 0.0, "mixed"),
    "mixed_k5": (5, [1, 0, 257, 300], [2, 1, 2, 1], 4.0, "mixed"),
    # one more bag than a block of the bag-term kernel holds
    "bags65_k3": (3, [1 + (b * 7) % 3 for b in range(65)], [1 + (b % 2) for b in range(65)], 4.0, "normal"),
    "bags65_k5": (5, [1 + (b * 5) % 3 for b in range(65)], [1 + ((b // 2) % 2) for b in range(65)], 0.0, "normal"),
    # class-1 logits near +80 and -80 under both labels: p_1 -> 1 and -> 0
    "underflow_k3": (3, [3, 2, 5, 4, 1, 1], [1, 2, 1, 2, 2, 1], 0.0, "underflow"),
    "underflow_k5": (5, [3, 2, 5, 4, 1, 1], [1, 2, 1, 4, 2, 1], 4.0, "underflow"),
}
DISC_WINNER = {2: 1, 3: -1}     # "mixed": the class that carries a disc-max bag's winning key, by bag (-1: class K-1)


def make_case(name, sel, device="cpu"):
    """One case for the selector pair `sel` (fixed seed by name; the same scores for every pair, then, per bag, what
    that bag's function is sensitive to):

      a selecting bag of >= 257 rows   its extremal row is moved to bag row r0 and copied to r0 + 1 (the neighbouring
                                       thread of the scan) and r0 + 256 (the same thread, one stride on): three equal
                                       keys, the lowest index must win.  Under disc-max the winning key first is put
                                       into class 1 (bag 2) or class K-1 (bag 3), above every other logit of the bag;
      a pooling bag, regime "mixed"    bag 2: half of the class-1 logits are +- pairs of magnitude ~1000, the other half
                                       of magnitude 1e-3, in random order: the sum nearly cancels, and only an f64
                                       accumulation keeps what the small ones add;
      regime "underflow"               class-1 logits of bags 0..3 within 0.5 of +80, +80, -80, -80, of bags 4, 5
                                       (one row) +80 and -80 exactly.

    Rows of no bag stand in front (negative bag index after the offset) and behind (>= n_bags) with logits that would
    win every selection and move every mean."""
    K, sizes, labels, offset, regime = CASES[name]
    idx = list(CASES).index(name)
    g = torch.Generator().manual_seed(9000 + idx)
    nb = len(sizes)
    bag_labels = torch.tensor(labels, dtype=torch.int32)
    bag = torch.cat([torch.full((FRONT,), -2.0), torch.repeat_interleave(torch.arange(nb), torch.tensor(sizes)).float(),
                     torch.full((BACK,), nb + 3.0)])
    Rn = bag.numel()
    logits = (torch.randn((Rn, K), generator=g) * 2.0).float()
    start = FRONT
    for b, n in enumerate(sizes):
        s = sel[0] if labels[b] == 1 else sel[1]
        blk = logits[start:start + n]
        if regime == "underflow":
            centre = [80.0, 80.0, -80.0, -80.0, 80.0, -80.0][b]
            blk[:, 1] = centre + (0.0 if n == 1 else 1.0) * (torch.rand((n,), generator=g) - 0.5)
        if s == MEAN_BEN and regime == "mixed" and b == 2:
            q = n // 4
            a = (500.0 + 1000.0 * torch.rand((q,), generator=g)).float()
            x = torch.cat([a, -a[torch.randperm(q, generator=g)], 1e-3 * torch.randn((n - 2 * q,), generator=g)])
            blk[:, 1] = x[torch.randperm(n, generator=g)]
        if s != MEAN_BEN and n >= 257:
            if s == DISC_MAX:
                orig = int(keys(blk, s).argmax())
                cls = DISC_WINNER[b] % K
                blk[orig, 1:] = blk[orig, 1:].min() - 1.0
                blk[orig, cls] = blk[:, 1:].max() + 1.5
            orig = int(keys(blk, s).argmax())
            r0 = int(torch.randint(0, n - 256, (1,), generator=g))
            keep = blk[r0].clone()
            blk[r0] = blk[orig]
            blk[orig] = keep
            blk[r0 + 1] = blk[r0]
            blk[r0 + 256] = blk[r0]
        start += n
    for junk in (slice(0, FRONT), slice(Rn - BACK, Rn)):
        logits[junk, 0] = logits[:, 0].min() - 5.0
        logits[junk, 1:] = logits[:, 1:].max() + 5.0
    if offset:
        blob = torch.zeros((Rn, 5))
        blob[:, 0] = bag + offset
        blob[:, 1:] = torch.randn((Rn, 4), generator=g)
        col_t = blob.to(device)[:, 0]
    else:
        col_t = bag.to(device)
    cw = torch.full((K,), 0.5)
    cw[0], cw[1], cw[2] = 0.0, R.MIL_PCT, 1.0 - R.MIL_PCT
    return dict(name=name, K=K, n_bags=nb, sel=tuple(sel), offset=offset, regime=regime, sizes=sizes,
                logits=logits.contiguous().to(device), col=col_t, bag_labels=bag_labels.to(device),
                cw=cw.float().to(device), scale=0.5 + 0.01 * idx,
                gl=torch.tensor(-1.7 if idx % 2 else 0.6, dtype=torch.float32, device=device))


def make_host_case(sel, seed=0):
    """A K = 3 case the host restatement (mil.core.get_bag_logit: grouped rows, bags counted from 0, no empty bag) can
    take: bags of 1, 40, 7 and 2 rows, labels 1, 2, 1, 2, every row of some bag, N(0, 2) scores."""
    g = torch.Generator().manual_seed(9500 + seed)
    sizes, labels = [1, 40, 7, 2], [1, 2, 1, 2]
    bag = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).float()
    logits = (torch.randn((bag.numel(), 3), generator=g) * 2.0).float()
    cw = torch.tensor([0.0, R.MIL_PCT, 1.0 - R.MIL_PCT])
    return dict(name="host", K=3, n_bags=len(sizes), sel=tuple(sel), offset=0.0, regime="normal", sizes=sizes,
                logits=logits, col=bag, bag_labels=torch.tensor(labels, dtype=torch.int32), cw=cw, scale=0.37,
                gl=torch.tensor(1.0))
