"""Shared by test_loss_reference_cpu.py and test_gpu_loss_reference.py: a plain float64 statement of the fused losses
(csrc/loss.hip: the four supervised terms; csrc/mil.hip: bag selection and the MIL term) and of their gradients,
elementwise error bounds counted from the kernels' roundings, case makers that sit on the kernels' own boundaries,
and a torch-f32 model of the kernels' arithmetic with switches that seed defects.  torch only, any device, no import
of the package.

THE RULE FOR BOUNDS (as in rowbn_reference.py).  u = 2^-24 is the unit roundoff of f32, e = 2^-53 that of f64.  Every
f32 rounding on an output's path costs u times the magnitude of the term it rounds; a rounding of an intermediate
reaches the output multiplied by whatever the intermediate is multiplied by; an error eta of an exponent reaches
exp() as the factor expm1(eta).  Each bound's docstring lists the roundings it counts.  SLACK = 1 + 2^-20 multiplies
every bound (products of two error terms, the rounding of the f64 reference itself) and is fixed in advance.  No
constant was chosen by looking at what a GPU produced.

LIBRARY FUNCTIONS.  expf and log1pf are the device library's; their accuracy is measured, not assumed: lib_accuracy()
gives the worst error in ulp against f64 over lib_grids() plus the arguments the cases produce, and set_allowance()
turns it into the allowance the bounds use (the measured worst rounded up to the next integer, plus 1 ulp for
arguments off the grid; at most MAX_ALLOWANCE = 4 ulp, more is a finding, not something to absorb).  A relative
error of a ulp is at most 2 a u.  Results below 2^-126 (subnormal) may be flushed to zero and nothing else: there the
comparison is absolute, 2^-126 times whatever multiplies the result; only the case named "underflow" holds such
elements (checked by subnormal_count()).

DECISIONS ARE DATA.  What a kernel decides on an f32 value is decided here on the same IEEE f32 value: d = pred - tg
(one f32 subtraction, identical on every machine) for |d| < 1 and sgn(d); the arg-max km with first-wins ties; the
label tests.  So no element is left out of any comparison.  Padding rows (label -1) carry zero box weights in every
case, as everywhere in the project: the op sums the box term over the first n_rows rows and divides by the count of
labelled rows.
"""
import math

import torch

U = 2.0 ** -24
E = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -20
TINY = 2.0 ** -126
BLOCK_ELEMS = 2048          # MTL_BLOCK * MTL_ITEMS: elements per workgroup of the RPN terms
ROW_BLOCK = 256             # rows per workgroup of the R-CNN backward; threads per bag of the selection
MAX_ALLOWANCE = 4
ALLOW = {}                  # "exp", "log1p": ulp; set by set_allowance()
SEL_COL = {0: (2, 1.0), 1: (1, 1.0), 2: (0, -1.0)}    # selector -> (column, sign): mal-max, ben-max, mass-max (arg-min)


# ---------------------------------------------------------------- library accuracy

def lib_grids(device="cpu"):
    """f32 arguments: expf dense over [-104, 0] (exp underflows to 0 below -103.3); log1pf over [0, 31] (z1 is a sum
    of at most 31 terms <= 1) plus very small arguments down to the subnormals."""
    ex = torch.linspace(-104.0, 0.0, 832001, dtype=torch.float64, device=device).float()
    small = torch.tensor([2.0 ** -k for k in range(1, 150)], dtype=torch.float64, device=device).float()
    lg = torch.cat([torch.linspace(0.0, 31.0, 496001, dtype=torch.float64, device=device).float(), small,
                    small * 1.2345])
    return ex, lg


def lib_accuracy(got, exact):
    """got f32, exact f64 (> 0 or 0).  -> (worst error in ulp over the normal results, worst error in units of 2^-149
    over the subnormal results that were not flushed, number flushed to zero)."""
    got, exact = got.double().reshape(-1), exact.reshape(-1)
    normal = exact >= TINY
    _, ex = torch.frexp(exact[normal])                        # exact = mant * 2^ex, mant in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(exact[normal]), ex - 24)
    worst = float(((got[normal] - exact[normal]).abs() / ulp).max()) if bool(normal.any()) else 0.0
    sub = ~normal & (exact > 0)
    flushed = sub & (got == 0) & (exact > 2.0 ** -150)         # below 2^-150 zero is the correctly rounded result
    kept = sub & (got != 0)
    worst_sub = float(((got[kept] - exact[kept]).abs() / 2.0 ** -149).max()) if bool(kept.any()) else 0.0
    zero_ok = bool((got[exact == 0] == 0).all())
    assert zero_ok, "a result that is exactly 0 in f64 is not 0"
    return worst, worst_sub, int(flushed.sum())


def set_allowance(exp_worst, log1p_worst):
    """the measured worst errors (ulp) -> the allowance of the bounds: next integer up, plus 1"""
    for name, w in (("exp", exp_worst), ("log1p", log1p_worst)):
        a = int(math.ceil(w)) + 1
        assert a <= MAX_ALLOWANCE, "%sf is %.3g ulp off at worst: allowance %d exceeds %d ulp" % (name, w, a, MAX_ALLOWANCE)
        ALLOW[name] = a
    return dict(ALLOW)


def _allow(name):
    assert name in ALLOW, "measure the library functions first (set_allowance)"
    return ALLOW[name]


# ---------------------------------------------------------------- softmax cross-entropy: reference and bounds

def _first_max(s):
    """(max [n,1], bool [n,K] true at the first maximal column: the kernels' km)"""
    m = s.max(1, keepdim=True).values
    eq = s == m
    return m, eq & (eq.cumsum(1) == 1)


def ce_parts(s, lab):
    """s [n, K] f32, lab [n] int64 in [0, K).  f64 of the f32 inputs: d = s - max, ex = exp(d), z1 = sum of ex without
    the first maximum's own term (ties add exact ones), lz = log1p(z1), the term t = (m - s_l) + lz, the softmax p =
    exp(d - lz) and `others` = 1 - p_l as the sum of the other probabilities."""
    s64 = s.double()
    K = s.shape[1]
    m, first = _first_max(s64)
    d = s64 - m
    ex = torch.exp(d)
    z1 = (ex * ~first).sum(1)
    lz = torch.log1p(z1)
    onehot = torch.zeros_like(first).scatter_(1, lab.view(-1, 1), True)
    sl = (s64 * onehot).sum(1)
    gap = m.squeeze(1) - sl
    p = torch.exp(d - lz.unsqueeze(1))
    others = (p * ~onehot).sum(1)
    arg32 = s - s.max(1, keepdim=True).values                   # what expf is handed: the forward's, the backward's
    return dict(K=K, d=d, ex=ex, first=first, z1=z1, lz=lz, gap=gap, t=gap + lz, p=p, onehot=onehot, others=others,
                arg32=torch.stack([arg32, arg32 - lz.float().unsqueeze(1)], 2))


def _lz_err(c):
    """absolute error of lz = log1pf(z1), z1 = sum_{k != km} expf(fl(s_k - m)):
      each argument's rounding, u|d_k|, through exp: ex_k expm1(u|d_k|); expf's own error, 2 a_exp u ex_k; a result
      below 2^-126 may be flushed: 2^-126;  the K-2 adds of z1 that round (the first add to 0 is exact), each u z1;
      through log1p, whose slope is at most 1 / (1 + z1 - Z);  log1pf's own error, 2 a_log1p u lz (2^-126 when lz is
      subnormal)."""
    ad = c["d"].abs()
    ek = c["ex"] * (torch.expm1(U * ad) + 2 * _allow("exp") * U) + TINY * (c["ex"] < TINY)
    Z = (ek * ~c["first"]).sum(1) + max(c["K"] - 2, 0) * U * c["z1"]
    return Z / (1.0 + (c["z1"] - Z).clamp_min(0.0)) + 2 * _allow("log1p") * U * c["lz"] + TINY * (c["lz"] < TINY)


def bound_ce_term(c):
    """[n].  t = fl(fl(m - s_l) + lz): the subtraction, u|m - s_l|; lz's error (_lz_err: the exp arguments'
    roundings, expf, the K-2 adds of z1, log1pf); the final add, u t."""
    return SLACK * (U * c["gap"].abs() + _lz_err(c) + U * c["t"])


def bound_ce_grad(c, scale, scale_roundings=1):
    """[n, K], for g_k = fl(expf(fl(fl(s_k - m) - lz)) * scale) and g_l = fl(-(sum of the others' expf) * scale), scale
    [n] or scalar in f64 (the kernel's is that value after `scale_roundings` f32 roundings).
      exponent: the first subtraction u|d_k|, lz's error, the second subtraction u(|d_k| + lz): eta_k; p_k expm1(eta_k)
      expf: 2 a_exp u p_k (p_k < 2^-126: 2^-126 in all, flushing allowed)
      scale: scale_roundings u |g_k|; the product: u |g_k|
      label's component: the others' errors summed, and the K-2 adds of the sum that round, u (sum of others) each,
      then scale and product as above.
    There is no term in |m|."""
    sc = scale if torch.is_tensor(scale) else torch.tensor(float(scale), dtype=torch.float64, device=c["d"].device)
    sc = sc.abs().reshape(-1, 1)
    ad, lz = c["d"].abs(), c["lz"].unsqueeze(1)
    eta = U * ad + _lz_err(c).unsqueeze(1) + U * (ad + lz)
    pe = c["p"] * (torch.expm1(eta) + 2 * _allow("exp") * U)
    pe = torch.where(c["p"] < TINY, torch.full_like(pe, TINY), pe)
    oe = (pe * ~c["onehot"]).sum(1, keepdim=True) + max(c["K"] - 2, 0) * U * c["others"].unsqueeze(1)
    mag = torch.where(c["onehot"], c["others"].unsqueeze(1), c["p"]) * sc
    return SLACK * (sc * torch.where(c["onehot"], oe, pe) + (scale_roundings + 1) * U * mag)


def ce_grad(c, scale):
    """[n, K] f64: softmax - onehot, the label's component as -(sum of the others), times scale"""
    sc = scale.reshape(-1, 1) if torch.is_tensor(scale) else scale
    return torch.where(c["onehot"], -c["others"].unsqueeze(1), c["p"]) * sc


def bound_value(per_bounds, per_abs, weight, value, n):
    """A loss value (float)(weight * sum): the f64 sum of the per-element bounds times the mean's weight; the f64
    sum's own (n + 4) e (sum of magnitudes); the one rounding to f32, u|value|."""
    return SLACK * (abs(weight) * (float(per_bounds.sum()) + (n + 4) * E * float(per_abs.sum())) + U * abs(value))


def subnormal_count(c):
    """elements whose reference exp / probability / log1p is below 2^-126 (and not 0)"""
    return int(((c["p"] < TINY) & (c["p"] > 0)).sum() + ((c["ex"] < TINY) & (c["ex"] > 0)).sum()
               + ((c["lz"] < TINY) & (c["lz"] > 0)).sum()) + int((c["ex"] == 0).sum() + (c["p"] == 0).sum())


# ---------------------------------------------------------------- multi-task loss: layouts, reference, bounds

def rpn_views(c):
    """anchor order e = ((n*H + h)*W + w)*A + a: scores [n_anchor, 2] (bg, fg), labels [n_anchor]; box element order
    = rpn_bbox_pred's own: targets / weights [N, H, W, 4A]"""
    N, H, W, A, _ = c["dims"]
    s2 = c["rpn_cls"].view(N, H, W, 2, A).permute(0, 1, 2, 4, 3).reshape(-1, 2)
    lab = c["rpn_labels"].view(N, A, H, W).permute(0, 2, 3, 1).reshape(-1).long()
    nhwc = [t.permute(0, 2, 3, 1) for t in (c["rpn_tg"], c["rpn_inw"], c["rpn_outw"])]
    return s2, lab, nhwc


def _scatter_scores(g2, dims):
    N, H, W, A, _ = dims
    return g2.view(N, H, W, A, 2).permute(0, 1, 2, 4, 3).reshape(N, H, W, 2 * A)


def bound_rpn_box_term(d32, d64, iw, ow, ref):
    """[...], the forward element fl(ow * per), d32 = fl(pred - tg) deciding the branch:
      |d| < 1, per = fl(fl(0.5 q) q), q = fl(fl(iw d) 3): d's rounding, the two products of q (3u on q, 6u on q^2;
               0.5 q is exact), the product q q, the product with ow: 8u|ref|
      else,    per = fl(|d| - c), c = (float)(0.5 / 9): d's rounding u|d|, c's u c, the subtraction u||d| - c|, each
               times |ow|; the product with ow, u|ref|."""
    inner = d32.abs() < 1.0
    ad = d64.abs()
    other = ow.abs() * U * (ad + 0.5 / 9.0 + (ad - 0.5 / 9.0).abs()) + U * ref.abs()
    return SLACK * torch.where(inner, 8 * U * ref.abs(), other)


def bound_rpn_box_grad(d32, ref):
    """[...], g = fl(fl(ow X) scale): |d| < 1, X = fl(fl(fl(9 iw) iw) d): d's rounding and 3 products, 4u; ow X: u;
    scale = (float)(10 gl / (n_box_images 4 A)): u (its f64 arithmetic: 4e); the last product: u -- 7u|ref|.  Else X =
    sgn(d) exactly: 3u|ref|.  Images beyond n_box_images: exactly 0."""
    return SLACK * torch.where(d32.abs() < 1.0, 7.0, 3.0) * (U + 4 * E) * ref.abs()


def bound_rcnn_box_row(terms_abs, K):
    """[n_rows], row = f32 sum over 4K columns of fl(outw fl(inw |fl(pred - tg)|)): 3 roundings per term, 3u sum|term|;
    the 4K-1 adds that round, each u sum|term|."""
    return SLACK * (3 + 4 * K - 1) * U * terms_abs.sum(1)


def bound_rcnn_box_grad(ref):
    """[rows, 4K], g = fl(fl(fl(outw inw) sgn) sc_box): outw inw, u; times sgn, exact; sc_box = (float)(gl / rows), u
    (its f64 division: 2e); the product, u -- 3u|ref|.  Rows beyond n_rows: exactly 0."""
    return SLACK * 3 * (U + 2 * E) * ref.abs()


def mt_reference(c):
    """The four terms and the four gradient tensors of one multi-task case in f64, with their bounds.
    -> dict(terms [4] (term 2 NaN without labelled rows), b_terms [4], grads / b_grads: rpn_cls, rpn_box, cls, box,
    zero: bool masks of the elements that must be exactly 0, sub: count of subnormal exp results, args: the f32
    arguments the case hands to expf)."""
    N, H, W, A, nbi = c["dims"]
    n_rows, rows_total, K = c["n_rows"], c["rows_total"], c["K"]
    gl = c["gl"].double()
    dev = c["rpn_cls"].device
    terms, b_terms = [], []

    # RPN cross-entropy: mean over the anchors with label != -1; the label's score is fg for any label != 0
    s2, lab, (tg, iw, ow) = rpn_views(c)
    on = lab >= 0
    ce = ce_parts(s2, ((lab != 0) & on).long())
    cnt = float(on.sum())
    terms.append(float((ce["t"] * on).sum()) / cnt if cnt else float("nan"))
    b_terms.append(bound_value(bound_ce_term(ce) * on, ce["t"] * on, 1.0 / max(cnt, 1.0), terms[0], on.numel()))
    sc0 = float(gl[0]) / cnt if cnt else 0.0
    g_cls2 = ce_grad(ce, sc0) * on.unsqueeze(1)
    b_cls2 = bound_ce_grad(ce, sc0) * on.unsqueeze(1) * (1.0 if float(gl[0]) != 0 else 0.0)
    sub = subnormal_count({k: (v[on] if torch.is_tensor(v) else v) for k, v in ce.items()})
    args = [ce["arg32"][on].reshape(-1)]

    # RPN box: 10 * mean over (image, channel) of the first n_box_images images
    pred = c["rpn_box"]
    d32 = pred - tg
    d64 = pred.double() - tg.double()
    iw64, ow64 = iw.double(), ow.double()
    inner = d32.abs() < 1.0
    per = torch.where(inner, 0.5 * (iw64 * d64 * 3.0) ** 2, d64.abs() - 0.5 / 9.0)
    el = ow64 * per
    w1 = 10.0 / (nbi * 4.0 * A)
    terms.append(w1 * float(el[:nbi].sum()))
    b_terms.append(bound_value(bound_rpn_box_term(d32, d64, iw64, ow64, el)[:nbi], el[:nbi].abs(), w1, terms[1],
                               el[:nbi].numel()))
    sgn = torch.sign(d32).double()
    g_rbox = ow64 * torch.where(inner, 9.0 * iw64 * iw64 * d64, sgn) * (w1 * float(gl[1]))
    g_rbox[nbi:] = 0.0
    b_rbox = bound_rpn_box_grad(d32, g_rbox)

    # R-CNN terms over the first n_rows rows; rows with label -1 are padding
    labr = c["labels"].reshape(-1).long()
    live = (labr >= 0) & (labr < K)
    rc = float(live.sum())
    cr = ce_parts(c["cls"][:n_rows], labr.clamp(0, K - 1))
    terms.append(float((cr["t"] * live).sum()) / rc if rc else float("nan"))
    b_terms.append(bound_value(bound_ce_term(cr) * live, cr["t"] * live, 1.0 / max(rc, 1.0),
                               terms[2] if rc else 0.0, n_rows))
    sc2 = float(gl[2]) / rc if rc else 0.0
    g_cls = torch.zeros((rows_total, K), dtype=torch.float64, device=dev)
    b_cls = torch.zeros_like(g_cls)
    g_cls[:n_rows] = ce_grad(cr, sc2) * live.unsqueeze(1)
    b_cls[:n_rows] = bound_ce_grad(cr, sc2) * live.unsqueeze(1) * (1.0 if sc2 != 0 else 0.0)
    sub += subnormal_count({k: (v[live] if torch.is_tensor(v) else v) for k, v in cr.items()})
    args.append(cr["arg32"][live].reshape(-1))

    bd32 = c["box"][:n_rows] - c["tg"]
    bd64 = c["box"][:n_rows].double() - c["tg"].double()
    rel = c["outw"].double() * (c["inw"].double() * bd64.abs())
    rows_mean = 1.0 / max(rc, 1.0)
    terms.append(rows_mean * float(rel.sum()))
    b_terms.append(bound_value(bound_rcnn_box_row(rel.abs(), K), rel.abs().sum(1), rows_mean, terms[3], n_rows))
    g_box = torch.zeros((rows_total, 4 * K), dtype=torch.float64, device=dev)
    g_box[:n_rows] = c["outw"].double() * c["inw"].double() * torch.sign(bd32).double() * (float(gl[3]) * rows_mean)
    b_box = bound_rcnn_box_grad(g_box)

    dims = c["dims"]
    grads = dict(rpn_cls=_scatter_scores(g_cls2, dims), rpn_box=g_rbox, cls=g_cls, box=g_box)
    b_grads = dict(rpn_cls=_scatter_scores(b_cls2, dims), rpn_box=b_rbox, cls=b_cls, box=b_box)
    beyond = torch.zeros_like(g_rbox, dtype=torch.bool)
    beyond[nbi:] = True
    off_rows = torch.ones((rows_total,), dtype=torch.bool, device=dev)
    off_rows[:n_rows] = ~live
    past = torch.zeros((rows_total, 1), dtype=torch.bool, device=dev)
    past[n_rows:] = True
    zero = dict(rpn_cls=_scatter_scores((~on).unsqueeze(1).expand(-1, 2).contiguous(), dims) | (float(gl[0]) == 0),
                rpn_box=beyond | (float(gl[1]) == 0),
                cls=off_rows.unsqueeze(1).expand(-1, K) | (float(gl[2]) == 0),
                box=past.expand(-1, 4 * K) | (float(gl[3]) == 0))
    return dict(terms=terms, b_terms=b_terms, grads=grads, b_grads=b_grads, zero=zero, sub=sub, args=torch.cat(args),
                z1=torch.cat([ce["z1"][on], cr["z1"][live]]).float())


# ---------------------------------------------------------------- MIL: reference and bounds

def mil_bag_of_row(c):
    """int64 [R]: (int)(fl(column - offset)), the kernels' own f32 subtraction and truncation"""
    return (c["col"] - torch.tensor(c["offset"], dtype=torch.float32, device=c["col"].device)).trunc().long()


def mil_select(c, last_tie=False):
    """int64 [n_bags]: per bag the first row (last with `last_tie`) whose selected column is extremal among the rows
    with (int)(column - offset) == bag; -1 for an empty bag.  Label 1 takes sel[0], any other label sel[1]."""
    bag = mil_bag_of_row(c)
    rows = torch.full((c["n_bags"],), -1, dtype=torch.int64, device=bag.device)
    labels = c["bag_labels"].tolist()
    for b in range(c["n_bags"]):
        idx = (bag == b).nonzero().squeeze(1)
        if idx.numel() == 0:
            continue
        col, sign = SEL_COL[c["sel"][0] if labels[b] == 1 else c["sel"][1]]
        v = sign * c["logits"][idx, col]
        hit = (v == v.max()).nonzero().squeeze(1)
        rows[b] = idx[hit[-1] if last_tie else hit[0]]
    return rows


def bound_mil_bag_loss(ce, w):
    """[n_bags], bag_loss = fl(w_l t): the term's bound (bound_ce_term) times |w_l|; the product, u|w_l t|."""
    return bound_ce_term(ce) * w.abs() + SLACK * U * (w * ce["t"]).abs()


def mil_reference(c):
    """rows (exact), bag_loss [n_bags], loss, grad [R, K] in f64 with their bounds.  The gradient's scale is c = gl
    scale w_l / n_bags, formed in f32 with three roundings, then as a cross-entropy gradient (bound_ce_grad with
    scale_roundings = 3).  Rows that are no bag's selected row, bags whose class weight is 0 and a zero gl give exact
    zeros."""
    logits, K, nb = c["logits"], c["K"], c["n_bags"]
    dev = logits.device
    rows = mil_select(c)
    valid = rows >= 0
    lab = c["bag_labels"].long()
    w = c["cw"].double()[lab] * valid
    ce = ce_parts(logits[rows.clamp_min(0)], lab)
    bag_loss = w * ce["t"]
    b_bag = bound_mil_bag_loss(ce, w)
    scale = float(torch.tensor(c["scale"], dtype=torch.float32).double())
    wt = scale / nb
    loss = wt * float(bag_loss.sum())
    b_loss = bound_value(b_bag, bag_loss.abs(), wt, loss, nb)
    gl = float(c["gl"].double())
    cs = gl * scale * w / nb
    grad = torch.zeros((logits.shape[0], K), dtype=torch.float64, device=dev)
    b_grad = torch.zeros_like(grad)
    sel = rows[valid]
    grad[sel] = ce_grad(ce, cs)[valid]
    b_grad[sel] = (bound_ce_grad(ce, cs, 3) * (cs != 0).unsqueeze(1))[valid]
    live = valid & (w != 0)
    sub = subnormal_count({k: (v[live] if torch.is_tensor(v) else v) for k, v in ce.items()})
    zero = torch.ones((logits.shape[0],), dtype=torch.bool, device=dev)
    zero[rows[valid & (cs != 0)]] = False
    return dict(rows=rows, bag_loss=bag_loss, b_bag=b_bag, loss=loss, b_loss=b_loss, grad=grad, b_grad=b_grad,
                zero=zero.unsqueeze(1).expand(-1, K), sub=sub, args=ce["arg32"][live].reshape(-1),
                z1=ce["z1"][live].float())


# ---------------------------------------------------------------- comparison

def ratio(got, ref, bound):
    """worst |got - ref| / bound over all elements (0 where the error is 0, inf where a bound of 0 is missed or the
    value is not finite)"""
    got = got.double() if torch.is_tensor(got) else torch.tensor(float(got), dtype=torch.float64)
    ref = ref.double() if torch.is_tensor(ref) else torch.tensor(float(ref), dtype=torch.float64, device=got.device)
    err = (got - ref).abs()
    if not torch.is_tensor(bound):
        bound = torch.full_like(err, float(bound))
    if err.numel() == 0:
        return 0.0
    r = err / bound.clamp_min(1e-300)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    r = torch.where((err > 0) & (bound <= 0), torch.full_like(r, float("inf")), r)
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def check_ratios(case, ratios, log=None):
    """prints and asserts every worst |error| / bound of one case; log keeps the worst per output"""
    for name, r in ratios.items():
        print("loss-ratio %s %.4g %s" % (name, r, case))
        if log is not None:
            log[name] = max(log.get(name, 0.0), r)
    for name, r in ratios.items():
        assert r <= 1.0, "%s: %s misses its bound, worst |error| / bound = %.4g" % (case, name, r)


def mt_ratios(ref, terms, grads):
    """worst |error| / bound of the four values (a NaN reference term must be NaN: ratio 0 then, inf otherwise) and the
    four gradient tensors"""
    r = {}
    for i, name in enumerate(("rpn_ce", "rpn_box", "ce", "box")):
        if math.isnan(ref["terms"][i]):
            r["v_" + name] = 0.0 if math.isnan(float(terms[i])) else float("inf")
        else:
            r["v_" + name] = ratio(terms[i], ref["terms"][i], ref["b_terms"][i])
    for k in ("rpn_cls", "rpn_box", "cls", "box"):
        r["g_" + k] = ratio(grads[k], ref["grads"][k], ref["b_grads"][k])
    return r


def mt_zero_violations(ref, grads):
    """per gradient tensor, the number of elements that must be exactly 0 and are not"""
    return {k: int((grads[k][ref["zero"][k].expand_as(grads[k])] != 0).sum()) for k in ref["zero"]}


def mil_ratios(ref, loss, bag_loss, grad):
    return dict(mil_loss=ratio(loss, ref["loss"], ref["b_loss"]), mil_bag_loss=ratio(bag_loss, ref["bag_loss"], ref["b_bag"]),
                mil_grad=ratio(grad, ref["grad"], ref["b_grad"]))


# ---------------------------------------------------------------- cases

def make_logits(g, n, K, lab, regime):
    """[n, K] f32 scores for labels lab [n]:
      normal     N(0, 2)
      correct    the label's logit 12 to 30 above the rest
      wrong      another class's logit 12 to 30 above the rest
      tie2       two equal maxima (both classes when K = 2); tieK: all K equal
      shiftP     the N(0, 2) scores plus 2^P, rounded to f32 as any input is
      underflow  every logit but one 91 to 109 below that one"""
    s = torch.randn((n, K), generator=g) * 2.0
    r = torch.arange(n)
    gap = 12.0 + 18.0 * torch.rand((n,), generator=g)
    other = (lab + 1 + torch.randint(0, max(K - 1, 1), (n,), generator=g)) % K
    if regime == "correct":
        s[r, lab] = s.max(1).values + gap
    elif regime == "wrong":
        s[r, other] = s.max(1).values + gap
    elif regime == "tie2":
        top = s.max(1).values + 1.0
        s[r, lab] = top
        s[r, other] = top
    elif regime == "tieK":
        s = s[:, :1].expand(n, K).clone()
    elif regime.startswith("shift"):
        s = s + 2.0 ** int(regime[5:])
    elif regime == "underflow":
        top = s[:, 0].clone()
        s = top.unsqueeze(1) - (91.0 + 18.0 * torch.rand((n, K), generator=g))
        s[r, torch.where(torch.rand((n,), generator=g) < 0.5, lab, other)] = top
    else:
        assert regime == "normal", regime
    return s.float().contiguous()


# pred, tg, in_w of the box elements every case carries: d = +-1 exactly, one ulp on either side of +-1, 0, and
# |d| >= 1 under in_w = 0 with out_w > 0 (the formula as written gives a non-zero term there)
_BOX_SPECIALS = [(1.5, 0.5, 0.5), (0.5, 1.5, 1.0), (1.5 + 2.0 ** -23, 0.5, 1.0), (1.5 - 2.0 ** -23, 0.5, 0.5),
                 (0.5, 1.5 + 2.0 ** -23, 0.5), (0.5, 1.5 - 2.0 ** -23, 1.0), (0.25, 0.25, 1.0), (3.0, 0.5, 0.0),
                 (-2.0, 0.5, 0.0), (1.5, 0.5, 0.0)]

# name: ((N, H, W, A, n_box_images), (n_rows, rows_total), K, regime)
MT_CASES = {
    "one_anchor": ((1, 1, 1, 1, 1), (1, 1), 2, "normal"),                # one anchor, four box elements
    "full_blocks": ((1, 16, 16, 8, 1), (256, 256), 32, "normal"),        # exactly 2048 anchors, 8192 box elements
    "below_block": ((1, 7, 13, 9, 1), (255, 255), 3, "correct"),         # 819 anchors, A no power of two
    "partial_nb1": ((2, 19, 23, 9, 1), (257, 300), 3, "wrong"),          # partial last blocks, box fwd < box bwd
    "partial_nb2": ((3, 19, 23, 9, 2), (300, 700), 32, "wrong"),
    "no_rows": ((1, 7, 13, 9, 1), (0, 0), 3, "normal"),
    "no_rows_pad": ((1, 7, 13, 9, 1), (0, 5), 3, "normal"),
    "tie2": ((1, 7, 13, 9, 1), (257, 300), 3, "tie2"),
    "tieK": ((1, 7, 13, 9, 1), (255, 255), 32, "tieK"),
    "correct_k2": ((1, 7, 13, 9, 1), (256, 256), 2, "correct"),
    "normal_k3": ((2, 19, 23, 9, 1), (300, 700), 3, "normal"),
    "shift5": ((2, 19, 23, 9, 1), (257, 300), 3, "shift5"),
    "shift10": ((1, 7, 13, 9, 1), (300, 700), 32, "shift10"),
    "shift12": ((1, 7, 13, 9, 1), (256, 256), 2, "shift12"),
    "underflow": ((1, 7, 13, 9, 1), (300, 700), 3, "underflow"),
    "wrong_k2": ((1, 7, 13, 9, 1), (1, 1), 2, "wrong"),
    "shift12_k3": ((1, 16, 16, 8, 1), (255, 255), 3, "shift12"),
}
GL_BASE = [0.7, -1.3, 2.0, 0.4]


def _not_pow2(n):
    return n + 1 if n > 1 and (n & (n - 1)) == 0 else n


def make_mt_case(name, device="cpu"):
    """One multi-task case (fixed seed by name).  Anchor labels -1 / 0 / 1 with about 45 % labelled, in every image
    (those beyond n_box_images carry live box weights too: the op must zero their box gradient itself); in_w in {0,
    0.5, 1}, out_w = 1 / n_examples (no power of two); the box specials on the first labelled elements; row labels in
    [0, K) with label -1 padding rows inside n_rows when n_rows > 256; gl unequal with one negative and one zero entry
    (which one rotates with the case)."""
    (N, H, W, A, nbi), (n_rows, rows_total), K, regime = MT_CASES[name]
    idx = list(MT_CASES).index(name)
    g = torch.Generator().manual_seed(5000 + idx)
    n_anchor = N * H * W * A
    pick = torch.rand((n_anchor,), generator=g)
    lab = torch.where(pick < 0.55, -1, torch.where(pick < 0.85, 0, 1))
    lab[0] = 1
    s2 = make_logits(g, n_anchor, 2, lab.clamp_min(0), regime)
    rpn_cls = _scatter_scores(s2, (N, H, W, A, nbi)).contiguous()
    rpn_labels = lab.view(N, H, W, A).permute(0, 3, 1, 2).reshape(N, 1, A * H, W).to(torch.int32).contiguous()
    n_ex = _not_pow2(int((lab >= 0).sum()))
    lab4 = lab.repeat_interleave(4)                              # element = anchor * 4 + j (channel a*4 + j)
    n_el = lab4.numel()
    pred = torch.randn((n_el,), generator=g) * 0.7
    tg = torch.randn((n_el,), generator=g) * 0.7
    half = torch.rand((n_el,), generator=g) < 0.5
    iw = torch.where(lab4 == 1, torch.where(half, 0.5, 1.0), 0.0)
    ow = torch.where(lab4 >= 0, 1.0 / n_ex, 0.0)
    far = (lab4 == 1) & (torch.rand((n_el,), generator=g) < 0.3)
    tg = tg + far * torch.where(half, 3.0, -2.5)
    spots = (lab4 >= 0).nonzero().squeeze(1)[:len(_BOX_SPECIALS)]
    for e, (p_, t_, w_) in zip(spots.tolist(), _BOX_SPECIALS):
        pred[e], tg[e], iw[e] = p_, t_, w_
    nchw = lambda t: t.float().view(N, H, W, 4 * A).permute(0, 3, 1, 2).contiguous()
    c = dict(name=name, dims=(N, H, W, A, nbi), n_rows=n_rows, rows_total=rows_total, K=K, regime=regime,
             rpn_cls=rpn_cls, rpn_labels=rpn_labels, rpn_box=pred.float().view(N, H, W, 4 * A).contiguous(),
             rpn_tg=nchw(tg), rpn_inw=nchw(iw), rpn_outw=nchw(ow))

    labr = torch.randint(0, K, (rows_total,), generator=g)
    c["cls"] = make_logits(g, rows_total, K, labr, regime)
    labr = labr[:n_rows].clone()
    if n_rows > ROW_BLOCK:
        labr[-(n_rows // 10):] = -1
    c["box"] = (torch.randn((rows_total, 4 * K), generator=g) * 0.5).float()
    rtg = torch.randn((n_rows, 4 * K), generator=g) * 0.5
    rhalf = torch.rand((n_rows, 4 * K), generator=g) < 0.5
    cols = torch.arange(4 * K).unsqueeze(0) // 4
    fg = (cols == labr.unsqueeze(1)) & (labr.unsqueeze(1) > 0)
    rinw = torch.where(fg, torch.where(rhalf, 0.5, 1.0), 0.0)
    routw = fg * (1.0 / 3.0)
    rtg = rtg + (fg & rhalf) * 2.0
    spots = fg.reshape(-1).nonzero().squeeze(1)[:3]
    for e, dd in zip(spots.tolist(), (0.0, 1.0, -1.0)):             # sgn(0) = 0; |d| = 1 exactly
        rtg.view(-1)[e] = 0.5
        c["box"][:n_rows].view(-1)[e] = 0.5 + dd
    c.update(labels=labr.to(torch.int32).view(n_rows, 1), tg=rtg.float().contiguous(), inw=rinw.float().contiguous(),
             outw=routw.float().contiguous())
    gl = list(GL_BASE)
    gl[idx % 4] = 0.0
    c["gl"] = torch.tensor(gl, dtype=torch.float32)
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}


_SIZES = [700, 0, 2, 255, 257, 1, 256]
# name: (K, n_bags, selector pair (label 1, other), bag_offset (4: strided column 0 of an [R, 5] blob), regime)
MIL_CASES = {
    "one_bag": (3, 1, (0, 0), 0.0, "normal"),
    "five_alt": (3, 5, (2, 0), 4.0, "normal"),
    "five_k8": (8, 5, (0, 0), 0.0, "wrong"),
    "bags65": (8, 65, (0, 0), 4.0, "correct"),           # one more than a block of the bag-term kernel
    "bags130": (3, 130, (2, 0), 0.0, "normal"),          # three blocks of it
    "tie2": (3, 5, (2, 0), 0.0, "tie2"),
    "tieK": (8, 5, (0, 0), 4.0, "tieK"),
    "shift5": (3, 5, (0, 0), 4.0, "shift5"),
    "shift10": (8, 5, (2, 0), 0.0, "shift10"),
    "shift12": (3, 5, (2, 0), 4.0, "shift12"),
    "underflow": (3, 5, (0, 0), 0.0, "underflow"),
}
MIL_PCT = 0.2209


def make_mil_case(name, device="cpu"):
    """One MIL case.  Bag sizes cycle through 700, 0, 2, 255, 257, 1, 256 (a lone bag holds 1 row); bag labels
    alternate 1, 2; class weights [0, p, 1 - p] (0.5 for the classes beyond); the bag column holds the bag index plus
    the offset, with rows of no bag in front (negative after the offset) and behind (>= n_bags), their logits made to
    win every selection they are wrongly let into.  Every bag of two or more rows holds a tie of its selected column
    at the extremum (the extremal row, moved and copied), rotating through: rows r, r+1; rows r, r+256 (one
    thread's); rows r, r+128 (the two halves of the shared-memory reduction); all rows equal (also where the bag is
    too short for the distance)."""
    K, nb, sel, offset, regime = MIL_CASES[name]
    idx = list(MIL_CASES).index(name)
    g = torch.Generator().manual_seed(7000 + idx)
    sizes = [1] if nb == 1 else [_SIZES[b % len(_SIZES)] for b in range(nb)]
    bag_labels = torch.tensor([1 + (b % 2) for b in range(nb)], dtype=torch.int32)
    front, back = 3, 4
    bag = torch.cat([torch.full((front,), -2.0), torch.repeat_interleave(torch.arange(nb), torch.tensor(sizes)).float(),
                     torch.full((back,), nb + 3.0)])
    R = bag.numel()
    row_lab = torch.cat([torch.ones(front, dtype=torch.int64), torch.repeat_interleave(bag_labels.long(), torch.tensor(sizes)),
                         torch.ones(back, dtype=torch.int64)])
    logits = make_logits(g, R, K, row_lab, regime)
    start, kind, ties = front, idx, []
    for b, n in enumerate(sizes):
        col, sign = SEL_COL[sel[0] if int(bag_labels[b]) == 1 else sel[1]]
        if n >= 2:
            blk = logits[start:start + n]
            want = [1, 256, 128, 0][kind % 4]
            kind += 1
            if want == 0 or want >= n:
                want = 0
                blk[:] = blk[0].clone()                             # all rows equal
            else:                                                   # whole rows move: the regime of every row stays
                orig = int((sign * blk[:, col]).argmax())
                r0 = int(torch.randint(0, n - want, (1,), generator=g))
                keep = blk[r0].clone()
                blk[r0] = blk[orig]
                blk[orig] = keep
                blk[r0 + want] = blk[r0]
            ties.append((b, want))
        start += n
    for junk in (slice(0, front), slice(R - back, R)):
        logits[junk, 0] = logits[:, 0].min() - 5.0
        logits[junk, 2] = logits[:, 2].max() + 5.0
    if offset:
        blob = torch.zeros((R, 5))
        blob[:, 0] = bag + offset
        blob[:, 1:] = torch.randn((R, 4), generator=g)
        col_t = blob.to(device)[:, 0]
    else:
        col_t = bag.to(device)
    cw = torch.full((K,), 0.5)
    cw[0], cw[1], cw[2] = 0.0, MIL_PCT, 1.0 - MIL_PCT
    c = dict(name=name, K=K, n_bags=nb, sel=sel, offset=offset, regime=regime, sizes=sizes, ties=ties,
             logits=logits.to(device),
             col=col_t, bag_labels=bag_labels.to(device), cw=cw.float().to(device), scale=0.5 + 0.01 * idx,
             gl=torch.tensor(-1.7 if idx % 2 else 0.6, dtype=torch.float32, device=device))
    return c


# ---------------------------------------------------------------- kernel models (torch f32 on the CPU)

DEFECTS = ["lse_sum", "log_of_sum", "p_minus_1", "all_anchor_count", "box_images", "drop_tail", "le_threshold",
           "iw_once", "last_tie", "bag_mean_nonempty"]


def _seq_sum(x, skip=None):
    """f32 sum over the columns in index order, as the kernels' loops add; skipped columns add an exact 0"""
    acc = torch.zeros((x.shape[0],), dtype=torch.float32, device=x.device)
    for k in range(x.shape[1]):
        acc = acc + (x[:, k] if skip is None else torch.where(skip[:, k], torch.zeros_like(acc), x[:, k]))
    return acc


def _f32(v):
    return torch.tensor(v, dtype=torch.float64).float()


def model_ce(s, lab, defects=()):
    """lse_minus_max and the two uses of it in f32: -> (t [n], p [n, K], others [n]), torch's exp / log1p standing in
    for the device's.  Defects: log_of_sum (forward through logf(1 + z)), lse_sum (probabilities through m + lz)."""
    m, first = _first_max(s)
    a = s - m
    z1 = _seq_sum(torch.exp(a), first)
    lz = torch.log(1.0 + z1) if "log_of_sum" in defects else torch.log1p(z1)
    onehot = torch.zeros_like(first).scatter_(1, lab.view(-1, 1), True)
    sl = s.gather(1, lab.view(-1, 1)).squeeze(1)
    t = (m.squeeze(1) - sl) + lz
    lzb = torch.log1p(z1)
    p = torch.exp(s - (m + lzb.unsqueeze(1))) if "lse_sum" in defects else torch.exp(a - lzb.unsqueeze(1))
    return t, p, _seq_sum(p, onehot), onehot


def _model_ce_grad(p, others, onehot, scale32, defects):
    """g_k = p_k scale, g_l = -(others) scale (p_minus_1: (p_l - 1) scale); scale32 an f32 scalar or [n] tensor"""
    sc = scale32.reshape(-1, 1) if scale32.dim() else scale32
    lab_part = ((p - 1.0) * sc) if "p_minus_1" in defects else ((-others).unsqueeze(1) * sc)
    return torch.where(onehot, lab_part, p * sc)


def _tail_mask(n, defects):
    """bool [n]: the elements a 2048-per-workgroup loop takes (drop_tail: not those of a last partial workgroup)"""
    keep = torch.ones((n,), dtype=torch.bool)
    if "drop_tail" in defects and n % BLOCK_ELEMS:
        keep[n - n % BLOCK_ELEMS:] = False
    return keep


def model_mt(c, defects=()):
    """loss.hip's arithmetic: f32 per element, f64 sums, the values rounded once.  -> (terms [4] f32, grads dict f32)"""
    N, H, W, A, nbi = c["dims"]
    n_rows, rows_total, K = c["n_rows"], c["rows_total"], c["K"]
    gl = c["gl"].double()
    s2, lab, (tg, iw, ow) = rpn_views(c)
    keep = _tail_mask(lab.numel(), defects)
    on = (lab >= 0) & keep
    t, p, others, onehot = model_ce(s2.contiguous(), ((lab != 0) & (lab >= 0)).long(), defects)
    cnt = float(lab.numel()) if "all_anchor_count" in defects else float(on.sum())
    terms = [(t.double() * on).sum() / cnt if cnt else torch.tensor(float("nan"), dtype=torch.float64)]
    sc0 = _f32(float(gl[0]) / cnt) if cnt else _f32(0.0)
    g2 = _model_ce_grad(p, others, onehot, sc0, defects) * on.unsqueeze(1)

    pred = c["rpn_box"]
    d = pred - tg
    thr = (d.abs() <= 1.0) if "le_threshold" in defects else (d.abs() < 1.0)
    q = (iw * d) * 3.0
    per = torch.where(thr, (0.5 * q) * q, d.abs() - _f32(0.5 / 9.0))
    el = (ow * per).double()
    el_live = el[:nbi].reshape(-1) * _tail_mask(el[:nbi].numel(), defects)
    terms.append(10.0 * el_live.sum() / (nbi * 4.0 * A))
    sc1 = _f32(10.0 * float(gl[1]) / (nbi * 4.0 * A))
    x9 = ((9.0 * iw) * d) if "iw_once" in defects else (((9.0 * iw) * iw) * d)
    gb = (ow * torch.where(thr, x9, torch.sign(d))) * sc1
    live_images = min(nbi + 1, N) if "box_images" in defects else nbi
    gb[live_images:] = 0.0
    gb = (gb.reshape(-1) * _tail_mask(gb.numel(), defects)).view_as(pred)

    labr = c["labels"].reshape(-1).long()
    live = (labr >= 0) & (labr < K)
    rc = float(live.sum())
    tr, pr, oth, oh = model_ce(c["cls"][:n_rows].contiguous(), labr.clamp(0, K - 1), defects)
    terms.append((tr.double() * live).sum() / rc if rc else torch.tensor(float("nan"), dtype=torch.float64))
    sc2 = _f32(float(gl[2]) / rc) if rc else _f32(0.0)
    g_cls = torch.zeros((rows_total, K))
    g_cls[:n_rows] = _model_ce_grad(pr, oth, oh, sc2, defects) * live.unsqueeze(1)
    bd = c["box"][:n_rows] - c["tg"]
    row = _seq_sum(c["outw"] * (c["inw"] * bd.abs()))
    terms.append(row.double().sum() / max(rc, 1.0))
    sc3 = _f32(float(gl[3]) / max(rc, 1.0))
    g_box = torch.zeros((rows_total, 4 * K))
    g_box[:n_rows] = ((c["outw"] * c["inw"]) * torch.sign(bd)) * sc3
    return (torch.stack([x.double() for x in terms]).float(),
            dict(rpn_cls=_scatter_scores(g2, c["dims"]), rpn_box=gb, cls=g_cls, box=g_box))


def model_mil(c, defects=()):
    """mil.hip's arithmetic -> (rows, bag_loss f32, loss f32, grad f32)"""
    logits, K, nb = c["logits"], c["K"], c["n_bags"]
    rows = mil_select(c, last_tie="last_tie" in defects)
    valid = rows >= 0
    lab = c["bag_labels"].long()
    w = c["cw"][lab] * valid
    t, p, others, onehot = model_ce(logits[rows.clamp_min(0)].contiguous(), lab, defects)
    bag_loss = torch.where(valid, w * t, torch.zeros_like(t))
    n = float(valid.sum()) if "bag_mean_nonempty" in defects else float(nb)
    scale = _f32(c["scale"])
    loss = (scale.double() * bag_loss.double().sum() / n).float()
    cs = ((c["gl"] * scale) * w) / _f32(n)
    g = _model_ce_grad(p, others, onehot, cs, defects)
    grad = torch.zeros((logits.shape[0], K))
    grad[rows[valid]] = g[valid]
    return rows, bag_loss, loss, grad
