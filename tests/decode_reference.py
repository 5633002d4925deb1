"""Shared by test_val_detect_cpu.py and test_gpu_val_detect.py: the arithmetic of wssdl_decode_detections
(include/wssdl_bus_hip.h) restated in NumPy, an f64 evaluation of the same formulas with a bound counted from the
statement's roundings, the guard under which two faithful f64 exp implementations round to the same f32, and the
seeded cases.  NumPy only, no import of the package.

The statement: every operation in np.float32 (NumPy rounds each elementwise f32 operation on its own; its f32 division
is IEEE), the exponential as np.float32(np.exp(np.float64(d))).  A row whose batch index, truncated to an integer, is
outside [0, n_images) is a dead row of zeros."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24                     # unit roundoff of f32: |fl(x) - x| <= U |x|


def live_rows(rois, n_images):
    """(live [R] bool, image [R] int; 0 where dead): (int)rois[r, 0] in [0, n_images), NaN dead"""
    b = np.asarray(rois, F32)[:, 0].astype(np.float64)
    live = (b > -1.0) & (b < float(n_images))
    return live, np.where(live, np.trunc(np.where(live, b, 0.0)), 0).astype(np.int64)


def clip_bounds(im_info, n_images, bounds=None):
    """[n_images, 2] f32 (xmax, ymax): `bounds` as given, or (float)((double)w / (double)s - 1.0) and the same of h"""
    info = np.asarray(im_info, F32)[:n_images]
    if bounds is not None:
        return np.asarray(bounds, F32).reshape(n_images, 2)
    s = info[:, 2].astype(np.float64)
    return np.stack((info[:, 1].astype(np.float64) / s - 1.0, info[:, 0].astype(np.float64) / s - 1.0), 1).astype(F32)


def statement(rois, deltas, im_info, n_images, bounds=None):
    """boxes [R, 4K] f32: the f32 statement, operation by operation"""
    rois, deltas, info = np.asarray(rois, F32), np.asarray(deltas, F32), np.asarray(im_info, F32)
    R, K = deltas.shape[0], deltas.shape[1] // 4
    live, img = live_rows(rois, n_images)
    lim = clip_bounds(info, n_images, bounds)[img]                     # [R, 2]
    s = info[img, 2][:, None]                                          # [R, 1] f32
    with np.errstate(all="ignore"):
        b = rois[:, 1:5] / s                                           # IEEE f32 division
        half, one = F32(0.5), F32(1.0)
        w = ((b[:, 2] - b[:, 0]) + one)[:, None]
        h = ((b[:, 3] - b[:, 1]) + one)[:, None]
        cx = b[:, 0:1] + half * w
        cy = b[:, 1:2] + half * h
        d = deltas.reshape(R, K, 4)
        pcx = d[:, :, 0] * w
        pcx = pcx + cx
        pcy = d[:, :, 1] * h
        pcy = pcy + cy
        pw = np.exp(d[:, :, 2].astype(np.float64)).astype(F32) * w
        ph = np.exp(d[:, :, 3].astype(np.float64)).astype(F32) * h
        hpw, hph = half * pw, half * ph
        xm, ym, zero = lim[:, 0:1], lim[:, 1:2], F32(0.0)
        out = np.stack((np.maximum(np.minimum(pcx - hpw, xm), zero), np.maximum(np.minimum(pcy - hph, ym), zero),
                        np.maximum(np.minimum(pcx + hpw, xm), zero), np.maximum(np.minimum(pcy + hph, ym), zero)), axis=2)
    assert out.dtype == F32 and all(a.dtype == F32 for a in (b, w, cx, pcx, pw, hpw))
    out[~live] = 0.0
    return out.reshape(R, 4 * K)


def evaluate_f64(rois, deltas, im_info, n_images, bounds=None):
    """(boxes [R, 4K] f64, bound [R, 4K] f64): the same formulas on the same f32 inputs evaluated in f64 (clipped to
    the same f32 bounds), and the elementwise bound on |statement - f64| counted from the statement's roundings.

    Each f32 operation contributes U times the magnitude of its result; errors already carried by its operands pass
    through an addition unchanged and through a multiplication scaled by the other factor.  With eb = U |b| for the
    division:
        w  = (b2 - b1) + 1        ew  = eb1 + eb2 + U |b2 - b1| + U |w|
        cx = b1 + 0.5 w           ecx = eb1 + 0.5 ew + U |cx|                    (0.5 * w is exact)
        pcx = d.x * w + cx        epc = |d.x| ew + U |d.x w| + ecx + U |pcx|
        pw = fl32(exp(d.z)) * w   epw = E ew + U E |w| + U |pw|                  (E = exp(d.z); fl32: one rounding;
                                                                                 the f64 exp itself adds < 2^-52)
        x  = pcx -+ 0.5 pw        ex  = epc + 0.5 epw + U |x|
    The clip is monotone and 1-Lipschitz, so it adds nothing.  The magnitudes are taken from the f64 evaluation; what
    that neglects is second order in U (relative 2^-24 of the bound), covered by the factor 1.001."""
    rois, deltas, info = np.asarray(rois, F32), np.asarray(deltas, F32), np.asarray(im_info, F32)
    R, K = deltas.shape[0], deltas.shape[1] // 4
    live, img = live_rows(rois, n_images)
    lim = clip_bounds(info, n_images, bounds)[img].astype(np.float64)
    s = info[img, 2].astype(np.float64)[:, None]
    b = rois[:, 1:5].astype(np.float64) / s
    eb = U * np.abs(b)
    d = deltas.reshape(R, K, 4).astype(np.float64)
    out, bound = np.zeros((R, K, 4)), np.zeros((R, K, 4))
    for a in (0, 1):                                                   # x, then y
        b1, b2, e1, e2 = b[:, a:a + 1], b[:, a + 2:a + 3], eb[:, a:a + 1], eb[:, a + 2:a + 3]
        w = (b2 - b1) + 1.0
        ew = e1 + e2 + U * np.abs(b2 - b1) + U * np.abs(w)
        c = b1 + 0.5 * w
        ec = e1 + 0.5 * ew + U * np.abs(c)
        dx, E = d[:, :, a], np.exp(d[:, :, a + 2])
        pc = dx * w + c
        epc = np.abs(dx) * ew + U * np.abs(dx * w) + ec + U * np.abs(pc)
        pw = E * w
        epw = E * ew + U * E * np.abs(w) + U * np.abs(pw)
        for col, sign in ((a, -1.0), (a + 2, 1.0)):
            x = pc + sign * 0.5 * pw
            out[:, :, col] = np.maximum(np.minimum(x, lim[:, a:a + 1]), 0.0)
            bound[:, :, col] = 1.001 * (epc + 0.5 * epw + U * np.abs(x))
    out[~live] = 0.0
    bound[~live] = 0.0
    return out.reshape(R, 4 * K), bound.reshape(R, 4 * K)


def exp_value_is_safe(e):
    """the rule of exp_is_safe on the f64 value e itself"""
    e = np.asarray(e, np.float64)
    f = e.astype(F32)
    up = (f.astype(np.float64) + np.nextafter(f, F32(np.inf)).astype(np.float64)) / 2.0       # exact in f64
    down = (f.astype(np.float64) + np.nextafter(f, F32(-np.inf)).astype(np.float64)) / 2.0
    margin = 4.0 * np.spacing(e)
    return (np.abs(e - up) > margin) & (np.abs(e - down) > margin)


def exp_is_safe(d):
    """True where the f64 value of exp(d) lies more than 4 f64 ulps from every midpoint between adjacent f32 values:
    two faithful f64 exp implementations (each within 1 ulp of the true value, so within 2 of each other) then round
    to the same f32."""
    return exp_value_is_safe(np.exp(np.asarray(d, F32).astype(np.float64)))


def exp_arguments(case):
    """the dw, dh columns of the case's live rows: every argument the exponential sees"""
    live, _ = live_rows(case["rois"], case["n_images"])
    d = case["deltas"].reshape(case["deltas"].shape[0], -1, 4)
    return d[live][:, :, 2:4].ravel()


# ------------------------------------------------------------------------------------------------ the cases ---

def _softmax(x):
    e = np.exp(x - x.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(F32)


def _rows(rs, image, n, h, w, K):
    """n rows of one image: boxes in the scaled image's pixels that start left of / above it (negative coordinates)
    and reach past its right and lower edge; dx, dy ~ N(0, 0.5), dw, dh uniform in [-4, 4]"""
    x1 = rs.uniform(-30.0, w - 20.0, n)
    y1 = rs.uniform(-30.0, h - 20.0, n)
    rois = np.stack((np.full(n, float(image)), x1, y1, x1 + rs.uniform(8.0, 0.6 * w, n), y1 + rs.uniform(8.0, 0.6 * h, n)), 1)
    d = np.empty((n, K, 4))
    d[:, :, 0:2] = rs.normal(0.0, 0.5, (n, K, 2))
    d[:, :, 2:4] = rs.uniform(-4.0, 4.0, (n, K, 2))
    return rois.astype(F32), d.reshape(n, 4 * K).astype(F32)


def _case(name, rois, deltas, im_info, shapes, rs):
    n, K = len(im_info), deltas.shape[1] // 4
    info = np.asarray(im_info, F32)
    live, img = live_rows(rois, n)
    first = {i: int(np.nonzero(live & (img == i))[0].min()) for i in set(img[live].tolist())}
    last = {i: int(np.nonzero(live & (img == i))[0].max()) for i in first}
    return dict(name=name, rois=rois, deltas=deltas, im_info=info, n_images=n, K=K, im_shapes=shapes,
                bounds=np.array([(wd - 1.0, ht - 1.0) for ht, wd in shapes], F32),
                scores=_softmax(rs.normal(0.0, 1.5, (rois.shape[0], K))),
                span=max([last[i] - first[i] + 1 for i in first] + [1]))        # longest run of one image in the blob


def mixed(seed=7101):
    """N = 3 (scales 1.0, 0.6, 1.7777778), K = 3, rows per image 0, 1 and 130, images in ascending order; dead rows
    (batch index -1 and N, with ordinary coordinates and deltas) before, between and inside the images' runs and at
    the end: R = 143, no multiple of 64; image 2's run spans 139 rows."""
    rs = np.random.RandomState(seed)
    K, N = 3, 3
    info = [(300.0, 500.0, 1.0, 1.0), (360.0, 480.0, 0.6, 2.0), (640.0, 1138.0, 1.7777778, 0.0)]
    shapes = [(300, 500), (600, 800), (360, 640)]                      # the original (H, W)
    dead = lambda i: _rows(rs, i, 1, 300.0, 500.0, K)                  # noqa: E731
    parts = [dead(-1), _rows(rs, 1, 1, info[1][0], info[1][1], K), dead(N)]
    r2, d2 = _rows(rs, 2, 130, info[2][0], info[2][1], K)
    for k in range(0, 130, 13):
        parts.append((r2[k:k + 13], d2[k:k + 13]))
        parts.append(dead(-1 if (k // 13) % 2 else N))
    rois = np.concatenate([p[0] for p in parts], 0)
    deltas = np.concatenate([p[1] for p in parts], 0)
    c = _case("mixed", rois, deltas, info, shapes, rs)
    assert rois.shape[0] % 64 != 0 and c["span"] == 139
    return c


def one_row(seed=7102):
    """R = 1, N = 1, K = 2"""
    rs = np.random.RandomState(seed)
    r, d = _rows(rs, 0, 1, 320.0, 480.0, 2)
    return _case("one_row", r, d, [(320.0, 480.0, 0.8, 1.0)], [(400, 600)], rs)


def wide(seed=7103):
    """R = 70, K = 21, two images (35 rows each, scales 1.25 and 0.5)"""
    rs = np.random.RandomState(seed)
    info = [(500.0, 625.0, 1.25, 1.0), (250.0, 300.0, 0.5, 2.0)]
    parts = [_rows(rs, i, 35, info[i][0], info[i][1], 21) for i in (0, 1)]
    return _case("wide", np.concatenate([p[0] for p in parts], 0), np.concatenate([p[1] for p in parts], 0), info,
                 [(400, 500), (500, 600)], rs)


BUILDERS = {"mixed": mixed, "one_row": one_row, "wide": wide}
_built = {}


def case(name):
    """the case, built once and shared (nobody writes into it)"""
    if name not in _built:
        c = BUILDERS[name]()
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _built[name] = c
    return _built[name]


# (case, bounds given?) pairs every test runs: mixed both ways, the others with the reference's bounds
RUNS = [("mixed", True), ("mixed", False), ("one_row", True), ("wide", True)]
