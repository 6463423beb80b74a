"""Float64 numpy restatements of the texture evaluator, written from the reference's text and taking nothing from the code under test:
no import of oracle_lib or of the package, no read of the two shared tables.  Every evaluator returns

    value, bound

where `bound` limits how far a correct float32 evaluation of the same formula (the reference computes in f32) may lie from the float64
value, and is +inf where the evaluation sits within its own error of a discontinuity (such evaluations are *left out* by the tests, and
their share is capped).  The bound is derived per evaluation:

  smooth parts   a count of float32 roundings x 2^-24 x the magnitude of the terms, with the conditioning of the cancelling ones
                 (A*C - B*B/4, the three terms of r2, bump_int(s1) - bump_int(s0) over 2 ds, lambda * p, log2);
  steps          wherever a floor, a comparison or a table index decides, see each function.

One thing comes from the shared headers: noise() is handed its 256-entry permutation by the caller, and the tests read it from
include/pbrtgpu_noise_perm.h -- but accept it only with the SHA-256 of the table in the reference's noise.rs (recorded in
test_texture_oracle.py), so a wrong entry fails the digest instead of being shared by both sides, and the table is not written out a
third time.  The EWA weight table is recomputed here from the reference's recipe.

The inputs are float32 numbers on both sides; what they carry beyond that (the observable of test_gpu_texture_truth.py hands over hits
computed in float32) comes in as absolute uncertainties: `e_p`, `e_uv` on the point and its uv, `e_dp`, `e_duv` on the differentials.
The constants of the formulas are the reference's f32 literals, so 1.99 below is float(np.float32(1.99)).

Where the reference's text and the textbook differ the text wins (DESIGN.md section 2 has the numbers):
  * trilinear width is max(|dst0|, |dst1|) by components, without the textbook's factor 2   (mipmap.rs:639-646)
  * IdentityMapping3D::map returns dpdx for both differentials                              (mapping3d.rs:32-33)
  * the wrap fix of the spherical and cylindrical mappings touches component [1] only       (mapping2d.rs:78-88, 121-131)
  * `triangle` with a "black" wrap mode on either axis wraps NEITHER axis (mipmap.rs:751) and reads t * w + s as it comes: out of
    range it panics, and s1 == w with t in range reads the first texel of the next row.  Here the text does NOT win: texel()
    semantics (black outside, the other axis wrapped as it asks) are stated, as in the project -- a decision, Q48 in DESIGN.md
  * marble's first = min(1, floor(t * nseg))                                                 (marble.rs:46)
  * turbulence adds the *signed* noise of the partial octave                                 (noise.rs:142)
"""
import numpy as np

U = 2.0 ** -24
INF = np.inf
REPEAT, BLACK, CLAMP = 0, 1, 2


def c32(x):
    """An f32 literal of the reference as the float64 number it is."""
    return float(np.float32(x))


PI, INV_PI, INV_2PI = c32(np.pi), c32(1.0 / np.pi), c32(0.5 / np.pi)      # core/base/constants: f32


def _r32(x):
    """|fl32(x) - x|: the rounding a correctly rounded float32 operation commits on the exact result x."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.abs(np.asarray(x, np.float64).astype(np.float32).astype(np.float64) - x)


# ---------------------------------------------------------------------------------------------------------------- the weight table
def ewa_lut():
    """mipmap_weight_lut.rs as its build script makes it: f32 exp(-2 r2) - exp(-2), r2 = i / 127, printed with 8 decimals, parsed back."""
    import ctypes
    import ctypes.util
    expf = ctypes.CDLL(ctypes.util.find_library("m")).expf             # f32::exp is libm's expf
    expf.restype, expf.argtypes = ctypes.c_float, [ctypes.c_float]
    r2 = (np.arange(128, dtype=np.float32) / np.float32(127)).astype(np.float32)
    v = [np.float32(np.float32(expf(float(np.float32(-2.0) * r))) - np.float32(expf(-2.0))) for r in r2]
    return np.array([float("%9.8f" % float(x)) for x in v], np.float32)


LUT = ewa_lut().astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- MIPMap
def pyramid(img):
    """make_pyramid (mipmap.rs:406-441) with downsample_half (:225-253): while the level is not 1 x 1, halve the width if it is > 1
    (a * 0.5 + b * 0.5), then the height likewise.  The levels are the f32 texels the reference stores, so the halving is done in
    float32: the two products are exact and numpy rounds the sum as every IEEE float32 add does.  img: (H, W) or (H, W, C)."""
    a = np.asarray(img, np.float32)
    if a.ndim == 2:
        a = a[:, :, None]
    lv = [a]
    half = np.float32(0.5)
    while lv[-1].shape[0] * lv[-1].shape[1] != 1:
        c = lv[-1]
        if c.shape[1] > 1:
            c = (c[:, 0::2] * half + c[:, 1::2] * half).astype(np.float32)
        if c.shape[0] > 1:
            c = (c[0::2] * half + c[1::2] * half).astype(np.float32)
        lv.append(c)
    return lv


def _wrap(i, n, mode):
    """wrap_coord / texel_static (mipmap.rs:503-544): index and whether it is inside (False: the texel is black)."""
    i = np.asarray(i, np.int64)
    if mode == REPEAT:
        return i & (n - 1), np.ones(i.shape, bool)
    if mode == CLAMP:
        return np.clip(i, 0, n - 1), np.ones(i.shape, bool)
    ok = (i >= 0) & (i < n)
    return np.where(ok, i, 0), ok


def texel(lv, s, t, swrap, twrap):
    """MIPMap::texel of one level (h, w, c) at integer arrays s, t (broadcast together): float64 (..., c)."""
    h, w = lv.shape[:2]
    s, oks = _wrap(s, w, swrap)
    t, okt = _wrap(t, h, twrap)
    v = lv[t, s].astype(np.float64)
    return v * (oks & okt)[..., None]


def _vrange(levels, swrap, twrap):
    lo, hi = float(levels[0].min()), float(levels[0].max())
    if BLACK in (swrap, twrap):
        lo, hi = min(lo, 0.0), max(hi, 0.0)
    return hi - lo, max(abs(lo), abs(hi))


def triangle(lv, st, swrap, twrap, e_st=0.0):
    """MIPMap::triangle (mipmap.rs:711-765) on one level for st (n, 2).  floor(s) is a step the value is continuous across (the weight
    of the texel that changes is ~0), so only the smooth term is needed: the float32 error of s = st * w - 0.5 (st * w is exact, w is a
    power of two) and of ds, times the difference of the neighbouring texels, plus 8 roundings of the weighted sum."""
    h, w = lv.shape[:2]
    s, t = st[:, 0] * w - 0.5, st[:, 1] * h - 0.5
    s0, t0 = np.floor(s), np.floor(t)
    ds, dt = (s - s0)[:, None], (t - t0)[:, None]
    s0, t0 = s0.astype(np.int64), t0.astype(np.int64)
    v00, v01 = texel(lv, s0, t0, swrap, twrap), texel(lv, s0, t0 + 1, swrap, twrap)
    v10, v11 = texel(lv, s0 + 1, t0, swrap, twrap), texel(lv, s0 + 1, t0 + 1, swrap, twrap)
    val = v00 * ((1 - ds) * (1 - dt)) + v01 * ((1 - ds) * dt) + v10 * (ds * (1 - dt)) + v11 * (ds * dt)
    es = _r32(s) + U + e_st * w
    et = _r32(t) + U + e_st * h
    dvs = np.maximum(np.abs(v10 - v00), np.abs(v11 - v01)).max(1)
    dvt = np.maximum(np.abs(v01 - v00), np.abs(v11 - v10)).max(1)
    vmax = np.max(np.abs(np.stack([v00, v01, v10, v11])), axis=(0, 2))
    return val, es * dvs + et * dvt + 8 * U * vmax


def _by_level(levels, lvl, fn, n, c):
    val, bnd = np.zeros((n, c)), np.zeros(n)
    for l in np.unique(lvl):
        m = lvl == l
        val[m], bnd[m] = fn(int(l), m)
    return val, bnd


def lookup(levels, st, width, swrap, twrap, e_st=0.0, e_w=0.0):
    """MIPMap::lookup (mipmap.rs:620-637), trilinear.  level = max_level + log2(max(width, 1e-8)).  level < 0 and floor(level) are
    steps the value is continuous across; level >= max_level switches from the bilinear read of the last level to its texel (0, 0),
    which differs under a "black" wrap: within the error of `level` of that switch the evaluation is left out."""
    n, c = len(st), levels[0].shape[2]
    nl = len(levels)
    max_level = float(nl - 1)
    e_st, e_w = np.broadcast_to(np.asarray(e_st, np.float64), (n,)), np.broadcast_to(np.asarray(e_w, np.float64), (n,))
    wd = np.maximum(width, c32(1e-8))
    lg = np.log2(wd)
    level = max_level + lg
    e_level = (U + e_w / wd) / np.log(2.0) + U * (np.abs(lg) + nl + 1)
    vr, vm = _vrange(levels, swrap, twrap)
    val, bnd = np.zeros((n, c)), np.zeros(n)
    lo, hi = level < 0, level >= max_level
    mid = ~lo & ~hi
    if lo.any():
        val[lo], bnd[lo] = triangle(levels[0], st[lo], swrap, twrap, e_st[lo])
    if hi.any():
        val[hi] = texel(levels[-1], np.zeros(int(hi.sum()), np.int64), np.zeros(int(hi.sum()), np.int64), swrap, twrap)
    if mid.any():
        il = np.floor(level).astype(np.int64)
        delta = np.clip(level - il, 0.0, 1.0)

        def pair(l, m):
            a, ba = triangle(levels[l], st[m], swrap, twrap, e_st[m])
            b, bb = triangle(levels[l + 1], st[m], swrap, twrap, e_st[m])
            d = delta[m][:, None]
            return a * (1 - d) + b * d, (1 - delta[m]) * ba + delta[m] * bb + e_level[m] * np.abs(b - a).max(1) + 3 * U * vm
        v, b = _by_level(levels, np.where(mid, il, -1), lambda l, m: pair(l, m) if l >= 0 else (0.0, 0.0), n, c)
        val[mid], bnd[mid] = v[mid], b[mid]
    near_int = np.abs(level - np.round(level)) <= e_level               # the float32 side may take the neighbouring pair of levels
    bnd = bnd + np.where(near_int, e_level * vr, 0.0)
    if BLACK in (swrap, twrap):
        bnd = np.where(np.abs(level - max_level) <= e_level, INF, bnd)
    return val, bnd


MAX_WINDOW = 60000


def _ewa_level(lv, st, d0, d1, swrap, twrap, e_st, e0, e1):
    """ewa_rgb / ewa_float = make_ewa_params + ewa_core (mipmap.rs:141-213) on one level, all evaluations at once.  e_st, e0, e1: the
    absolute uncertainty of every component of st, d0 and d1.

    Smooth terms.  st * w and d * w are exact (w, h are powers of two).  The unnormalised A, B, C are sums of two products (+ 1): 3
    roundings on their sums of magnitudes (for B that is Bm = 2 (|a0x a0y| + |a1x a1y|)), and the inputs' uncertainty to first
    order, 2 (|a0y| e0 + |a1y| e1) for A and likewise for B and C.  F = A C - B B / 4 cancels: its absolute error is
    C eA + A eC + |B| eB / 2 and 2 roundings on A C + B B / 4, and every normalised coefficient inherits it.  r2 adds the error of
    ss = is - s and tt through its gradient, and 6 roundings on the sum of its three terms' magnitudes.
    Steps.  A texel whose r2 * 128 lies within that error of an integer may take the neighbouring table entry: it contributes
    |lut[i] - lut[i +- 1]| * |v - result| / sum_wts.  Near r2 = 1, and at the ceil / floor of the ellipse's box, a texel contributes its
    own weight, which is ~0 there: the table ends in 0, and the box is the exact bound of the ellipse, so a texel the float32 box drops
    has r2 ~ 1.  The float64 window is taken one texel wider for that reason.
    The sum: (2 n + 4) roundings on the largest texel for n texels inside."""
    n, c = len(st), lv.shape[2]
    h, w = lv.shape[:2]
    sx, sy = st[:, 0] * w - 0.5, st[:, 1] * h - 0.5
    a0x, a0y, a1x, a1y = d0[:, 0] * w, d0[:, 1] * h, d1[:, 0] * w, d1[:, 1] * h
    A = a0y * a0y + a1y * a1y + 1.0
    B = -2.0 * (a0x * a0y + a1x * a1y)
    Bm = 2.0 * (np.abs(a0x * a0y) + np.abs(a1x * a1y))
    Cc = a0x * a0x + a1x * a1x + 1.0
    F = A * Cc - B * B * 0.25
    nA = 3 * U * A + 2 * h * (np.abs(a0y) * e0 + np.abs(a1y) * e1)      # absolute errors of the unnormalised coefficients
    nC = 3 * U * Cc + 2 * w * (np.abs(a0x) * e0 + np.abs(a1x) * e1)
    nB = 3 * U * Bm + 2 * (np.abs(a0x) * h * e0 + np.abs(a0y) * w * e0 + np.abs(a1x) * h * e1 + np.abs(a1y) * w * e1)
    cF = (Cc * nA + A * nC + np.abs(B) * nB * 0.5 + 2 * U * (A * Cc + B * B * 0.25)) / F + 3 * U          # relative; + 1 / F and the product with it
    A, B, Cc = A / F, B / F, Cc / F
    eA, eB, eC = nA / F + A * cF, nB / F + np.abs(B) * cF, nC / F + Cc * cF
    det = -B * B + 4 * A * Cc
    us, vs = np.sqrt(det * Cc), np.sqrt(det * A)
    s0, s1 = np.ceil(sx - 2 / det * us) - 1, np.floor(sx + 2 / det * us) + 1
    t0, t1 = np.ceil(sy - 2 / det * vs) - 1, np.floor(sy + 2 / det * vs) + 1
    ns, nt = (s1 - s0 + 1), (t1 - t0 + 1)
    es, et = _r32(sx) + e_st * w, _r32(sy) + e_st * h
    val, bnd = np.zeros((n, c)), np.full(n, INF)
    ok = np.isfinite(ns * nt) & (ns * nt <= MAX_WINDOW)
    idx = np.nonzero(ok)[0]
    idx = idx[np.argsort((ns * nt)[idx], kind="stable")]
    i = 0
    while i < len(idx):
        j = i + 1
        ms, mt = int(ns[idx[i]]), int(nt[idx[i]])
        while j < len(idx) and j - i < 512:                             # grow the chunk while its padded size stays moderate
            ms2, mt2 = max(ms, int(ns[idx[j]])), max(mt, int(nt[idx[j]]))
            if (j - i + 1) * ms2 * mt2 > 400000:
                break
            ms, mt = ms2, mt2
            j += 1
        k = idx[i:j]
        i = j
        S = s0[k, None] + np.arange(ms)[None, :]                        # (m, ms)
        T = t0[k, None] + np.arange(mt)[None, :]
        inwin = (S <= s1[k, None])[:, None, :] & (T <= t1[k, None])[:, :, None]
        ss = (S - sx[k, None])[:, None, :]
        tt = (T - sy[k, None])[:, :, None]
        a, b, cc = A[k, None, None], B[k, None, None], Cc[k, None, None]
        r2 = a * ss * ss + b * ss * tt + cc * tt * tt
        terms = a * ss * ss + np.abs(b * ss * tt) + cc * tt * tt
        e_r2 = (eA[k, None, None] * ss * ss + eB[k, None, None] * np.abs(ss * tt) + eC[k, None, None] * tt * tt + 6 * U * terms +
                (es[k, None, None] + U * np.abs(ss)) * np.abs(2 * a * ss + b * tt) + (et[k, None, None] + U * np.abs(tt)) * np.abs(b * ss + 2 * cc * tt))

        def weight(r):
            ix = np.clip(np.floor(np.maximum(r, 0.0) * 128.0), 0, 127).astype(np.int64)
            return np.where((r < 1.0) & inwin, LUT[ix], 0.0)
        wgt = weight(r2)
        dw = np.maximum(np.abs(weight(r2 - e_r2) - wgt), np.abs(weight(r2 + e_r2) - wgt))
        v = texel(lv, S.astype(np.int64)[:, None, :], T.astype(np.int64)[:, :, None], swrap, twrap)          # (m, mt, ms, c)
        sw = wgt.sum((1, 2))
        res = (v * wgt[..., None]).sum((1, 2)) / sw[:, None]
        dev = np.abs(v - res[:, None, None, :]).max(3)
        sdw = dw.sum((1, 2))
        step = (dev * dw).sum((1, 2)) / sw
        step = np.where(sdw < 0.5 * sw, step / np.maximum(1.0 - sdw / sw, 0.5), INF)
        cnt = (wgt > 0).sum((1, 2))
        vmax = np.abs(v * (wgt > 0)[..., None]).max((1, 2, 3))
        val[k], bnd[k] = res, step + (2 * cnt + 4) * U * vmax
    return val, bnd


def lookup_delta(levels, st, dst0, dst1, trilinear, max_aniso, swrap, twrap, e_st=0.0, e_d=0.0):
    """lookup_delta_rgb / lookup_delta_float (mipmap.rs:819-852, :913-946) for st, dst0, dst1 (n, 2).  e_st, e_d: absolute uncertainty
    of every component of st and of the two differentials (scalars or (n,)).

    The swap (|dst0| < |dst1|) and the clamp to max_anisotropy are steps the value is continuous across: A, B, C are symmetric in the
    two vectors, and the clamp's scale is 1 where it starts.  floor(lod) is continuous as well (t is ~0 or ~1): where lod lies within
    its error of an integer, the error of lod times the image's value range is added, because the float32 side may blend the
    neighbouring pair of levels.  `minor_length > 0` decides exactly (no test input has a length that underflows in f32)."""
    st, dst0, dst1 = (np.asarray(x, np.float64) for x in (st, dst0, dst1))
    n, c = len(st), levels[0].shape[2]
    e_st, e_d = np.broadcast_to(np.asarray(e_st, np.float64), (n,)), np.broadcast_to(np.asarray(e_d, np.float64), (n,))
    if trilinear:
        width = np.maximum(np.abs(dst0).max(1), np.abs(dst1).max(1))
        return lookup(levels, st, width, swrap, twrap, e_st, e_d)
    nl = len(levels)
    swp = (dst0 * dst0).sum(1) < (dst1 * dst1).sum(1)
    d0, d1 = np.where(swp[:, None], dst1, dst0), np.where(swp[:, None], dst0, dst1)
    major, minor = np.sqrt((d0 * d0).sum(1)), np.sqrt((d1 * d1).sum(1))
    ma = c32(max_aniso)
    with np.errstate(divide="ignore", invalid="ignore"):
        clamp = (minor * ma < major) & (minor > 0)
        scale = np.where(clamp, major / (minor * ma), 1.0)
        # the clamped minor axis is the unit vector of d1 times major / maxanisotropy (the float32 side divides by the length of the
        # same d1 it scales): its direction carries d1's relative uncertainty, its length the major axis's
        e_minor = np.where(clamp, scale * (np.sqrt(2.0) * e_d + 4 * U * minor) + np.sqrt(2.0) * e_d / ma, e_d)
        rel = np.where(minor > 0, np.sqrt(2.0) * e_d / np.where(clamp, major, minor) + np.where(clamp, 4 * U, 0.0), 0.0)       # of the final minor length
    d1 = d1 * scale[:, None]
    minor = minor * scale
    val, bnd = np.zeros((n, c)), np.zeros(n)
    z = minor <= 0
    if z.any():
        val[z], bnd[z] = lookup(levels, st[z], np.zeros(int(z.sum())), swrap, twrap, e_st[z], 0.0)
    nz = ~z
    if nz.any():
        with np.errstate(divide="ignore"):
            lg = np.log2(np.where(nz, minor, 1.0))
        lod = np.maximum(0.0, nl - 1.0 + lg)
        e_lod = (8 * U + rel) / np.log(2.0) + U * (np.abs(lg) + nl + 2)
        il = np.floor(lod).astype(np.int64)
        t = lod - il
        vr, vm = _vrange(levels, swrap, twrap)
        last = texel(levels[-1], np.zeros(1, np.int64), np.zeros(1, np.int64), swrap, twrap)[0]

        def one(l, m):
            if l >= nl:
                return np.broadcast_to(last, (int(m.sum()), c)), np.zeros(int(m.sum()))
            return _ewa_level(levels[l], st[m], d0[m], d1[m], swrap, twrap, e_st[m], e_d[m], e_minor[m])
        v0, b0 = _by_level(levels, np.where(nz, il, nl), one, n, c)
        v1, b1 = _by_level(levels, np.where(nz, il + 1, nl), one, n, c)
        v = v0 * (1 - t)[:, None] + v1 * t[:, None]
        b = (1 - t) * b0 + t * b1 + e_lod * np.abs(v1 - v0).max(1) + 4 * U * vm
        b = b + np.where(np.abs(lod - np.round(lod)) <= e_lod, e_lod * vr, 0.0)
        val[nz], bnd[nz] = v[nz], b[nz]
    return val, bnd


# ---------------------------------------------------------------------------------------------------------------- interactions
class Hit:
    """What a SurfaceInteraction hands a texture: p, dpdx, dpdy (n, 3), uv (n, 2), dudx, dvdx, dudy, dvdy (n,), float64 copies of the
    float32 inputs, and the absolute uncertainty of each group beyond float32 representation (0 when both sides get the same numbers)."""

    def __init__(self, n, p=None, uv=None, dpdx=None, dpdy=None, dudx=None, dvdx=None, dudy=None, dvdy=None, e_p=0.0, e_uv=0.0, e_dp=0.0, e_duv=0.0):
        z = lambda a, k: np.zeros((n, k)) if a is None else np.asarray(a, np.float64).reshape(n, k)
        self.n = n
        self.p, self.uv, self.dpdx, self.dpdy = z(p, 3), z(uv, 2), z(dpdx, 3), z(dpdy, 3)
        self.dudx, self.dvdx, self.dudy, self.dvdy = (z(a, 1)[:, 0] for a in (dudx, dvdx, dudy, dvdy))
        b = lambda e: np.broadcast_to(np.asarray(e, np.float64), (n,))
        self.e_p, self.e_uv, self.e_dp, self.e_duv = b(e_p), b(e_uv), b(e_dp), b(e_duv)


def _xf_point(m, p):
    """Transform::transform_point (transform.rs): row-major 4 x 4, divided by w where it is not 1."""
    m = np.asarray(m, np.float64).reshape(4, 4)
    q = p @ m[:3, :3].T + m[:3, 3]
    wp = p @ m[3, :3] + m[3, 3]
    return np.where((wp == 1.0)[:, None], q, q / wp[:, None])


def _xf_vector(m, v):
    return v @ np.asarray(m, np.float64).reshape(4, 4)[:3, :3].T


def _xf_err(m, v, point=True):
    """Rounding error of a 4 x 4 applied to v (n, 3): three roundings on the largest row's sum of magnitudes."""
    m = np.abs(np.asarray(m, np.float64).reshape(4, 4))
    return (np.abs(v) @ m[:3, :3].T + (m[:3, 3] if point else 0.0)).max(1) * 3 * U


def _sphere(m, p, e_p):
    """SphericalMapping2D::sphere (mapping2d.rs:60-66), spherical_theta / spherical_phi (misc.rs:96-104): (theta / pi, phi / 2 pi) and
    the absolute error of each.  acos is ill-conditioned at the poles (error / sin theta); a point exactly on the axis normalises
    exactly.  phi < 0 gets + 2 pi: a point within its error of the half-plane y = 0, x > 0 may land on either side (returned as `seam`)."""
    q = _xf_point(m, p)
    mag = np.abs(q).max(1) + 1e-300
    eq = _xf_err(m, p) * (not np.array_equal(np.asarray(m, np.float64).reshape(4, 4), np.eye(4))) + np.abs(np.asarray(m, np.float64).reshape(4, 4)[:3, :3]).sum(1).max() * e_p
    ln = np.sqrt((q * q).sum(1))
    v = q / ln[:, None]
    ev = (3 * U + 2 * eq / mag)                                          # relative-to-one error of each component of the unit vector
    z = np.clip(v[:, 2], -1.0, 1.0)
    on_axis = (q[:, 0] == 0) & (q[:, 1] == 0) & (eq == 0)
    sin_t = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    theta = np.arccos(z)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_theta = np.where(on_axis, 0.0, ev * np.abs(z) / sin_t) + 2 * U * theta
    ph = np.arctan2(v[:, 1], v[:, 0])
    phi = np.where(ph < 0, ph + 2 * PI, ph)
    rxy = np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_phi = np.where(on_axis, 0.0, 2 * ev / np.maximum(rxy, 1e-300) * np.maximum(np.abs(v[:, 0]), np.abs(v[:, 1]))) + 3 * U * (np.abs(phi) + 1)
    seam = (np.abs(ph) <= e_phi) & (v[:, 0] > 0) & ~((v[:, 1] == 0) & (eq == 0))
    st = np.stack([theta * INV_PI, phi * INV_2PI], 1)
    e = np.stack([e_theta * INV_PI + U * st[:, 0], e_phi * INV_2PI + U * st[:, 1]], 1)
    return st, e, seam


def _cylinder(m, p, e_p):
    """CylindricalMapping2D::cylinder (mapping2d.rs:105-109): ((pi + atan2(y, x)) / 2 pi, z) of the normalised vector.  atan2 jumps
    across y = 0, x < 0."""
    q = _xf_point(m, p)
    ident = np.array_equal(np.asarray(m, np.float64).reshape(4, 4), np.eye(4))
    mag = np.abs(q).max(1) + 1e-300
    eq = _xf_err(m, p) * (not ident) + np.abs(np.asarray(m, np.float64).reshape(4, 4)[:3, :3]).sum(1).max() * e_p
    v = q / np.sqrt((q * q).sum(1))[:, None]
    ev = 3 * U + 2 * eq / mag
    ph = np.arctan2(v[:, 1], v[:, 0])
    rxy = np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_phi = 2 * ev / np.maximum(rxy, 1e-300) * np.maximum(np.abs(v[:, 0]), np.abs(v[:, 1])) + 3 * U * (np.abs(ph) + PI)
    seam = (np.abs(np.abs(ph) - np.pi) <= e_phi) & ~((v[:, 1] == 0) & (eq == 0))
    st = np.stack([(PI + ph) * INV_2PI, v[:, 2]], 1)
    e = np.stack([e_phi * INV_2PI + U * st[:, 0], ev * np.abs(v[:, 2]) + U], 1)
    return st, e, seam


def _fix_wrap(d):
    """mapping2d.rs:78-88 (and :121-131, the same lines in the cylindrical mapping): component [1] only; continuous at +-0.5."""
    t = d[:, 1]
    t = np.where(t > 0.5, 1.0 - t, np.where(t < -0.5, -(t + 1.0), t))
    return np.stack([d[:, 0], t], 1)


def map2d(tex, hit):
    """TextureMapping2D::map (mapping2d.rs:40-46 uv, :68-91 spherical, :111-134 cylindrical, :155-174 planar).
    Returns st, dstdx, dstdy (n, 2), the absolute error of st (n,) and of the differentials (n,), and `seam` (n,): within its error of
    the mapping's own discontinuity.  The finite differences of the two angular mappings divide a difference of two mapped points by
    DELTA = 0.1: both points' errors come through, times 10."""
    kind = tex.get("mapping", "uv")
    n = hit.n
    no = np.zeros(n, bool)
    if kind == "uv":
        su, sv, du, dv = (c32(tex.get(k, d)) for k, d in (("uscale", 1.0), ("vscale", 1.0), ("udelta", 0.0), ("vdelta", 0.0)))
        sc = np.array([su, sv])
        st = sc * hit.uv + np.array([du, dv])
        dx, dy = sc * np.stack([hit.dudx, hit.dvdx], 1), sc * np.stack([hit.dudy, hit.dvdy], 1)
        e_st = (2 * U * (np.abs(sc * hit.uv) + np.abs([du, dv])) + np.abs(sc) * hit.e_uv[:, None]).max(1)
        e_d = U * np.maximum(np.abs(dx), np.abs(dy)).max(1) + np.abs(sc).max() * hit.e_duv
        return st, dx, dy, e_st, e_d, no
    if kind == "planar":
        v1, v2 = (np.array([c32(x) for x in tex.get(k, d)]) for k, d in (("v1", (1, 0, 0)), ("v2", (0, 1, 0))))
        du, dv = c32(tex.get("udelta", 0.0)), c32(tex.get("vdelta", 0.0))
        V = np.stack([v1, v2], 1)
        st = hit.p @ V + np.array([du, dv])
        dx, dy = hit.dpdx @ V, hit.dpdy @ V
        aV = np.abs(V)
        e_st = (4 * U * (np.abs(hit.p) @ aV + np.abs([du, dv])) + hit.e_p[:, None] * aV.sum(0)).max(1)
        e_d = (3 * U * np.maximum(np.abs(hit.dpdx) @ aV, np.abs(hit.dpdy) @ aV) + hit.e_dp[:, None] * aV.sum(0)).max(1)
        return st, dx, dy, e_st, e_d, no
    fn = _sphere if kind == "spherical" else _cylinder
    m = tex.get("world_to_texture", np.eye(4))
    delta = c32(0.1)
    inv_delta = c32(np.float32(1.0) / np.float32(0.1))
    st, e0, seam = fn(m, hit.p, hit.e_p)
    out = [st]
    e_d = np.zeros(n)
    for dp in (hit.dpdx, hit.dpdy):
        pd = hit.p + delta * dp
        e_pd = hit.e_p + delta * hit.e_dp + U * (delta * np.abs(dp).max(1) + np.abs(pd).max(1))       # the product and the sum, one rounding each
        sd, e1, _ = fn(m, pd, e_pd)
        d = (sd - st) * inv_delta
        e_d = np.maximum(e_d, ((e0 + e1).max(1) + U * np.abs(sd - st).max(1)) * inv_delta + U * np.abs(d).max(1))
        out.append(_fix_wrap(d))
    return out[0], out[1], out[2], e0.max(1), e_d, seam


def map3d(tex, hit):
    """IdentityMapping3D::map (mapping3d.rs:30-35): p and the differentials through the matrix; dpdy comes back as dpdx (:33)."""
    m = tex.get("world_to_texture", np.eye(4))
    ident = np.array_equal(np.asarray(m, np.float64).reshape(4, 4), np.eye(4))
    rs = np.abs(np.asarray(m, np.float64).reshape(4, 4)[:3, :3]).sum(1).max()
    p, dpdx = _xf_point(m, hit.p), _xf_vector(m, hit.dpdx)
    e_p = (0.0 if ident else _xf_err(m, hit.p)) + rs * hit.e_p
    e_dp = (0.0 if ident else _xf_err(m, hit.dpdx, False)) + rs * hit.e_dp
    return p, dpdx, dpdx, e_p, e_dp


# ---------------------------------------------------------------------------------------------------------------- noise
def noise(perm, x, y, z):
    """noise() and grad() (noise.rs:10-27, :60-94) with the permutation `perm` (256 entries, handed in by the caller).  Perlin noise is
    continuous across the lattice planes and under the & 255 of the lattice, so the floors need no step term."""
    perm = np.concatenate([perm, perm]).astype(np.int64)
    fx, fy, fz = np.floor(x), np.floor(y), np.floor(z)
    dx, dy, dz = x - fx, y - fy, z - fz
    ix, iy, iz = (f.astype(np.int64) & 255 for f in (fx, fy, fz))

    def grad(a, b, c, gx, gy, gz):
        hh = perm[perm[perm[a] + b] + c] & 15
        u = np.where((hh < 8) | (hh == 12) | (hh == 13), gx, gy)
        v = np.where((hh < 4) | (hh == 12) | (hh == 13), gy, gz)
        return np.where(hh & 1, -u, u) + np.where(hh & 2, -v, v)

    def wgt(t):
        t3 = t * t * t
        t4 = t3 * t
        return 6.0 * t4 * t - 15.0 * t4 + 10.0 * t3
    lerp = lambda t, a, b: (1.0 - t) * a + t * b
    w000, w100 = grad(ix, iy, iz, dx, dy, dz), grad(ix + 1, iy, iz, dx - 1, dy, dz)
    w010, w110 = grad(ix, iy + 1, iz, dx, dy - 1, dz), grad(ix + 1, iy + 1, iz, dx - 1, dy - 1, dz)
    w001, w101 = grad(ix, iy, iz + 1, dx, dy, dz - 1), grad(ix + 1, iy, iz + 1, dx - 1, dy, dz - 1)
    w011, w111 = grad(ix, iy + 1, iz + 1, dx, dy - 1, dz - 1), grad(ix + 1, iy + 1, iz + 1, dx - 1, dy - 1, dz - 1)
    wx, wy, wz = wgt(dx), wgt(dy), wgt(dz)
    x00, x10, x01, x11 = lerp(wx, w000, w100), lerp(wx, w010, w110), lerp(wx, w001, w101), lerp(wx, w011, w111)
    return lerp(wz, lerp(wy, x00, x10), lerp(wy, x01, x11))


def _noise_err(perm, lp, e_rel):
    """Error of one noise(lp) whose coordinates carry the relative error e_rel (x - floor(x) is exact in float32): the slope of the
    noise there, by central differences in float64, times each coordinate's error; the second-order term with 30 for the largest
    second derivative of a corner's weighted gradient; 40 roundings on values <= 2."""
    h = 1e-5
    e = np.abs(lp) * e_rel[:, None]
    lin = np.zeros(len(lp))
    for a in range(3):
        d = np.zeros(3)
        d[a] = h
        q0, q1 = lp - d, lp + d
        lin += np.abs(noise(perm, q1[:, 0], q1[:, 1], q1[:, 2]) - noise(perm, q0[:, 0], q0[:, 1], q0[:, 2])) / (2 * h) * e[:, a]
    return 1.1 * lin + 30.0 * e.sum(1) ** 2 + 40 * U


def fbm(perm, p, dpdx, dpdy, omega, max_octaves, turb=False, e_p=0.0, e_dp=0.0):
    """fbm (noise.rs:96-116) and turbulence (:118-148).  n = clamp(-1 - log2(len2) / 2, 0, octaves); log2(0) = -inf gives n = octaves.
    fbm is continuous where floor(n) steps: smooth_step(0.3, 0.7, .) is 0 and 1 around an integer.  turbulence is not (the loop adds
    |noise|, the partial term the signed noise, and the 0.2 tail gains a term): within the error of n of an integer it is left out.
    lambda is 1.99^i in f32: i roundings, so the point lambda * p carries (i + 1) u relative."""
    n_ev = len(p)
    omega = c32(omega)
    len2 = np.maximum((dpdx * dpdx).sum(1), (dpdy * dpdy).sum(1))
    with np.errstate(divide="ignore"):
        lg = np.log2(len2)
    n = np.clip(-1.0 - 0.5 * lg, 0.0, float(max_octaves))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_len = np.where(len2 > 0, 2 * np.sqrt(3.0) * e_dp / np.sqrt(len2), 0.0)
        e_n = np.where(np.isfinite(lg), 0.5 * ((6 * U + rel_len) / np.log(2.0) + 2 * U * np.abs(lg)) + 2 * U * (np.abs(n) + 1), 0.0)
    e_n = np.where((n <= 0) & (-1.0 - 0.5 * lg < -e_n), 0.0, e_n)      # clamped well inside: n is exactly 0 (or octaves) on both sides
    e_n = np.where((n >= max_octaves) & (-1.0 - 0.5 * lg > max_octaves + e_n), 0.0, e_n)
    n_int = np.floor(n).astype(np.int64)
    total, bound = np.zeros(n_ev), np.zeros(n_ev)
    lam, o = np.ones(n_ev), np.ones(n_ev)
    c199 = c32(1.99)
    pm = np.abs(p).max(1)
    for i in range(int(max_octaves) + 1):
        lp = lam[:, None] * p
        nz = noise(perm, lp[:, 0], lp[:, 1], lp[:, 2])
        e_nz = _noise_err(perm, lp, (i + 1) * U + e_p / np.maximum(pm, 1e-300))
        full = i < n_int
        part = i == n_int
        total += np.where(full, o * (np.abs(nz) if turb else nz), 0.0)
        bound += np.where(full, o * (e_nz + (i + 2) * U * np.abs(nz)), 0.0)
        v = np.clip((n - n_int - c32(0.3)) / (c32(0.7) - c32(0.3)), 0.0, 1.0)
        ss = v * v * (-2.0 * v + 3.0)
        e_ss = 1.5 / (c32(0.7) - c32(0.3)) * (e_n + 4 * U) + 4 * U
        total += np.where(part, o * ss * nz, 0.0)
        bound += np.where(part, o * (ss * e_nz + e_ss * np.abs(nz) + (i + 4) * U * np.abs(ss * nz)), 0.0)
        keep = full
        lam = np.where(keep, lam * c199, lam)
        o = np.where(keep, o * omega, o)
    if turb:
        for i in range(int(max_octaves)):
            m = i < n_int
            total += np.where(m, o * c32(0.2), 0.0)
            o = np.where(m, o * omega, o)
        bound = np.where((e_n > 0) & (np.abs(n - np.round(n)) <= e_n), INF, bound)
    bound = bound + (2 * max_octaves + 4) * U * np.abs(total)
    return total, bound


MARBLE_C = [[0.58, 0.58, 0.6], [0.58, 0.58, 0.6], [0.58, 0.58, 0.6], [0.5, 0.5, 0.5], [0.6, 0.59, 0.58], [0.58, 0.58, 0.6], [0.58, 0.58, 0.6],
            [0.2, 0.2, 0.33], [0.58, 0.58, 0.6]]                      # marble.rs:63-73: the colours are settings of the texture, not code


def marble(perm, tex, hit):
    """MarbleTexture::evaluate_colors (marble.rs:34-60).  first = min(1, floor(6 t)) (:46) jumps between two Bezier segments that do
    not meet: within the error of 6 t of 1 the evaluation is left out.  De Casteljau runs at t up to 5, outside [0, 1]: the error of t
    goes through the cubic's slope, and the roundings through (|1 - t| + |t|)^3 times the largest colour."""
    p, dpdx, dpdy, e_p, e_dp = map3d(tex, hit)
    sc, var = c32(tex.get("scale", 1.0)), c32(tex.get("variation", 0.2))
    p = sc * p
    f, bf = fbm(perm, p, sc * dpdx, sc * dpdy, tex.get("roughness", 0.5), tex.get("octaves", 8), False, sc * e_p + U * np.abs(p).max(1), sc * e_dp + U * sc * np.abs(dpdx).max(1))
    mb = p[:, 1] + var * f
    e_mb = sc * e_p + 2 * U * np.abs(p[:, 1]) + var * bf + 2 * U * np.abs(var * f)
    t = 0.5 + 0.5 * np.sin(mb)
    e_t = 0.5 * (e_mb + 2 * U * np.abs(mb) + 2 * U) + 2 * U
    x = t * 6.0
    first = np.minimum(1, np.floor(x)).astype(np.int64)
    tt = x - first
    e_tt = 6 * e_t + 2 * U * 6
    C = np.array([[c32(v) for v in row] for row in MARBLE_C])

    def spline(u):
        u = u[:, None]
        lr = lambda a, b: a * (1 - u) + b * u
        c0, c1, c2, c3 = C[first], C[first + 1], C[first + 2], C[first + 3]
        s0, s1, s2 = lr(c0, c1), lr(c1, c2), lr(c2, c3)
        s0, s1 = lr(s0, s1), lr(s1, s2)
        return lr(s0, s1) * 1.5
    val = spline(tt)
    hstep = 1e-6
    slope = np.abs(spline(tt + hstep) - spline(tt - hstep)).max(1) / (2 * hstep)
    amp = (np.abs(1 - tt) + np.abs(tt)) ** 3 * 1.5 * C.max()
    bound = 2 * slope * e_tt + 12 * U * amp
    bound = np.where(np.abs(x - 1.0) <= 6 * e_t + 12 * U, INF, bound)
    return val, bound


# ---------------------------------------------------------------------------------------------------------------- checkerboard
def bump_int(x):
    """checkerboard.rs:36-39: the integral of the square wave that is 1 on odd cells."""
    return np.floor(x / 2.0) + 2.0 * np.maximum(x / 2.0 - np.floor(x / 2.0) - 0.5, 0.0)


def checker_area(s, t, ds, dt):
    """The share of the box [s - ds, s + ds] x [t - dt, t + dt] covered by cells with odd floor(s) + floor(t), summed cell by cell:
    the geometric meaning of the closed form, computed without it.  Scalars; ds, dt > 0."""
    s0, s1, t0, t1 = s - ds, s + ds, t - dt, t + dt
    odd = 0.0
    for i in range(int(np.floor(s0)), int(np.floor(s1)) + 1):
        ws = min(s1, i + 1.0) - max(s0, float(i))
        if ws <= 0:
            continue
        for j in range(int(np.floor(t0)), int(np.floor(t1)) + 1):
            wt = min(t1, j + 1.0) - max(t0, float(j))
            if wt > 0 and (i + j) % 2 != 0:
                odd += ws * wt
    return odd / ((s1 - s0) * (t1 - t0))


def _near_int(x, e):
    return np.abs(x - np.round(x)) <= e


def checkerboard2d(tex, hit, c0, c1, b0, b1):
    """Checkerboard2DTexture::evaluate (checkerboard.rs:44-81) given the two children's values (n, 3) and bounds.
    Point sampling (aamode none, or the box inside one cell) is discontinuous at the cell edges: st within its error of one is left
    out (for the box-inside-one-cell branch only if the box itself does not reach the edge; where it does, the closed form takes over
    continuously).  The closed form divides a difference of two bump_int by 2 ds: each bump_int carries 4 u (|x| + 1) and the error of
    its argument (slope <= 1).  ds > 1 or dt > 1 switches to 1/2: left out within the error of ds of 1.  ds == 0 with the box
    crossing an edge in t divides 0 by 0: NaN on both sides, returned as NaN with bound 0."""
    st, dx, dy, e_st, e_d, seam = map2d(tex, hit)
    s, t = st[:, 0], st[:, 1]
    dc = np.abs(c1 - c0).max(1)

    def point():
        par = (np.floor(s) + np.floor(t)) % 2 == 0
        return np.where(par[:, None], c0, c1), np.where(par, b0, b1)
    pv, pb = point()
    at_edge = _near_int(s, e_st + U * np.abs(s)) | _near_int(t, e_st + U * np.abs(t)) | seam
    if tex.get("aamode", "closedform") == "none":
        return pv, np.where(at_edge & (dc > 0), INF, pb)
    ds = np.maximum(np.abs(dx[:, 0]), np.abs(dy[:, 0]))
    dt = np.maximum(np.abs(dx[:, 1]), np.abs(dy[:, 1]))
    s0, s1, t0, t1 = s - ds, s + ds, t - dt, t + dt
    inside = (np.floor(s0) == np.floor(s1)) & (np.floor(t0) == np.floor(t1))
    ex_s, ex_t = e_st + e_d + 2 * U * (np.abs(s) + ds), e_st + e_d + 2 * U * (np.abs(t) + dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        sint = (bump_int(s1) - bump_int(s0)) / (2.0 * ds)
        tint = (bump_int(t1) - bump_int(t0)) / (2.0 * dt)
        e_sint = (2 * ex_s + 4 * U * (np.abs(s0) + np.abs(s1) + 2)) / (2.0 * ds) + np.abs(sint) * (3 * U + e_d / ds)
        e_tint = (2 * ex_t + 4 * U * (np.abs(t0) + np.abs(t1) + 2)) / (2.0 * dt) + np.abs(tint) * (3 * U + e_d / dt)
    area2 = sint + tint - 2.0 * sint * tint
    e_area = e_sint * (1 + 2 * np.abs(tint)) + e_tint * (1 + 2 * np.abs(sint)) + 6 * U
    big = (ds > 1.0) | (dt > 1.0)
    area2 = np.where(big, 0.5, area2)
    e_area = np.where(big, 0.0, e_area)
    a = area2[:, None]
    cv = c0 * (1 - a) + c1 * a
    with np.errstate(invalid="ignore"):
        cb = e_area * dc + np.abs(1 - area2) * b0 + np.abs(area2) * b1 + 4 * U * np.maximum(np.abs(c0), np.abs(c1)).max(1)
    cb = np.where(_near_int(ds, e_d + U) & (np.round(ds) == 1) | _near_int(dt, e_d + U) & (np.round(dt) == 1), INF, cb)
    cb = np.where(np.isnan(area2), 0.0, cb)
    cb = np.where(seam, INF, cb)
    # box inside one cell: the point sample, unless the point itself is within its error of an edge while the box is not known to reach it
    box_reaches = _near_int(s0, ex_s) | _near_int(s1, ex_s) | _near_int(t0, ex_t) | _near_int(t1, ex_t)
    pb2 = np.where(at_edge & (dc > 0), INF, pb + np.where(box_reaches, (e_area + 2 * (ex_s / np.maximum(ds, 1e-300) + ex_t / np.maximum(dt, 1e-300))) * dc, 0.0))
    with np.errstate(invalid="ignore"):
        pb2 = np.where(np.isfinite(pb2), pb2, INF)
    return np.where(inside[:, None], pv, cv), np.where(inside, pb2, cb)


def checkerboard3d(tex, hit, c0, c1, b0, b1):
    """Checkerboard3DTexture::evaluate (checkerboard.rs:104-117): the parity of the three floors of the mapped point; left out within
    the point's error of a cell face."""
    p, _, _, e_p, _ = map3d(tex, hit)
    par = np.floor(p).sum(1) % 2 == 0
    edge = _near_int(p, np.broadcast_to(e_p, (len(p),))[:, None] + 4 * U * np.abs(p)).any(1)
    dc = np.abs(c1 - c0).max(1)
    return np.where(par[:, None], c0, c1), np.where(edge & (dc > 0), INF, np.where(par, b0, b1))


def dots(perm, tex, hit, c_out, c_in, b_out, b_in):
    """DotsTexture::evaluate (dots.rs:26-41).  Three deciding comparisons: the cell (floor(st + 0.5)), noise > 0, and the squared
    distance against radius^2; within its error of the first or the last the evaluation is left out.  The middle one decides exactly:
    its arguments (cell + 0.5, cell + 0.5, 0) are half-integers, and every intermediate of noise() at a half-integer point is a dyadic
    number of a few bits, the same in float32 and float64."""
    st, _, _, e_st, _, seam = map2d(tex, hit)
    cell = np.floor(st + 0.5)
    z = np.zeros(len(st))
    n0 = noise(perm, cell[:, 0] + 0.5, cell[:, 1] + 0.5, z)
    radius = c32(0.35)
    shift = c32(np.float32(0.5) - np.float32(0.35))
    ctr = cell + shift * np.stack([noise(perm, cell[:, 0] + c32(1.5), cell[:, 1] + c32(2.8), z), noise(perm, cell[:, 0] + c32(4.5), cell[:, 1] + c32(9.8), z)], 1)
    e_noise = 40 * U + 2 * 4 * U * (np.abs(cell).max(1) + 10)           # the centres: cell + 2.8 (9.8) rounds, through a slope <= 4, and 40 roundings
    d = st - ctr
    d2 = (d * d).sum(1)
    e_d2 = 2 * np.abs(d).sum(1) * (e_st + shift * e_noise + 3 * U * (np.abs(st).max(1) + 1)) + 4 * U * d2
    inside = (n0 > 0) & (d2 < radius * radius)
    unsure = _near_int(st + 0.5, (e_st + 2 * U * (np.abs(st) + 0.5).max(1))[:, None]).any(1) | ((n0 > 0) & (np.abs(d2 - radius * radius) <= e_d2 + 2 * U)) | seam
    dc = np.abs(c_in - c_out).max(1)
    return np.where(inside[:, None], c_in, c_out), np.where(unsure & (dc > 0), INF, np.where(inside, b_in, b_out))


# ---------------------------------------------------------------------------------------------------------------- the evaluator
def evaluate(tex, hit, perm=None):
    """Texture::evaluate of a texture given as a dict {"type": ..., parameters as in the scene file} whose children ("tex1", "tex2",
    "amount") are dicts, numbers or RGB triples.  Returns value (n, 3), bound (n,), scale (n,): the scale the cap of 1e-3 is taken
    of (the image's texel range, the difference of the two children for checkerboard / mix / dots, 1 for the noise kinds)."""
    n = hit.n
    if not isinstance(tex, dict):
        v = np.array([c32(x) for x in (tex if isinstance(tex, (tuple, list)) else (tex,) * 3)])
        return np.broadcast_to(v, (n, 3)).copy(), np.zeros(n), np.full(n, max(np.abs(v).max(), 1e-30))
    kind = tex["type"]
    child = lambda k, d: evaluate(tex.get(k, d), hit, perm)
    one = np.ones(n)
    if kind == "constant":
        return evaluate(tex["value"], hit, perm)
    if kind == "scale":                                                                   # scale.rs: tex1 * tex2
        a, ba, sa = child("tex1", 1.0)
        b, bb, sb = child("tex2", 1.0)
        am, bm = np.abs(a).max(1), np.abs(b).max(1)
        return a * b, ba * bm + bb * am + ba * bb + U * am * bm, np.maximum(sa * bm, sb * am)
    if kind == "mix":                                                                     # mix.rs: (1 - amt) * t1 + amt * t2
        a, ba, sa = child("tex1", 1.0)
        b, bb, sb = child("tex2", 1.0)
        m, bm, _ = child("amount", 0.5)
        m = m[:, :1]
        dc = np.abs(b - a).max(1)
        return a * (1 - m) + b * m, np.abs(1 - m[:, 0]) * ba + np.abs(m[:, 0]) * bb + bm * dc + 4 * U * np.maximum(np.abs(a), np.abs(b)).max(1), np.maximum(dc, np.maximum(sa, sb))
    if kind == "checkerboard":
        a, ba, sa = child("tex1", 1.0)
        b, bb, sb = child("tex2", 0.0)
        f = checkerboard3d if tex.get("dimension", 2) == 3 else checkerboard2d
        v, bd = f(tex, hit, a, b, ba, bb)
        return v, bd, np.maximum(np.abs(b - a).max(1), 1e-30)
    if kind == "dots":                                                                    # dots.rs
        a, ba, _ = child("tex1", 1.0)                                                     # :19-20: tex1 is outside_dot, tex2 inside_dot
        b, bb, _ = child("tex2", 0.0)
        v, bd = dots(perm, tex, hit, a, b, ba, bb)
        return v, bd, np.maximum(np.abs(b - a).max(1), 1e-30)
    if kind == "uv":                                                                      # uv.rs: (s - floor(s), t - floor(t), 0); a sawtooth
        st, _, _, e_st, _, seam = map2d(tex, hit)
        fr = st - np.floor(st)
        bd = np.where(_near_int(st, (e_st + U * np.abs(st).max(1))[:, None]).any(1) | seam, INF, e_st + 2 * U * (np.abs(st).max(1) + 1))
        return np.concatenate([fr, np.zeros((n, 1))], 1), bd, one
    if kind == "bilerp":                                                                  # bilerp.rs
        st, _, _, e_st, _, seam = map2d(tex, hit)
        s, t = st[:, :1], st[:, 1:]
        vs = [np.array([c32(x) for x in (tex[k] if isinstance(tex[k], (tuple, list)) else (tex[k],) * 3)]) for k in ("v00", "v01", "v10", "v11")]
        w = [(1 - s) * (1 - t), (1 - s) * t, s * (1 - t), s * t]
        val = sum(wi * vi for wi, vi in zip(w, vs))
        vm = max(np.abs(v).max() for v in vs)
        mag = (1 + np.abs(s[:, 0])) * (1 + np.abs(t[:, 0]))
        bd = vm * (2 * e_st * (2 + np.abs(s[:, 0]) + np.abs(t[:, 0])) + 12 * U * mag)
        return val, np.where(seam, INF, bd), np.full(n, max(vm, 1e-30))
    if kind == "imagemap":                                                                # imagemap.rs:57-70
        st, dx, dy, e_st, e_d, seam = map2d(tex, hit)
        lv = tex["levels"]
        sw, tw = tex.get("swrap", tex.get("wrap", REPEAT)), tex.get("twrap", tex.get("wrap", REPEAT))
        v, bd = lookup_delta(lv, st, dx, dy, tex.get("trilinear", False), tex.get("maxanisotropy", 8.0), sw, tw, e_st, e_d)
        if v.shape[1] == 1:
            v = np.repeat(v, 3, 1)
        vr, vm = _vrange(lv, sw, tw)                                                       # a one-texel image has no range: its texel's magnitude then
        return v, np.where(seam & (REPEAT not in (tw,)), INF, bd), np.full(n, vr if vr > 0 else max(vm, 1e-30))
    if kind in ("fbm", "wrinkled"):                                                       # fbm.rs, wrinkled.rs
        p, dpdx, dpdy, e_p, e_dp = map3d(tex, hit)
        v, bd = fbm(perm, p, dpdx, dpdy, tex.get("roughness", 0.5), tex.get("octaves", 8), kind == "wrinkled", e_p, e_dp)
        return np.repeat(v[:, None], 3, 1), bd, one
    if kind == "windy":                                                                   # windy.rs:14-19
        p, dpdx, dpdy, e_p, e_dp = map3d(tex, hit)
        k = c32(0.1)
        ws, b1 = fbm(perm, k * p, k * dpdx, k * dpdy, 0.5, 3, False, k * e_p + U * k * np.abs(p).max(1), k * e_dp + U * k * np.abs(dpdx).max(1))
        wh, b2 = fbm(perm, p, dpdx, dpdy, 0.5, 6, False, e_p, e_dp)
        v = np.abs(ws) * wh
        return np.repeat(v[:, None], 3, 1), b1 * np.abs(wh) + b2 * np.abs(ws) + b1 * b2 + U * np.abs(v), one
    if kind == "marble":
        v, bd = marble(perm, tex, hit)                                                    # the spline runs outside [0, 1] (:46): the value's own size
        return v, bd, np.maximum(one, np.abs(v).max(1))
    raise ValueError(kind)


CAP = 1e-3


def judge(got, value, bound, scale, extra=0.0):
    """The comparison every test makes: `got` against `value` within `bound` (+ extra), evaluations whose bound exceeds CAP times their
    scale (or is infinite: next to a discontinuity) left out.  Returns (worst excess over the bound among the kept, share left out,
    index of the worst).  NaN equals NaN."""
    got = np.asarray(got, np.float64)
    keep = np.isfinite(bound) & (bound <= CAP * scale)
    both_nan = np.isnan(got) & np.isnan(value)
    with np.errstate(invalid="ignore"):
        err = np.where(both_nan, 0.0, np.abs(got - value))
    err = np.where(np.isnan(err), INF, err).max(1)
    excess = np.where(keep, err - (bound + extra), -INF)
    i = int(np.argmax(excess)) if len(excess) else 0
    return (float(excess[i]) if len(excess) else -INF), float(1.0 - keep.mean()), i


# ---------------------------------------------------------------------------------------------------------------- camera and hit
def look_at_c2w(eye, look, up):
    """Matrix4x4::camera_to_world (matrix4x4.rs:146-...): columns right, up, dir, pos with right = normalize(cross(normalize(up), dir))."""
    eye, look, up = (np.asarray(v, np.float64) for v in (eye, look, up))
    d = look - eye
    d /= np.linalg.norm(d)
    up = up / np.linalg.norm(up)
    right = np.cross(up, d)
    right /= np.linalg.norm(right)
    nu = np.cross(d, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, nu, d, eye
    return m


def concentric_sample_disk(u):
    """sampling.rs concentric_sample_disk."""
    o = 2.0 * u - 1.0
    x, y = o[:, 0], o[:, 1]
    a = np.abs(x) > np.abs(y)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(a, x, y)
        th = np.where(a, (np.pi / 4) * (y / x), np.pi / 2 - (np.pi / 4) * (x / y))
    out = r[:, None] * np.stack([np.cos(th), np.sin(th)], 1)
    return np.where(((x == 0) & (y == 0))[:, None], 0.0, out)


class Camera:
    """PerspectiveCamera (cameras/perspective.rs:28-81, :121-180) over ProjectiveCamera::new (core/camera/projective.rs:34-43) and
    Transform::perspective (transform.rs:89-99), in float64 from the scene description: look_at, fov, resolution, lens."""

    def __init__(self, eye, look, up, fov, xres, yres, lensradius=0.0, focaldistance=1e6, spp=1):
        self.c2w = look_at_c2w(eye, look, up)
        n, f = c32(1e-2), 1000.0
        persp = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, f / (f - n), -f * n / (f - n)], [0, 0, 1, 0]], np.float64)
        it = 1.0 / np.tan(np.radians(c32(fov)) / 2.0)
        c2s = np.diag([it, it, 1.0, 1.0]) @ persp
        aspect = xres / yres
        sw = (-aspect, aspect, -1.0, 1.0) if aspect > 1 else (-1.0, 1.0, -1.0 / aspect, 1.0 / aspect)          # x0, x1, y0, y1 (api.rs screen window)
        tr = np.eye(4)
        tr[0, 3], tr[1, 3] = -sw[0], -sw[3]
        s2r = np.diag([xres, yres, 1.0, 1.0]) @ np.diag([1.0 / (sw[1] - sw[0]), 1.0 / (sw[2] - sw[3]), 1.0, 1.0]) @ tr
        self.r2c = np.linalg.inv(c2s) @ np.linalg.inv(s2r)
        o = self._r2c(np.zeros((1, 2)))
        self.dx = self._r2c(np.array([[1.0, 0.0]])) - o
        self.dy = self._r2c(np.array([[0.0, 1.0]])) - o
        self.lens, self.focal, self.scale = c32(lensradius), c32(focaldistance), np.sqrt(1.0 / spp)             # sampler.rs:218

    def _r2c(self, pf):
        q = np.concatenate([pf, np.zeros((len(pf), 1)), np.ones((len(pf), 1))], 1) @ self.r2c.T
        return q[:, :3] / q[:, 3:]

    def rays(self, pfilm, plens=None):
        """generate_ray_differential (:121-180) then scale_differentials (ray_differential.rs:26-35) by sqrt(1 / spp): world-space
        o, d, rx_o, rx_d, ry_o, ry_d (n, 3)."""
        nrm = lambda v: v / np.linalg.norm(v, axis=1)[:, None]
        pc = self._r2c(np.asarray(pfilm, np.float64))
        o = np.zeros_like(pc)
        d = nrm(pc)
        dxd, dyd = nrm(pc + self.dx), nrm(pc + self.dy)
        rxo = ryo = o
        if self.lens > 0:
            pl = concentric_sample_disk(np.asarray(plens, np.float64)) * self.lens
            pl3 = np.concatenate([pl, np.zeros((len(pl), 1))], 1)
            focus = lambda v: v * (self.focal / v[:, 2])[:, None]
            d, dxd, dyd = nrm(focus(d) - pl3), nrm(focus(dxd) - pl3), nrm(focus(dyd) - pl3)
            o = rxo = ryo = pl3
        R, T = self.c2w[:3, :3], self.c2w[:3, 3]
        w = lambda v: v @ R.T
        o, rxo, ryo = w(o) + T, w(rxo) + T, w(ryo) + T
        d, dxd, dyd = w(d), w(dxd), w(dyd)
        s = self.scale
        return o, d, o + (rxo - o) * s, d + (dxd - d) * s, o + (ryo - o) * s, d + (dyd - d) * s


def quad_hit(P, UV, o, d, rxo, rxd, ryo, ryd):
    """The hit of the main ray with the planar quad P[0..3] (two triangles 0 1 2, 0 2 3, uv UV) and
    SurfaceInteraction::compute_differentials (surface_interaction.rs:221-282) there: the offset rays meet the tangent plane at px, py;
    dpdx = px - p, and (dudx, dvdx) solves [dpdu dpdv] (du, dv) = dpdx on the two axes the normal is smallest on.  The uv of a quad
    whose uv is affine in position is affine too, so uv and its differences are computed from that map directly; the 2 x 2 solve of the
    reference has the same solution wherever its determinant is not ~0.
    Returns a dict: p, uv, dpdx, dpdy, dudx.., `inside` (main and offset rays hit inside the quad), `margin` (smallest barycentric
    distance of the three hits from an edge, in uv units), cos (|n . d|), t."""
    P, UV = np.asarray(P, np.float64), np.asarray(UV, np.float64)
    e1, e2 = P[1] - P[0], P[3] - P[0]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm)
    M = np.stack([e1, e2], 1)                                           # p - P0 = M (a, b)
    Mp = np.linalg.pinv(M)

    def plane(oo, dd):
        t = ((P[0] - oo) @ nrm) / (dd @ nrm)
        return oo + t[:, None] * dd, t
    p, t = plane(o, d)
    px, _ = plane(rxo, rxd)
    py, _ = plane(ryo, ryd)
    ab = lambda q: (q - P[0]) @ Mp.T
    A = np.stack([UV[1] - UV[0], UV[3] - UV[0]], 1)
    uv = lambda q: ab(q) @ A.T + UV[0]
    a0, ax, ay = ab(p), ab(px), ab(py)
    margin = np.min(np.stack([np.minimum(a, 1 - a).min(1) for a in (a0, ax, ay)]), 0)
    u0, ux, uy = uv(p), uv(px), uv(py)
    return dict(p=p, uv=u0, dpdx=px - p, dpdy=py - p, dudx=ux[:, 0] - u0[:, 0], dvdx=ux[:, 1] - u0[:, 1], dudy=uy[:, 0] - u0[:, 0], dvdy=uy[:, 1] - u0[:, 1],
                inside=(margin > 0) & (t > 0), margin=margin, cos=np.abs(d @ nrm), t=t, n=nrm)


def quad_hit_errors(P, UV, h, o, rxo, rxd, ryo, ryd, gain=1.0):
    """What a float32 evaluation of the same hit may differ by (absolute): e_p, e_uv, e_dp, e_duv for texture_ref.Hit, per sample.

      p, uv      interpolated from the vertices with the barycentrics: 4 roundings on the largest vertex (uv) magnitude;
      px, py     t = (n . p - n . o) / (n . d): each dot carries 3 roundings on its sum of magnitudes, the offset direction 4 more;
                 the point o + t d adds 2 on |o| + |t d|.  The division by n . d makes this grow as 1 / cos at grazing incidence.
                 The normal's own error (4 roundings) tilts the plane about p, which it contains by construction: that moves px by
                 4 u |px - p| / cos, relative to the differential and not to the distance;
      dpdx       px - p: both errors, and one rounding;
      du, dv     the 2 x 2 solve A x = b on the two axes the normal is smallest on (surface_interaction.rs:255-281): |A^-1| times
                 (the error of b + 8 roundings of A times |x|), and the cancellation of a11 b0 - a01 b1 over the determinant.
    `gain` multiplies what went through a matrix when the quad is an instance: p, uv and the normal (the hit is computed in object
    space and carried back); the offset rays meet the plane in world space either way."""
    P, UV = np.asarray(P, np.float64), np.asarray(UV, np.float64)
    n = h["n"]
    pm, om = np.abs(P).max(), np.abs(o).max(1)
    e_p = gain * 4 * U * pm + 0 * om
    e_uv = gain * 4 * U * np.abs(UV).max() + 0 * om
    an = np.abs(n)
    Snp = np.abs(h["p"]) @ an

    def offset(oo, dd, pt):
        num, den = (P[0] - oo) @ n, dd @ n
        e_num = 3 * U * (np.abs(oo) @ an + Snp) + U * np.abs(num)
        e_den = 7 * U * (np.abs(dd) @ an)
        t = num / den
        rel_t = e_num / np.abs(num) + e_den / np.abs(den) + 2 * U
        td = np.abs(t[:, None] * dd).max(1)
        return td * rel_t + 2 * U * (np.abs(oo).max(1) + td) + gain * 4 * U * np.abs(pt).max(1) / np.abs(den)
    e_px, e_py = offset(rxo, rxd, h["dpdx"]), offset(ryo, ryd, h["dpdy"])
    e_dp = np.maximum(e_px, e_py) + e_p + U * np.maximum(np.abs(h["dpdx"]).max(1), np.abs(h["dpdy"]).max(1))
    e1, e2 = P[1] - P[0], P[3] - P[0]
    Auv = np.stack([UV[1] - UV[0], UV[3] - UV[0]], 1)
    D = np.stack([e1, e2], 1) @ np.linalg.inv(Auv)                      # columns dpdu, dpdv
    drop = int(np.argmax(an))
    ax = [a for a in range(3) if a != drop]
    A = D[ax, :]
    Ai = np.linalg.inv(A)
    det = abs(np.linalg.det(A))
    e_duv = np.zeros(len(om))
    for dp, x0, x1 in ((h["dpdx"], h["dudx"], h["dvdx"]), (h["dpdy"], h["dudy"], h["dvdy"])):
        xm = np.maximum(np.abs(x0), np.abs(x1))
        b = np.abs(dp[:, ax])
        cancel = 3 * U * np.maximum(np.abs(A[1, 1]) * b[:, 0] + np.abs(A[0, 1]) * b[:, 1], np.abs(A[0, 0]) * b[:, 1] + np.abs(A[1, 0]) * b[:, 0]) / det
        e_duv = np.maximum(e_duv, np.abs(Ai).sum(1).max() * (e_dp + 16 * U * np.abs(A).max() * xm) + cancel + 4 * U * xm)
    return dict(e_p=e_p, e_uv=e_uv, e_dp=e_dp, e_duv=e_duv)
