"""Float64 numpy restatement of the last stage of every render: the reconstruction filters, Film::new's table and bounds, the film tile's
add_sample_filter, the tile merge and write_image -- written from the reference's text and taking nothing from the code under test: no
import of oracle_lib or of the package.  Every evaluator returns a value and a *bound*: how far a correct float32 evaluation of the same
formula (the reference computes in f32, in whatever order its tiles merge; the device's atomics reorder too) may lie from the float64
value.  The bound is derived per table entry and per pixel:

  smooth parts   a count of float32 roundings x 2^-24 x the magnitude of the terms; sums in any order, gamma(n) on the sum of |terms|;
  steps          a table index (floor of d * lx) or a `d <= r` that the float32 chain may decide the other way widens the bound by what
                 the other decision would change, for the pixel and -- through 1 / sum -- for every pixel of that sample's footprint;
  integers       Film::new's crop and get_sample_bounds are decisions, restated exactly in np.float32.

The inputs (p_film, radiance, the table, the radii, the clamp) are float32 numbers on both sides and are taken as data.  The constants
are the reference's f32 literals.

Where the reference's text and the textbook differ the text wins:
  * the table samples the filter at x * r / 15, x = 0..15, both ends included, not at bin centres            (film.rs:109-116)
  * the cropped bounds floor both minima ("ceil -> floor")                                                  (film.rs:73-80)
  * sample bounds and footprints are floor(p - r) .. ceil(p + r) without the half-pixel shift               (film.rs:174-177, film_tile.rs:95-96)
  * the footprint's weights are divided by their own sum (quirk Q1), and a sum <= 0 drops the sample         (film_tile.rs:151-160)
  * SincFilter::sinc multiplies by PI itself, and the window is sinc(x / tau)                               (sinc.rs:17-33)
"""
import numpy as np

U = 2.0 ** -24            # unit roundoff of float32
ULP = 2.0 * U             # one ulp of a float32 result, relative (a libm expf / sinf term)
FT_W = 16                 # film.rs: FT_W, the table is FT_W x FT_W
LEAVE_OUT = 1e-3          # a pixel whose bound exceeds this share of the largest |value| on the film is left out (the rule of texture_ref.py)


def c32(x):
    """An f32 literal of the reference as the float64 number it is."""
    return float(np.float32(x))


def gamma(n):
    """n float32 roundings on one term: n u / (1 - n u)."""
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


PI = c32(np.pi)
YWEIGHT = np.array([c32(0.212671), c32(0.715160), c32(0.072169)])                                    # spectrum/rgb.rs:8
RGB2XYZ = np.array([[c32(0.412453), c32(0.357580), c32(0.180423)],                                   # spectrum/convert.rs:11-17
                    [c32(0.212671), c32(0.715160), c32(0.072169)],
                    [c32(0.019334), c32(0.119193), c32(0.950227)]])
XYZ2RGB = np.array([[c32(3.240479), c32(-1.537150), c32(-0.498535)],                                 # spectrum/convert.rs:3-9
                    [c32(-0.969256), c32(1.875991), c32(0.041556)],
                    [c32(0.055648), c32(-0.204043), c32(1.057311)]])


# ---------------------------------------------------------------------------------------------------------------- the five filters
# Each 1-D factor takes the real argument x >= 0 with its absolute uncertainty ex and returns (value, bound).
def _lin(terms):
    """A coefficient `a0*v0 + a1*v1 + ...` evaluated left to right in f32 (a term with v None is a literal): value and bound.  Every
    product and every partial sum rounds once."""
    val, err, first = 0.0, 0.0, True
    for a, v in terms:
        t = a if v is None else a * v
        if v is not None:
            err += U * abs(t)
        val += t
        if not first:
            err += U * abs(val)
        first = False
    return val, err


def _poly(coefs, x, ex):
    """sum c_k x^k as the reference writes it, ((c*x)*x)*x + (c*x)*x + c*x + c, term by term: coefs = {k: (c, err_c)}.  A term rounds k
    times and carries k times the relative error of x; the additions are gamma(3) on the sum of |terms| (they cancel near the zero
    crossings, which is why the count is on magnitudes)."""
    val, err, mag = 0.0, 0.0, 0.0
    relx = ex / x if x > 0 else 0.0
    for k, (c, ec) in coefs.items():
        t = c * x ** k
        val += t
        mag += abs(t)
        err += ec * x ** k + abs(t) * (gamma(k) + ((1.0 + relx) ** k - 1.0))
    return val, err + gamma(3) * (mag + err)


def box_1d(x, ex, r):
    """filters/box_filter.rs:18-20: evaluate == 1."""
    return 1.0, 0.0


def triangle_1d(x, ex, r):
    """filters/triangle.rs:17-21: max(0, r - |x|).  One subtraction."""
    v = r - abs(x)
    return max(0.0, v), ex + U * abs(v)


def gaussian_1d(x, ex, r, alpha):
    """filters/gaussian.rs:12-24: max(0, exp(-alpha d d) - exp(-alpha r r)); (-alpha * d) * d rounds twice, expf is 1 ulp of its result.
    The error is counted before the max: the two exponentials cancel near the edge, so their absolute errors add."""
    def e(d, ed):
        z = alpha * d * d
        ez = abs(z) * (gamma(2) + ((1.0 + (ed / d if d > 0 else 0.0)) ** 2 - 1.0))
        v = np.exp(-z)
        return v, v * np.expm1(ez) + ULP * v * (1.0 + np.expm1(ez))
    v, bv = e(abs(x), ex)
    vr, bvr = e(r, 0.0)
    return max(0.0, v - vr), bv + bvr + U * (abs(v - vr) + bv + bvr)


def mitchell_1d(x, ex, r, B, C):
    """filters/mitchell.rs:20-47 on x * inv_radius: the two cubics term by term.  inv_radius = fl(1 / r) and the product round once
    each, the doubling is exact.  The cubics meet continuously at |2x| = 1; an argument within its error of 1 adds their difference."""
    b, c = B, C
    a = 2.0 * abs(x) / r
    ea = 2.0 * ex / r + gamma(2) * a
    outer = {3: _lin([(-b, None), (-6.0, c)]), 2: _lin([(6.0, b), (30.0, c)]), 1: _lin([(-12.0, b), (-48.0, c)]), 0: _lin([(8.0, b), (24.0, c)])}
    inner = {3: _lin([(12.0, None), (-9.0, b), (-6.0, c)]), 2: _lin([(-18.0, None), (12.0, b), (6.0, c)]), 0: _lin([(6.0, None), (-2.0, b)])}
    vo, bo = _poly(outer, a, ea)
    vi, bi = _poly(inner, a, ea)
    v, bv = (vo, bo) if a > 1.0 else (vi, bi)
    if abs(a - 1.0) <= ea:
        bv += abs(vo - vi)
    sixth = c32(1.0 / 6.0)
    return v * sixth, (bv + U * (abs(v) + bv)) * sixth


def _sinc(x, ex):
    """SincFilter::sinc (sinc.rs:17-24): sin(PI x) / (PI x), 1 below 1e-5.  PI * x rounds once; sinf is 1 ulp of its result, and its
    argument's absolute error stays what it is where sin crosses zero (the integers): that is the conditioning."""
    x = abs(x)
    small = c32(1e-5)
    if x + ex < small:
        return 1.0, 0.0
    y = PI * x
    ey = PI * ex + U * y
    s = np.sin(y)
    es = abs(np.cos(y)) * ey + 0.5 * ey * ey
    es += ULP * (abs(s) + es)
    q = s / y
    eq = (es + abs(q) * ey) / (y - ey)
    eq += U * (abs(q) + eq)
    if x - ex < small:
        eq += abs(1.0 - q)
    return q, eq


def sinc_1d(x, ex, r, tau, beyond=False):
    """SincFilter::windowed_sinc (sinc.rs:25-33): 0 beyond the radius (`beyond`, an exact float32 decision made by the caller), else
    sinc(x) * sinc(x / tau).  The division by tau and the product round once each."""
    if beyond:
        return 0.0, 0.0
    x = abs(x)
    s, es = _sinc(x, ex)
    xt = x / tau
    w, ew = _sinc(xt, ex / tau + U * xt)
    return s * w, abs(s) * ew + abs(w) * es + es * ew + U * abs(s * w)


def filter_table(kind, xwidth, ywidth, **kw):
    """Film::new's table (film.rs:102-120): table[y * 16 + x] = evaluate(x * (rx / 15), y * (ry / 15)), with the parameters as the
    float32 numbers the scene description carries.  Returns (table, bound), both (256,) float64; bound[i] limits a float32 evaluation
    of entry i: the division r / 15 and the product x * (r / 15) round once each (2 u on the argument), then the filter's own count,
    then the product of the two factors."""
    rx, ry = c32(xwidth), c32(ywidth)
    kw = {k: c32(v) for k, v in kw.items()}
    f = {"box": box_1d, "triangle": triangle_1d, "gaussian": gaussian_1d, "mitchell": mitchell_1d, "sinc": sinc_1d}[kind]
    one = []
    for r in (rx, ry):
        col = []
        for i in range(FT_W):
            x = i * r / (FT_W - 1)
            ex = gamma(2) * x
            extra = {}
            if kind == "sinc":          # `x > radius` on the float32 argument, exactly as film.rs:114 computes it
                x32 = np.float32(i) * (np.float32(r) / np.float32(FT_W - 1))
                extra["beyond"] = bool(x32 > np.float32(r))
            col.append(f(x, ex, r, **kw, **extra))
        one.append(col)
    tab, bnd = np.empty(FT_W * FT_W), np.empty(FT_W * FT_W)
    for y in range(FT_W):
        for x in range(FT_W):
            (gx, bx), (gy, by) = one[0][x], one[1][y]
            tab[y * FT_W + x] = gx * gy
            bnd[y * FT_W + x] = abs(gy) * bx + abs(gx) * by + bx * by + U * (abs(gx * gy) + abs(gy) * bx + abs(gx) * by + bx * by)
    if kind == "box":          # a literal 1.0, no product (box_filter.rs:18-20)
        bnd[:] = 0.0
    return tab, bnd


# ---------------------------------------------------------------------------------------------------------------- crop and sample bounds
def film_bounds(xres, yres, crop_window, radius):
    """Film::new's cropped pixel bounds (film.rs:73-90: floor on both minima, ceil on the maxima, clamped to the resolution) and
    get_sample_bounds (film.rs:166-179), exactly in np.float32.  crop_window = (x0, x1, y0, y1) as the scene description orders it.
    Returns (cropped (x0, y0, x1, y1), sample_bounds (x0, y0, x1, y1), undecided): undecided lists the crop products that lie within
    1 ulp of an integer and whose floor (minima) or ceil (maxima) the exact product decides the other way: there an evaluation in another
    precision gives another film.  The float32 answer is the reference's and is what is returned."""
    f = np.float32
    res = (int(xres), int(yres))
    cw = [f(v) for v in crop_window]
    und, prod = [], {}
    for name, axis, v in (("x0", 0, cw[0]), ("x1", 0, cw[1]), ("y0", 1, cw[2]), ("y1", 1, cw[3])):
        p = f(res[axis]) * v
        prod[name] = p
        exact = float(f(res[axis])) * float(v)          # 24 x 24 bits: exact in float64
        rnd = np.floor if name in ("x0", "y0") else np.ceil
        if abs(float(p) - np.rint(float(p))) <= float(np.spacing(p)) and rnd(exact) != rnd(float(p)):
            und.append(name)
    x0 = max(0, int(np.floor(prod["x0"]))); y0 = max(0, int(np.floor(prod["y0"])))
    x1 = min(int(np.ceil(prod["x1"])), res[0]); y1 = min(int(np.ceil(prod["y1"])), res[1])
    rx, ry = f(radius[0]), f(radius[1])
    sb = (int(np.floor(f(x0) - rx)), int(np.floor(f(y0) - ry)), int(np.ceil(f(x1) + rx)), int(np.ceil(f(y1) + ry)))
    return (x0, y0, x1, y1), sb, und


# ---------------------------------------------------------------------------------------------------------------- the radiance guard
def validate_radiance(l):
    """validate_radiance_result (sampler.rs:151-176): black where a component is not finite (is_valid), where the luminance is below
    -1e-5 or infinite.  The comparisons are decisions: the luminance is formed in np.float32 as rgb.rs:60-63 writes it."""
    l = np.asarray(l, np.float32).reshape(-1, 3)
    yw = YWEIGHT.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (yw[0] * l[:, 0] + yw[1] * l[:, 1]) + yw[2] * l[:, 2]
        bad = ~np.isfinite(l).all(axis=1) | (y < np.float32(-1e-5)) | np.isinf(y)
    out = l.copy()
    out[bad] = 0.0
    return out


# ---------------------------------------------------------------------------------------------------------------- add_sample_filter
def _axis(p, r, lo, hi):
    """One axis of the footprint for every sample (film_tile.rs:95-132): the pixels floor(p - r) .. ceil(p + r) clipped to [lo, hi), and for
    each its table index, min(floor(d * (1 / r) * 15), 15) with d = |x + 0.5 - p|, or -1 where d > r.  Returns (x, idx, alts): x (n, W)
    pixel coordinates, idx the index in real arithmetic (-2 outside the footprint), alts two arrays of indices a float32 chain may
    arrive at instead (equal to idx where the decision is safe).  A footprint that rounding makes one pixel wider or narrower changes
    nothing: that pixel's centre is farther than r."""
    p = np.asarray(p, np.float32).astype(np.float64)
    r32 = np.float32(r); r = float(r32)
    last = FT_W - 1
    p0 = np.maximum(np.floor(p - r), lo).astype(np.int64)
    p1 = np.minimum(np.ceil(p + r), hi).astype(np.int64)
    W = int(max(1, (p1 - p0).max())) if len(p) else 1
    x = p0[:, None] + np.arange(W)[None, :]
    inside = x < p1[:, None]
    d = np.abs(x + 0.5 - p[:, None])                        # exact in float64
    d32 = d.astype(np.float32)                              # what a correctly rounded f32 subtraction gives
    lx32 = (np.float32(1.0) / r32) * np.float32(last)
    t = d * (last / r)
    t32 = d32 * lx32                                        # the float32 product
    idx = np.where(d <= r, np.minimum(np.floor(t), last).astype(np.int64), -1)
    i32 = np.where(d32 <= r32, np.minimum(np.floor(t32.astype(np.float64)), last).astype(np.int64), -1)
    # `d <= r`: d rounds once.  On the edge t is 15 to a rounding, so the index is 14 or 15 if there is one.
    edge = ((d32.astype(np.float64) != d) & (np.abs(d - r) <= U * d)) | ((i32 < 0) != (idx < 0))
    # the index: d, 1 / r, (1 / r) * 15 and d * lx round once each
    k = np.rint(t)
    near = (t32.astype(np.float64) != t) & (np.abs(t - k) <= gamma(4) * t) & (k >= 1) & (k <= last) & (idx >= 0)
    other = np.minimum(np.where(np.floor(t) == k, k - 1, k), last).astype(np.int64)
    alt1 = np.where(edge, np.where(idx < 0, last, -1), np.where(near, other, idx))
    alt2 = np.where(edge, np.where(idx < 0, last - 1, np.where(near, other, idx)), idx)
    alt2 = np.where((i32 != idx) & (i32 != alt1), i32, alt2)            # what the float32 chain itself decides is never left uncovered
    return x, np.where(inside, idx, -2), [np.where(inside, a, -2) for a in (alt1, alt2)]


def add_samples(p_film, radiance, table, radius, cropped, max_sample_luminance=np.inf, repeat=1, chunk=32768):
    """FilmTile::add_sample_filter (film_tile.rs:84-183) for every sample, then Film::merge_film_tile (film.rs:219-241), summed in float64.

    p_film (n, 2) and radiance (n, 3) float32 as the caller has them (radiance after validate_radiance), table (256,) float32, radius
    (rx, ry), cropped (x0, y0, x1, y1).  `repeat` renders the same samples that many times into one film.

    Per sample: the luminance clamp first (l *= max / l.y() where l.y() > max), the footprint clipped to the crop, the weights read
    from the table, their row-major sum, return where sum <= 0, weights * (1 / sum), contrib += l * 1 * w and weight += w.
    Returns a dict: xyz (H, W, 3), weight (H, W), their bounds b_xyz, b_weight; count (contributions per pixel), n_contributing (samples
    with a non-empty footprint and sum > 0), n_clamped, and per sample `contributes`, `clamped`."""
    p_film = np.asarray(p_film, np.float32).reshape(-1, 2)
    radiance = np.asarray(radiance, np.float32).reshape(-1, 3)
    T = np.asarray(table, np.float32).astype(np.float64).reshape(FT_W, FT_W)
    n = len(p_film)
    cx0, cy0, cx1, cy1 = [int(v) for v in cropped]
    Hf, Wf = cy1 - cy0, cx1 - cx0
    npix = Hf * Wf
    acc = {k: np.zeros((npix, 3)) for k in ("rgb", "rgb_mag", "rgb_err")}
    acc.update({k: np.zeros(npix) for k in ("wt", "wt_mag", "wt_err", "cnt")})
    bad = np.zeros(npix, bool)
    contributes = np.zeros(n, bool); clamped_all = np.zeros(n, bool)
    n_steps = n_lost = 0
    mx = float(np.float32(max_sample_luminance))

    def look(jy, jx):
        ok = (jy[:, :, None] >= 0) & (jx[:, None, :] >= 0)
        return np.where(ok, T[np.maximum(jy, 0)[:, :, None], np.maximum(jx, 0)[:, None, :]], 0.0)

    for c0 in range(0, n, chunk):
        sl = slice(c0, min(n, c0 + chunk))
        L = radiance[sl].astype(np.float64)
        m = len(L)
        # ---- the clamp (film_tile.rs:86-89).  l.y(): three products, two sums; max / y and l * that round once each.  Continuous at
        # the threshold, so a luminance within its error of the clamp adds nothing beyond the clamped branch's own error.
        y = L @ YWEIGHT
        ey = gamma(3) * (np.abs(L) @ YWEIGHT)
        clamped = y > mx
        maybe = (y + ey > mx) & np.isfinite(mx)
        scale = np.where(clamped, mx / np.where(clamped, y, 1.0), 1.0)
        rel_l = np.where(maybe, (1.0 + gamma(2)) / (1.0 - np.minimum(ey / np.maximum(np.abs(y), 1e-300), 0.5)) - 1.0, 0.0)
        Lc = L * scale[:, None]
        clamped_all[sl] = clamped

        # ---- footprint and weights (film_tile.rs:95-160)
        xs, ix, ax = _axis(p_film[sl, 0], radius[0], cx0, cx1)
        ys, iy, ay = _axis(p_film[sl, 1], radius[1], cy0, cy1)
        Wt = look(iy, ix)                                                        # (m, Wy, Wx)
        in_fp = (iy[:, :, None] > -2) & (ix[:, None, :] > -2)
        dT = np.zeros_like(Wt)
        for jy in [iy] + ay:
            for jx in [ix] + ax:
                if jy is iy and jx is ix:
                    continue
                if np.array_equal(jy, iy) and np.array_equal(jx, ix):
                    continue
                dT = np.maximum(dT, np.abs(look(jy, jx) - Wt))
        dT = np.where(in_fp, dT, 0.0)
        npx = in_fp.sum(axis=(1, 2))
        S = Wt.sum(axis=(1, 2))
        A = np.abs(Wt).sum(axis=(1, 2))
        dS = dT.sum(axis=(1, 2))
        nnz = ((Wt != 0.0) | (dT > 0.0)).sum(axis=(1, 2))
        eS = gamma(np.maximum(nnz - 1, 0)) * A                                     # the f32 sum, any order; adding a zero is exact
        contrib = (npx > 0) & (S > 0)
        contributes[sl] = contrib
        # `sum <= 0` undecided, or a step large enough to bring the sum to zero: nothing can be said about this footprint
        lost = (npx > 0) & (eS + dS > 0) & (np.abs(S) <= eS + dS)
        Ssafe = np.where(contrib, S, 1.0)
        w = np.where(contrib[:, None, None], Wt / Ssafe[:, None, None], 0.0)
        denom = np.maximum(np.abs(Ssafe) - eS - dS, 1e-300)
        rel_w = (1.0 + gamma(2)) * np.abs(Ssafe) / np.maximum(np.abs(Ssafe) - eS, 1e-300) - 1.0      # 1 / sum and w * isum round once each
        # a step of dT in one weight moves that weight by dT / sum and every weight by |w| dS / sum
        step_w = np.where(contrib[:, None, None] & in_fp, (dT + np.abs(w) * dS[:, None, None]) / denom[:, None, None], 0.0)
        err_w = np.abs(w) * rel_w[:, None, None] + step_w                          # |w_f32 - w|
        rel_c = (1.0 + rel_l) * (1.0 + U) - 1.0                                    # (l * 1) * w: one rounding per channel
        absL = np.abs(Lc)

        pix = (ys - cy0)[:, :, None] * Wf + (xs - cx0)[:, None, :]                  # (m, Wy, Wx) film index
        use = in_fp & contrib[:, None, None] & ((Wt != 0.0) | (step_w > 0.0))
        fi = pix[use]
        sidx = np.broadcast_to(np.arange(m)[:, None, None], pix.shape)[use]
        wv, ew = w[use], err_w[use]

        def add(name, vals, c=None):
            s = np.bincount(fi, weights=vals, minlength=npix)
            if c is None:
                acc[name] += s
            else:
                acc[name][:, c] += s
        for c in range(3):
            term = Lc[sidx, c] * wv
            e = np.abs(term) * rel_c[sidx] + absL[sidx, c] * ew * (1.0 + rel_c[sidx])
            add("rgb", term, c); add("rgb_err", e, c); add("rgb_mag", np.abs(term) + e, c)
        add("wt", wv); add("wt_err", ew); add("wt_mag", np.abs(wv) + ew); add("cnt", np.ones(len(fi)))
        bad[pix[lost[:, None, None] & in_fp]] = True
        n_steps += int(((dT > 0) & in_fp).sum()); n_lost += int(lost.sum())

    k = float(repeat)
    rgb, rgb_mag, rgb_err = acc["rgb"] * k, acc["rgb_mag"] * k, acc["rgb_err"] * k
    wt, wt_mag, wt_err, cnt = acc["wt"] * k, acc["wt_mag"] * k, acc["wt_err"] * k, acc["cnt"] * k
    # ---- accumulation and merge (film_tile.rs:179-180, film.rs:232-237).  A term goes through at most cnt - 1 additions whatever the
    # grouping (per tile, then per film; or own / spill), then through one product and two sums of the colour matrix, and one more sum
    # where two partial films are added: gamma(cnt + 3) on the sum of |terms|.
    g = gamma(cnt + 3.0)
    xyz = rgb @ RGB2XYZ.T
    b_xyz = (rgb_err + g[:, None] * rgb_mag) @ np.abs(RGB2XYZ).T
    b_w = wt_err + gamma(cnt) * wt_mag
    b_xyz[bad] = np.inf; b_w[bad] = np.inf
    return {"xyz": xyz.reshape(Hf, Wf, 3), "weight": wt.reshape(Hf, Wf), "b_xyz": b_xyz.reshape(Hf, Wf, 3), "b_weight": b_w.reshape(Hf, Wf),
            "count": cnt.reshape(Hf, Wf), "n_contributing": int(contributes.sum()), "contributes": contributes, "clamped": clamped_all,
            "n_clamped": int(clamped_all.sum()), "n_samples": n, "n_steps": n_steps, "n_lost": n_lost}


def scaled(film, k):
    """The same film with every sum multiplied by the power of two k (an exact operation in float32): values and bounds scale."""
    out = dict(film)
    for key in ("xyz", "weight", "b_xyz", "b_weight"):
        out[key] = film[key] * float(k)
    return out


def resolve(film, scale=1.0):
    """Film::write_image (film.rs:440-484) on the truth of add_samples: XYZ -> RGB, divided by the weight only where it is > 0, max(0, .),
    then the film scale.  Adds to the dict: rgb, b_rgb (H, W, 3) and left_out (H, W).

    b_rgb: the XYZ bounds through |matrix|, the matrix's own three roundings on the magnitudes, then c * (1 / w): the reciprocal, the product
    and the scale round once each, and the weight's bound enters as b_w / |w| -- the conditioning where negative lobes cancel.
    left_out: a bound above 1e-3 of the largest |value| of its quantity over the film, or a weight within its bound of 0 (the `> 0` of
    write_image is then undecided)."""
    xyz, w, b_xyz, b_w = film["xyz"], film["weight"], film["b_xyz"], film["b_weight"]
    s = c32(scale)
    c = xyz @ XYZ2RGB.T
    cmag = np.abs(xyz) @ np.abs(XYZ2RGB).T
    with np.errstate(invalid="ignore"):
        b_c = b_xyz @ np.abs(XYZ2RGB).T
        b_c = b_c + gamma(3) * (cmag + b_c)
    undecided = (b_w > 0) & (np.abs(w) <= b_w)
    pos = (w > 0) & ~undecided
    wsafe = np.where(pos, w, 1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = (1.0 + gamma(3)) / (1.0 - np.minimum(np.where(pos, b_w / wsafe, 0.0), 0.5)) - 1.0
        q = np.where(pos[..., None], np.maximum(0.0, c / wsafe[..., None]), c)
        b_q = np.where(pos[..., None], (np.abs(c) * rel[..., None] + b_c * (1.0 + rel[..., None])) / wsafe[..., None], b_c + U * (np.abs(c) + b_c))
    rgb = q * s
    b_rgb = b_q * abs(s)
    b_rgb[undecided] = np.inf

    def over(b, v):
        fin = np.isfinite(v)
        top = np.abs(v[fin]).max() if fin.any() else 0.0
        with np.errstate(invalid="ignore"):
            m = ~(b <= LEAVE_OUT * top)
        m &= b > 0
        return m if m.ndim == 2 else m.any(axis=-1)
    left = undecided | over(b_xyz, xyz) | over(b_w, w) | over(b_rgb, rgb)
    out = dict(film)
    out.update(rgb=rgb, b_rgb=b_rgb, left_out=left, scale=s)
    return out


def film_truth(p_film, radiance, table, radius, cropped, max_sample_luminance=np.inf, scale=1.0, repeat=1):
    """add_samples followed by resolve."""
    return resolve(add_samples(p_film, radiance, table, radius, cropped, max_sample_luminance, repeat), scale)


def compare(truth, xyzw, rgb=None):
    """A film {X, Y, Z, weight} (H, W, 4) and its resolved RGB against a truth: the largest err / bound per quantity outside the left-out
    pixels (0 / 0 counts as 0: an exact zero is a pass), and the left-out share.  Returns a dict; `ok` says every quantity holds."""
    keep = ~truth["left_out"]
    out = {"left_out": float(truth["left_out"].mean())}

    def ratio(got, want, bound):
        err = np.abs(np.asarray(got, np.float64) - want)[keep]
        b = bound[keep]
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err == 0, 0.0, err / b)
        r = np.where(np.isnan(r), np.inf, r)
        return float(r.max()) if r.size else 0.0
    out["xyz"] = ratio(xyzw[..., :3], truth["xyz"], truth["b_xyz"])
    out["weight"] = ratio(xyzw[..., 3], truth["weight"], truth["b_weight"])
    out["rgb"] = ratio(rgb, truth["rgb"], truth["b_rgb"]) if rgb is not None else 0.0
    out["worst"] = max(out["xyz"], out["weight"], out["rgb"])
    out["ok"] = out["worst"] <= 1.0
    return out
