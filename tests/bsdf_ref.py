"""Restatement of the BSDF layer in numpy, parameterised by dtype: Material::compute_scattering_functions of the eight materials of the
accelerated path, the BxDFs behind them, and BSDF::f / pdf / sample_f on the canonical frame ns = ng = (0,0,1), ss = (1,0,0).  Written
from the reference's text; independent of the oracle and of the product (it imports neither).

Run in float64 it is the truth the oracle and the device are held to; run in float32 it is the reference's arithmetic without either
(the calibration of test_bsdf_truth_oracle.py).  It starts from the material's PARAMETERS as the scene description carries them, not
from lobe records, so the material-to-lobe translation is under test as well.

What is restated (file:line of the reference)
  * core/reflection/math.rs:5-111         cos / sin / tan / phi helpers, reflect, refract, same_hemisphere
  * core/reflection/fresnel.rs:16-42      fr_dielectric;  :45-82 fr_conductor;  :100-122 the Fresnel objects;  :150-216 FresnelSpecular
  * core/reflection/lambertian.rs:16-47   LambertianReflection;  :59-86 LambertianTransmission (Q53: its pdf has no INV_PI)
  * core/reflection/bxdf.rs:74-94         the default sample_f (cosine_sample_hemisphere, core/sampling/sampling.rs:114-159) and pdf
  * core/reflection/oren_nayar.rs:17-49   OrenNayar::new and f
  * core/reflection/specular.rs:26-38     SpecularReflection::sample_f;  :78-107 SpecularTransmission::sample_f
  * core/reflection/microfacet.rs:29-103  MicrofacetReflection;  :143-254 MicrofacetTransmission (Q19: pdf without the wo . wh < 0 guard)
  * core/reflection/fresnel_blend.rs:13-104   FresnelBlend (pow5 is powf(v, 5))
  * core/distribution/trowbridge_reitz.rs:6-93 sample_11 and the stretch / rotate / unstretch;  :103-121 new, roughness_to_alpha;
    :153-179 d, lambda;  :181-221 sample_wh (samplevis) and pdf;  core/distribution/microfacet.rs:6-11 g1, g
  * core/reflection/bsdf.rs:92-206        sample_f: component choice, the remapped u, the pdf averaged over the matching lobes, f re-summed
    for a non-specular pick;  :208-236 f;  :238-270 pdf
  * materials/matte.rs:37-51  plastic.rs:43-69  mirror.rs:30-39  glass.rs:58-108  metal.rs:62-83  uber.rs:75-125  substrate.rs:46-66
    translucent.rs:48-106 (Q54: no BSDF for black reflect and transmit; Q55: eta is 1.5; Q56: one roughness for both glossy lobes)

It restates the reference, not physics: Q19, Q53, Q55, Q56 are carried as they are.  The reference's constants (PI, INV_PI, 0.9999, 1e-4,
the polynomial coefficients, ...) are the float32 numbers it holds; the truth is exact arithmetic on them.

Bounds.  Every quantity is aov_ref's E: a value in the run's dtype and a float64 bound on the distance of a float32 evaluation of the same
expression from its exact value -- first-order propagation, plus one float32 rounding (2^-24 |value|) per operation, accumulated as
evaluated, so the cancelling steps (1 - cos^2, tan^2 = sin^2 / cos^2, 1 / (4 cos_i cos_o), 1 / |cos|, sqrt_denom^2, the conductor's t0,
a a - 1 and the dd radicand of sample_11) carry their conditioning into the result.  ln, sin, cos add LIBM_ULP = 2 ulp; powf(x, 5) is
x ** 5 with POW_ULP = 2 ulp (glibc documents powf below 1 ulp; the second is the result's own rounding).  No constant is fitted.

A branch whose condition lies within its bound of its threshold makes the evaluation undecided (`und`), see decide().  The rules, as the
reference's text has them: the sign of wo.z wi.z (same_hemisphere, `reflect`); wo . wh < 0; wo_wh wi_wh > 0; sin2_theta_t >= 1 (refract)
and sin_theta_t >= 1 (fr_dielectric); the side the Fresnel term is entered from (cos > 0, the sign of wh.z under face_forward);
Oren-Nayar's sin > 1e-4; isinf(tan^2); the lobe index floor(u.x matching); u.x < fr of FresnelSpecular; u.x < 0.5 of FresnelBlend;
cos_t > 0.9999; the slope selection a < 0 || slope_x_2 > 1 / tan_t; u2 > 0.5; pdf > 0 where sample_f returns None on it.
"""
import numpy as np

from aov_ref import E, U, where, cos as ecos, sin as esin, vadd, vscale, vneg, vdot, vnorm, vwhere

F = np.float32
REFL, TRANS, DIFFUSE, GLOSSY, SPECULAR = 1, 2, 4, 8, 16
ALL, NOSPEC, REFL_ONLY = 31, 31 & ~16, 1 | 4 | 8 | 16
LIBM_ULP, POW_ULP = 2.0, 2.0
TINY = 2.0 ** -126            # below this a float32 product has underflowed: a sign read from it is not the float64 product's sign
REL_CAP = 1e-3                # a bound past this share of its value leaves the evaluation out (the line the texture truths use)


def c32(x):
    """A literal of the reference as the float32 number it holds."""
    return float(F(x))


PI, INV_PI, PI_OVER_2, PI_OVER_4 = c32(np.pi), c32(1 / np.pi), c32(np.pi / 2), c32(np.pi / 4)
ONE_MINUS_EPSILON = float(F(1) - F(2.0 ** -24))


def decide(x, und, thr=0.0):
    """A comparison of x against thr is undecided within x's bound; a product compared against 0 also where float32 underflows."""
    d = np.abs(x.v.astype(np.float64) - thr)
    und |= ((d <= x.e) & (x.e > 0)) | ((d <= TINY) if thr == 0.0 else False) | ~np.isfinite(x.e)


def emax(a, lo):
    return E(np.maximum(a.v, np.asarray(lo, a.v.dtype)), a.e)


def emin(a, hi):
    return E(np.minimum(a.v, np.asarray(hi, a.v.dtype)), a.e)


def eclamp(a, lo, hi):
    return E(np.clip(a.v, np.asarray(lo, a.v.dtype), np.asarray(hi, a.v.dtype)), a.e)


def emax2(a, b):
    return where(a.v > b.v, a, b)


def elog(a):
    with np.errstate(all="ignore"):
        v = np.log(a.v)
        return E(v, a.e / np.abs(a.v.astype(np.float64)) + LIBM_ULP * U * np.abs(v.astype(np.float64)))


def pow5(a):
    """fresnel_blend.rs:13-15: powf(v, 5)."""
    v = a.v ** 5
    return E(v, 5.0 * np.abs(a.v.astype(np.float64)) ** 4 * a.e + POW_ULP * U * np.abs(v.astype(np.float64)))


def zeros_like(a):
    return E(np.zeros(a.v.shape, a.v.dtype))


def full_like(a, x):
    return E(np.full(a.v.shape, x, a.v.dtype))


def bcast(x, like):
    """A per-material scalar as a per-evaluation quantity (no operation, no rounding)."""
    return E(np.broadcast_to(x.v, like.v.shape).copy(), np.broadcast_to(x.e, like.v.shape))


def rgb_where(m, a, b):
    return [where(m, a[i], b[i]) for i in range(3)]


def vexact(a, dt):
    a = np.asarray(a, np.float32)
    return [E(a[:, i].astype(dt)) for i in range(3)]


# ------------------------------------------------------------------------------------------------------------------ reflection/math.rs
def cos2_theta(w): return w[2] * w[2]                                  # :10-12
def sin2_theta(w): return emax(1.0 - cos2_theta(w), 0.0)               # :20-22
def sin_theta(w): return sin2_theta(w).sqrt()                          # :25-27
def tan_theta(w): return sin_theta(w) / w[2]                           # :30-32
def tan2_theta(w): return sin2_theta(w) / cos2_theta(w)                # :35-37


def cos_phi(w):                                                        # :40-47
    s = sin_theta(w)
    return where(s.v == 0, full_like(s, 1.0), eclamp(w[0] / s, -1.0, 1.0))


def sin_phi(w):                                                        # :50-57
    s = sin_theta(w)
    return where(s.v == 0, zeros_like(s), eclamp(w[1] / s, -1.0, 1.0))


def reflect(wo, n):                                                    # :84-88
    d = 2.0 * vdot(wo, n)
    return [d * n[i] + (-wo[i]) for i in range(3)]


def refract(wi, n, eta, und):                                          # :91-106 -> (wt, refracted)
    cos_i = vdot(n, wi)
    sin2_i = emax(1.0 - cos_i * cos_i, 0.0)
    sin2_t = eta * eta * sin2_i
    decide(sin2_t, und, 1.0)
    ok = ~(sin2_t.v >= 1.0)
    cos_t = (1.0 - sin2_t).sqrt()
    k = eta * cos_i - cos_t
    return [eta * (-wi[i]) + k * n[i] for i in range(3)], ok


def same_hemisphere(w, wp, und):                                       # :109-111
    p = w[2] * wp[2]
    decide(p, und)
    return p.v > 0


# ------------------------------------------------------------------------------------------------------------------ fresnel.rs
def fr_dielectric(cos_i, eta_i, eta_t, und):                           # :16-42; eta_i, eta_t: E scalars
    cos_i = eclamp(cos_i, -1.0, 1.0)
    decide(cos_i, und)
    entering = cos_i.v > 0
    ei, et = where(entering, eta_i, eta_t), where(entering, eta_t, eta_i)
    cos_i = cos_i.abs()
    sin_i = emax(1.0 - cos_i * cos_i, 0.0).sqrt()
    sin_t = ei / et * sin_i
    decide(sin_t, und, 1.0)
    tir = sin_t.v >= 1.0
    cos_t = emax(1.0 - sin_t * sin_t, 0.0).sqrt()
    rparl = ((et * cos_i) - (ei * cos_t)) / ((et * cos_i) + (ei * cos_t))
    rperp = ((ei * cos_i) - (et * cos_t)) / ((ei * cos_i) + (et * cos_t))
    r = (rparl * rparl + rperp * rperp) / 2.0
    return where(tir, full_like(r, 1.0), r)


def fr_conductor(cos_i, eta_i, eta_t, k):                              # :45-82, per channel
    cos_i = eclamp(cos_i, -1.0, 1.0)
    c2 = cos_i * cos_i
    s2 = 1.0 - c2
    s22 = s2 * s2
    out = []
    for ch in range(3):
        eta = eta_t[ch] / eta_i[ch]
        etak = k[ch] / eta_i[ch]
        eta2, etak2 = eta * eta, etak * etak
        t0 = eta2 - etak2 - s2
        a2plusb2 = (t0 * t0 + eta2 * etak2 * 4.0).sqrt()
        t1 = a2plusb2 + c2
        a = ((a2plusb2 + t0) * 0.5).sqrt()
        t2 = cos_i * a * 2.0
        rs = (t1 - t2) / (t1 + t2)
        t3 = c2 * a2plusb2 + s22
        t4 = t2 * s2
        rp = rs * (t3 - t4) / (t3 + t4)
        out.append((rp + rs) * 0.5)
    return out


# ------------------------------------------------------------------------------------------------------------------ trowbridge_reitz.rs
def roughness_to_alpha(r, dt):                                         # :113-121
    x = elog(emax(r, c32(1e-3)))
    k = [E(np.asarray(c32(c), dt)) for c in (1.62142, 0.819955, 0.1734, 0.0171201, 0.000640711)]
    return k[0] + k[1] * x + k[2] * x * x + k[3] * x * x * x + k[4] * x * x * x * x


class TR:
    def __init__(self, ax, ay):                                        # :103-111
        self.ax, self.ay = emax(ax, c32(0.001)), emax(ay, c32(0.001))

    def d(self, wh, und):                                              # :153-166
        t2 = tan2_theta(wh)
        c2 = cos2_theta(wh)
        und |= c2.v.astype(np.float64) <= 4.0 * TINY                   # isinf(tan^2): only where float32 cos^2 leaves the normal range
        inf = np.isinf(t2.v)
        cos4 = c2 * c2
        cp, sp = cos_phi(wh), sin_phi(wh)
        e = ((cp * cp) / (self.ax * self.ax) + (sp * sp) / (self.ay * self.ay)) * t2
        e2 = (1.0 + e) * (1.0 + e)
        d = 1.0 / (PI * self.ax * self.ay * cos4 * e2)
        return where(inf, zeros_like(d), d)

    def lam(self, w, und):                                             # :168-179
        at = tan_theta(w).abs()
        inf = np.isinf(at.v)
        cp, sp = cos_phi(w), sin_phi(w)
        alpha = ((cp * cp) * self.ax * self.ax + (sp * sp) * self.ay * self.ay).sqrt()
        a2t2 = (alpha * at) * (alpha * at)
        lam = (-1.0 + (1.0 + a2t2).sqrt()) / 2.0
        return where(inf, zeros_like(lam), lam)

    def g1(self, w, und): return 1.0 / (1.0 + self.lam(w, und))        # microfacet.rs:6-8
    def g(self, wo, wi, und): return 1.0 / (1.0 + self.lam(wo, und) + self.lam(wi, und))      # :9-11

    def pdf(self, wo, wh, und):                                        # :215-217 (samplevis)
        return self.d(wh, und) * self.g1(wo, und) * vdot(wo, wh).abs() / wo[2].abs()

    def sample_wh(self, wo, u1, u2, und):                              # :181-213 (samplevis), :64-93
        flip = wo[2].v < 0                                             # wo is an exact input: its sign is decided
        wo = vwhere(flip, vneg(wo), wo)
        ws = vnorm([self.ax * wo[0], self.ay * wo[1], wo[2]])
        sx, sy = sample_11(ws[2], u1, u2, und)
        cp, sp = cos_phi(ws), sin_phi(ws)
        tmp = cp * sx - sp * sy
        sy = sp * sx + cp * sy
        sx = tmp * self.ax
        sy = sy * self.ay
        wh = vnorm([-sx, -sy, full_like(sx, 1.0)])
        return vwhere(flip, vneg(wh), wh)


def _slopes_plain(cos_t, u1, eps, xp=np):
    """trowbridge_reitz.rs:18-35 as plain arithmetic; every operation's result is multiplied by the next factor of `eps`."""
    k = iter(eps)

    def r(x):
        return x * next(k)
    sin_t = r(xp.sqrt(xp.maximum(0.0, r(1.0 - r(cos_t * cos_t)))))
    tan_t = r(sin_t / cos_t)
    a = r(1.0 / tan_t)
    g1 = r(2.0 / r(1.0 + r(xp.sqrt(r(1.0 + r(1.0 / r(a * a)))))))
    a = r(r(2.0 * u1 / g1) - 1.0)                                      # (2 u1 is exact)
    tmp = xp.minimum(1e10, r(1.0 / r(r(a * a) - 1.0)))
    b = tan_t
    rad = r(r(r(r(b * b) * tmp) * tmp) - r(r(r(a * a) - r(b * b)) * tmp))
    d = r(xp.sqrt(xp.maximum(rad, 0.0)))
    bt = r(b * tmp)                                                    # (the reference multiplies twice: the same value, one rounding)
    return a, r(bt - d), r(bt + d), r(1.0 / tan_t), rad


def _count_slope_ops():
    n = [0]

    def ones():
        while True:
            n[0] += 1
            yield 1.0
    _slopes_plain(np.array([0.5]), np.array([0.3]), ones())
    return n[0]


N_SLOPE_OPS = _count_slope_ops()


def _slopes(cos_t, u1):
    """a, slope_x_1, slope_x_2, 1 / tan_t and the dd radicand of sample_11 with first-order bounds that keep the CORRELATION between the
    steps: slope_x_2 = b tmp + dd cancels for a near 1, and its sensitivity to tmp's own rounding cancels with it, which step-by-step
    propagation cannot see.  The bound of an output is the sum over the operations of |its change when that operation's result moves
    by one float32 rounding (a factor 1 + 2^-24)|, plus |its change when an input moves by the input's bound|: the same first-order
    model as E, one rounding per operation, with the sensitivities taken by differences in float64."""
    dt = cos_t.v.dtype
    with np.errstate(all="ignore"):
        ones = [1.0] * N_SLOPE_OPS
        vals = _slopes_plain(cos_t.v, u1.v, [dt.type(1.0)] * N_SLOPE_OPS)             # the run's own arithmetic
        c64, u64 = cos_t.v.astype(np.float64), u1.v.astype(np.float64)
        base = _slopes_plain(c64, u64, ones)
        bound = [np.zeros(len(c64)) for _ in base]
        for k in range(N_SLOPE_OPS):
            eps = list(ones)
            eps[k] = 1.0 + U
            for o, (p, q) in enumerate(zip(_slopes_plain(c64, u64, eps), base)):
                bound[o] += np.abs(p - q)
        for dc, du in ((cos_t.e, 0.0), (0.0, u1.e)):
            for o, (p, q) in enumerate(zip(_slopes_plain(c64 + dc, u64 + du, ones), base)):
                bound[o] += np.abs(p - q)
    return [E(v, e) for v, e in zip(vals, bound)]


def sample_11(cos_t, u1, u2, und):                                     # :6-62
    dt = cos_t.v.dtype
    decide(cos_t - c32(0.9999), und)
    normal = cos_t.v > np.asarray(c32(0.9999), dt)
    with np.errstate(all="ignore"):
        r = (u1 / (1.0 - u1)).sqrt()
        phi = 2.0 * PI * u2
        nx, ny = r * ecos(phi), r * esin(phi)
        a, s1, s2, inv_tan, rad = _slopes(cos_t, u1)
        decide(rad, und_rad := np.zeros(len(normal), bool))
        und |= ~normal & und_rad
        ua, us = np.zeros(len(normal), bool), np.zeros(len(normal), bool)
        decide(a, ua)
        decide(s2 - inv_tan, us)
        first = (a.v < 0) | (s2.v > inv_tan.v)
        und |= ~normal & (ua | (~(a.v < 0) & us))
        slope_x = where(first, s1, s2)
        uu = np.zeros(len(normal), bool)
        decide(u2 - 0.5, uu)
        und |= ~normal & uu
        up = u2.v > np.asarray(0.5, dt)
        s = np.where(up, 1.0, -1.0).astype(dt)
        v2 = where(up, 2.0 * (u2 - 0.5), 2.0 * (0.5 - u2))
        k = [c32(c) for c in (0.27385, 0.73369, 0.46341, 0.093073, 0.309420, 1.000000, 0.597999)]
        z = (v2 * (v2 * (v2 * k[0] - k[1]) + k[2])) / (v2 * (v2 * (v2 * k[3] + k[4]) - k[5]) + k[6])
        slope_y = E(s) * z * (1.0 + slope_x * slope_x).sqrt()
    return where(normal, nx, slope_x), where(normal, ny, slope_y)


# ------------------------------------------------------------------------------------------------------------------ sampling.rs
def cosine_sample_hemisphere(u1, u2):                                  # :114-133, :155-159
    ox, oy = u1 * 2.0 - 1.0, u2 * 2.0 - 1.0
    zero = (ox.v == 0) & (oy.v == 0)
    with np.errstate(all="ignore"):
        xa = np.abs(ox.v) > np.abs(oy.v)
        t1 = PI_OVER_4 * (oy / ox)
        t2 = PI_OVER_2 - PI_OVER_4 * (ox / oy)
        r, th = where(xa, ox, oy), where(xa, t1, t2)
        dx, dy = r * ecos(th), r * esin(th)
    dx, dy = where(zero, zeros_like(dx), dx), where(zero, zeros_like(dy), dy)
    z = emax(1.0 - dx * dx - dy * dy, 0.0).sqrt()
    return [dx, dy, z]


# ------------------------------------------------------------------------------------------------------------------ the lobes
class Lobe:
    """One BxDF as a material adds it.  kind: lambert lambert_t oren spec_r spec_t fr_spec mf_r mf_t blend."""

    def __init__(self, kind, type_, r, **kw):
        self.kind, self.type, self.r = kind, type_, r
        self.t = self.k = self.a = self.b = self.dist = self.eta_a = self.eta_b = self.fr_i = self.fr_t = None
        self.fresnel = "noop"
        for k, v in kw.items():
            setattr(self, k, v)

    def matches(self, flags):                                          # bxdf.rs:17-20
        return (self.type & flags) == self.type

    def fresnel_eval(self, cos_i, und):                                # fresnel.rs:100-122, :226-229
        if self.fresnel == "dielectric":
            f = fr_dielectric(cos_i, self.fr_i, self.fr_t, und)
            return [f, f, f]
        if self.fresnel == "conductor":
            one = full_like(cos_i, 1.0)
            return fr_conductor(cos_i.abs(), [one, one, one], self.t, self.k)
        one = full_like(cos_i, 1.0)
        return [one, one, one]


def rgb_zero(like):
    return [zeros_like(like) for _ in range(3)]


def lobe_f(l, wo, wi, und):
    """BxDF::f of one lobe: RGB of E.  `und` collects the undecided evaluations."""
    like = wo[2] + wi[2]
    if l.kind in ("lambert", "lambert_t"):                             # lambertian.rs:17-19, :60-62
        return [bcast(c * INV_PI, like) for c in l.r]
    if l.kind == "oren":                                               # oren_nayar.rs:27-49
        si, so = sin_theta(wi), sin_theta(wo)
        decide(si, und, c32(1e-4))
        decide(so, und, c32(1e-4))
        both = (si.v > F(1e-4)) & (so.v > F(1e-4))
        d_cos = cos_phi(wi) * cos_phi(wo) + sin_phi(wi) * sin_phi(wo)
        max_cos = where(both, emax(d_cos, 0.0), zeros_like(d_cos))
        ai, ao = wi[2].abs(), wo[2].abs()
        with np.errstate(all="ignore"):
            i_big = ai.v > ao.v
            sin_a = where(i_big, so, si)
            tan_b = where(i_big, si / ai, so / ao)
        k = l.a + l.b * max_cos * sin_a * tan_b
        return [c * INV_PI * k for c in l.r]
    if l.kind == "mf_r":                                               # microfacet.rs:29-60
        co, ci = wo[2].abs(), wi[2].abs()
        wh = vadd(wi, wo)
        zero = (ci.v == 0) | (co.v == 0) | ((wh[0].v == 0) & (wh[1].v == 0) & (wh[2].v == 0))
        und |= np.all([np.abs(c.v.astype(np.float64)) <= c.e for c in wh], 0) & np.any([c.e > 0 for c in wh], 0)
        with np.errstate(all="ignore"):
            wh = vnorm(wh)
            uf = np.zeros(len(zero), bool)
            if l.fresnel == "dielectric":
                decide(wh[2], uf)                                      # face_forward(wh, (0,0,1)): the side the Fresnel term is entered from
            whf = vwhere(wh[2].v < 0, vneg(wh), wh)
            fr = l.fresnel_eval(vdot(wi, whf), uf)
            und |= uf & ~zero
            s = l.dist.d(wh, und) * l.dist.g(wo, wi, und) / (4.0 * ci * co)
            f = [l.r[c] * fr[c] * s for c in range(3)]
        return rgb_where(zero, rgb_zero(like), f)
    if l.kind == "mf_t":                                               # microfacet.rs:143-192
        us = np.zeros(len(like.v), bool)
        same = same_hemisphere(wo, wi, us)
        und |= us
        co, ci = wo[2], wi[2]
        zero = same | (ci.v == 0) | (co.v == 0)
        with np.errstate(all="ignore"):
            eta = where(co.v > 0, l.eta_b / l.eta_a, l.eta_a / l.eta_b)
            wh = vnorm(vadd(wo, vscale(wi, eta)))
            wh = vwhere(wh[2].v < 0, vneg(wh), wh)                     # (f is even in wh up to the Fresnel side, which decide() below reads)
            wo_wh, wi_wh = vdot(wo, wh), vdot(wi, wh)
            ub = np.zeros(len(zero), bool)
            p = wo_wh * wi_wh
            decide(p, ub)
            back = p.v > 0
            fr = fr_dielectric(vdot(wo, wh), l.eta_a, l.eta_b, ub)
            und |= ub & ~zero
            sqrt_denom = wo_wh + eta * wi_wh
            factor = 1.0 / eta                                         # TransportMode::Radiance
            ud = np.zeros(len(zero), bool)
            d = (l.dist.d(wh, ud) * l.dist.g(wo, wi, ud) * eta * eta * wi_wh.abs() * wo_wh.abs() * factor * factor
                 / (ci * co * sqrt_denom * sqrt_denom)).abs()
            und |= ud & ~zero & ~back
            f = [((1.0 - fr) * l.r[c]) * d for c in range(3)]
        return rgb_where(zero | back, rgb_zero(like), f)
    if l.kind == "blend":                                              # fresnel_blend.rs:36-55
        ai, ao = wi[2].abs(), wo[2].abs()
        k = E(np.asarray(c32(28.0), like.v.dtype)) / (E(np.asarray(c32(23.0), like.v.dtype)) * PI)
        a = 1.0 - pow5(1.0 - 0.5 * ai)
        b = 1.0 - pow5(1.0 - 0.5 * ao)
        diffuse = [l.r[c] * (1.0 - l.t[c]) * a * b * k for c in range(3)]
        wh = vadd(wi, wo)
        zero = (wh[0].v == 0) & (wh[1].v == 0) & (wh[2].v == 0)
        with np.errstate(all="ignore"):
            wh = vnorm(wh)
            p5 = pow5(1.0 - vdot(wi, wh))
            s = l.dist.d(wh, und) / (4.0 * vdot(wi, wh).abs() * emax2(ai, ao))
            f = [diffuse[c] + (l.t[c] + (1.0 - l.t[c]) * p5) * s for c in range(3)]
        return rgb_where(zero, rgb_zero(like), f)
    return rgb_zero(like)                                              # the specular lobes: fresnel.rs:151-153, specular.rs:22-24, :74-76


def lobe_pdf(l, wo, wi, und):
    like = wo[2] + wi[2]
    zero = zeros_like(like)
    if l.kind in ("lambert", "oren"):                                  # bxdf.rs:88-94
        same = same_hemisphere(wo, wi, und)
        return where(same, wi[2].abs() * INV_PI, zero)
    if l.kind == "lambert_t":                                          # lambertian.rs:80-86 (Q53)
        same = same_hemisphere(wo, wi, und)
        return where(~same, wi[2].abs(), zero)
    if l.kind in ("mf_r", "blend"):                                    # microfacet.rs:90-103, fresnel_blend.rs:91-104
        same = same_hemisphere(wo, wi, und)
        with np.errstate(all="ignore"):
            wh = vnorm(vadd(wo, wi))
            d = vdot(wo, wh)
            ub = np.zeros(len(same), bool)
            decide(d, ub)
            back = d.v < 0
            ud = np.zeros(len(same), bool)
            p = l.dist.pdf(wo, wh, ud) / (4.0 * d)
            und |= (ub | (ud & ~back)) & same
            if l.kind == "blend":
                p = 0.5 * (wi[2].abs() * INV_PI + p)
        return where(same & ~back, p, zero)
    if l.kind == "mf_t":                                               # microfacet.rs:226-254 (Q19: no wo . wh < 0 guard)
        same = same_hemisphere(wo, wi, und)
        with np.errstate(all="ignore"):
            eta = where(wo[2].v > 0, l.eta_b / l.eta_a, l.eta_a / l.eta_b)
            wh = vnorm(vadd(wo, vscale(wi, eta)))
            wo_wh, wi_wh = vdot(wo, wh), vdot(wi, wh)
            ub = np.zeros(len(same), bool)
            pr = wo_wh * wi_wh
            decide(pr, ub)
            back = pr.v > 0
            sqrt_denom = wo_wh + eta * wi_wh
            dwh_dwi = ((eta * eta * wi_wh) / (sqrt_denom * sqrt_denom)).abs()
            ud = np.zeros(len(same), bool)
            p = l.dist.pdf(wo, wh, ud) * dwh_dwi
            und |= (ub | (ud & ~back)) & ~same
        return where(~same & ~back, p, zero)
    return zero                                                        # specular lobes


def lobe_sample(l, wo, u1, u2, und):
    """BxDF::sample_f of one lobe on exact wo and a (possibly remapped) u: dict f (RGB or None = "re-summed by the BSDF"), wi, pdf,
    type (0 = get_type()), some (False where it returns None)."""
    n = len(wo[2].v)
    dt = wo[2].v.dtype
    some = np.ones(n, bool)
    t = np.zeros(n, np.uint32)
    one = full_like(wo[2], 1.0)
    if l.kind in ("lambert", "oren", "lambert_t"):                     # bxdf.rs:74-86, lambertian.rs:63-79
        wi = cosine_sample_hemisphere(u1, u2)
        neg = (wo[2].v > 0) if l.kind == "lambert_t" else (wo[2].v < 0)
        wi[2] = where(neg, -wi[2], wi[2])
        pdf = lobe_pdf(l, wo, wi, und)
        if l.kind == "lambert_t":
            decide(pdf, und)
            some &= pdf.v > 0
        return dict(f=None, wi=wi, pdf=pdf, type=t, some=some)
    if l.kind == "spec_r":                                             # specular.rs:26-38
        wi = [-wo[0], -wo[1], wo[2]]
        fr = l.fresnel_eval(wi[2], und)
        f = [(fr[c] * l.r[c]) / wi[2].abs() for c in range(3)]
        return dict(f=f, wi=wi, pdf=one, type=t, some=some)
    if l.kind in ("spec_t", "fr_spec"):
        entering = wo[2].v > 0
        eta_i, eta_t = where(entering, l.eta_a, l.eta_b), where(entering, l.eta_b, l.eta_a)
        nz = full_like(wo[2], 1.0)
        nrm = [zeros_like(nz), zeros_like(nz), where(entering, nz, -nz)]        # face_forward((0,0,1), wo): wo exact, wo.z != 0 here
        with np.errstate(all="ignore"):
            ur = np.zeros(n, bool)
            wt, ok = refract(wo, nrm, eta_i / eta_t, ur)
            scale = (eta_i * eta_i) / (eta_t * eta_t)
            if l.kind == "spec_t":                                     # specular.rs:78-107
                und |= ur
                uf = np.zeros(n, bool)
                fr = fr_dielectric(wt[2], l.eta_a, l.eta_b, uf)
                und |= uf & ok
                f = [(l.r[c] * (1.0 - fr)) * scale / wt[2].abs() for c in range(3)]
                return dict(f=f, wi=wt, pdf=one, type=t, some=ok)
            fr = fr_dielectric(wo[2], l.eta_a, l.eta_b, und)            # fresnel.rs:155-203
            decide(fr - u1, und)
            refl = u1.v < fr.v
            und |= ur & ~refl
            wr = [-wo[0], -wo[1], wo[2]]
            f_r = [l.r[c] * (fr / wr[2].abs()) for c in range(3)]
            f_t = [(l.t[c] * (1.0 - fr)) * scale / wt[2].abs() for c in range(3)]
        t = np.where(refl, SPECULAR | REFL, SPECULAR | TRANS).astype(np.uint32)
        return dict(f=rgb_where(refl, f_r, f_t), wi=vwhere(refl, wr, wt), pdf=where(refl, fr, 1.0 - fr), type=t, some=refl | ok)
    if l.kind == "mf_r":                                               # microfacet.rs:62-88
        with np.errstate(all="ignore"):
            wh = l.dist.sample_wh(wo, u1, u2, und)
            d = vdot(wo, wh)
            decide(d, und)
            some &= ~(d.v < 0)
            wi = reflect(wo, wh)
            some &= same_hemisphere(wo, wi, und)
            pdf = l.dist.pdf(wo, wh, und) / (4.0 * d)
            some &= ~(pdf.v == 0)
        return dict(f=None, wi=wi, pdf=pdf, type=t, some=some)
    if l.kind == "mf_t":                                               # microfacet.rs:194-224
        with np.errstate(all="ignore"):
            wh = l.dist.sample_wh(wo, u1, u2, und)
            d = vdot(wo, wh)
            decide(d, und)
            some &= ~(d.v < 0)
            eta = where(wo[2].v > 0, l.eta_a / l.eta_b, l.eta_b / l.eta_a)
            ur = np.zeros(n, bool)
            wi, ok = refract(wo, wh, eta, ur)
            und |= ur & some
            some &= ok
            up = np.zeros(n, bool)
            pdf = lobe_pdf(l, wo, wi, up)
            decide(pdf, up)
            und |= up & some
            some &= pdf.v > 0
        return dict(f=None, wi=wi, pdf=pdf, type=t, some=some)
    if l.kind == "blend":                                              # fresnel_blend.rs:57-89
        decide(u1 - 0.5, und)
        diff = u1.v < np.asarray(0.5, dt)
        with np.errstate(all="ignore"):
            ua = emin(2.0 * u1, ONE_MINUS_EPSILON)
            wd = cosine_sample_hemisphere(ua, u2)
            wd[2] = where(wo[2].v < 0, -wd[2], wd[2])
            ub = emin(2.0 * (u1 - 0.5), ONE_MINUS_EPSILON)
            us = np.zeros(n, bool)
            wh = l.dist.sample_wh(wo, ub, u2, us)
            ws = reflect(wo, wh)
            same = same_hemisphere(wo, ws, us)
            und |= us & ~diff
            some &= diff | same
            wi = vwhere(diff, wd, ws)
            up = np.zeros(n, bool)
            pdf = lobe_pdf(l, wo, wi, up)
            decide(pdf, up)
            und |= up & some
            some &= pdf.v > 0
        return dict(f=None, wi=wi, pdf=pdf, type=t, some=some)
    raise ValueError(l.kind)


# ------------------------------------------------------------------------------------------------------------------ the materials
def build_lobes(p, dt):
    """Material::compute_scattering_functions for constant parameters p (a dict: "type" and the scene description's parameter names):
    (has_bsdf, [Lobe]) in the order the material adds them."""
    def num(x): return E(np.asarray(c32(x), dt))
    def rgb(name, default): return [num(c) for c in p.get(name, (default,) * 3)]
    def cz(c): return [emax(x, 0.0) for x in c]                        # Spectrum::clamp_zero
    def black(c): return all(float(x.v) == 0.0 for x in c)
    def mul(a, b): return [a[i] * b[i] for i in range(3)]
    remap = bool(p.get("remaproughness", True))
    def alpha(x): return roughness_to_alpha(x, dt) if remap else x
    def rough_uv():                                                    # metal.rs:36-49 / uber.rs:48-61: "uroughness" falls back to "roughness"
        r = num(p.get("roughness", 0.01 if kind == "metal" else 0.1))
        u = r if p.get("uroughness") is None else num(p["uroughness"])
        v = r if p.get("vroughness") is None else num(p["vroughness"])
        return alpha(u), alpha(v)
    kind = p["type"]
    one = num(1.0)
    lobes = []
    if kind == "matte":                                                # matte.rs:37-51 (Kd is not clamped)
        r = rgb("Kd", 0.5)
        sig = eclamp(num(p.get("sigma", 0.0)), 0.0, 90.0)
        if not black(r):
            if float(sig.v) == 0.0:
                lobes.append(Lobe("lambert", REFL | DIFFUSE, r))
            else:                                                      # oren_nayar.rs:17-23
                s = sig * (E(np.asarray(PI, dt)) / num(180.0))
                s2 = s * s
                a = 1.0 - (s2 / (2.0 * (s2 + num(0.33))))
                b = num(0.45) * s2 / (s2 + num(0.09))
                lobes.append(Lobe("oren", REFL | DIFFUSE, r, a=a, b=b))
        return True, lobes
    if kind == "plastic":                                              # plastic.rs:43-69
        kd, ks = cz(rgb("Kd", 0.25)), cz(rgb("Ks", 0.25))
        if not black(kd):
            lobes.append(Lobe("lambert", REFL | DIFFUSE, kd))
        if not black(ks):
            a = alpha(num(p.get("roughness", 0.1)))
            lobes.append(Lobe("mf_r", REFL | GLOSSY, ks, dist=TR(a, a), fresnel="dielectric", fr_i=num(1.5), fr_t=one))
        return True, lobes
    if kind == "mirror":                                               # mirror.rs:30-39
        r = cz(rgb("Kr", 0.9))
        if not black(r):
            lobes.append(Lobe("spec_r", REFL | SPECULAR, r))
        return True, lobes
    if kind == "glass":                                                # glass.rs:58-108, allow_multiple_lobes = true (Kr, Kt not clamped)
        eta = num(p.get("eta", 1.5))
        ur, vr = num(p.get("uroughness", 0.0)), num(p.get("vroughness", 0.0))
        r, t = rgb("Kr", 1.0), rgb("Kt", 1.0)
        if black(r) and black(t):
            return False, []
        if float(ur.v) == 0.0 and float(vr.v) == 0.0:
            return True, [Lobe("fr_spec", REFL | TRANS | SPECULAR, r, t=t, eta_a=one, eta_b=eta)]
        ur, vr = alpha(ur), alpha(vr)
        if not black(r):
            lobes.append(Lobe("mf_r", REFL | GLOSSY, r, dist=TR(ur, vr), fresnel="dielectric", fr_i=one, fr_t=eta))
        if not black(t):
            lobes.append(Lobe("mf_t", TRANS | GLOSSY, t, dist=TR(ur, vr), eta_a=one, eta_b=eta))
        return True, lobes
    if kind == "metal":                                                # metal.rs:62-83
        u, v = rough_uv()
        return True, [Lobe("mf_r", REFL | GLOSSY, [one, one, one], dist=TR(u, v), fresnel="conductor", t=rgb("eta", 1.0), k=rgb("k", 1.0))]
    if kind == "uber":                                                 # uber.rs:75-125
        e = num(p.get("eta", 1.5))
        op = rgb("opacity", 1.0)
        t = cz([1.0 - c for c in op])
        if not black(t):
            lobes.append(Lobe("spec_t", TRANS | SPECULAR, t, eta_a=one, eta_b=one))
        kd = mul(op, cz(rgb("Kd", 0.25)))
        if not black(kd):
            lobes.append(Lobe("lambert", REFL | DIFFUSE, kd))
        ks = mul(op, cz(rgb("Ks", 0.25)))
        if not black(ks):
            u, v = rough_uv()
            lobes.append(Lobe("mf_r", REFL | GLOSSY, ks, dist=TR(u, v), fresnel="dielectric", fr_i=one, fr_t=e))
        kr = mul(op, cz(rgb("Kr", 0.0)))
        if not black(kr):
            lobes.append(Lobe("spec_r", REFL | SPECULAR, kr, fresnel="dielectric", fr_i=one, fr_t=e))
        kt = mul(op, cz(rgb("Kt", 0.0)))
        if not black(kt):
            lobes.append(Lobe("spec_t", TRANS | SPECULAR, kt, eta_a=one, eta_b=e))
        return True, lobes
    if kind == "substrate":                                            # substrate.rs:46-66
        d, s = cz(rgb("Kd", 0.5)), cz(rgb("Ks", 0.5))
        if not black(d) and not black(s):
            u, v = alpha(num(p.get("uroughness", 0.1))), alpha(num(p.get("vroughness", 0.1)))
            lobes.append(Lobe("blend", REFL | GLOSSY, d, t=s, dist=TR(u, v)))
        return True, lobes
    if kind == "translucent":                                          # translucent.rs:48-106
        eta = num(1.5)                                                 # :48 (Q55)
        r, t = cz(rgb("reflect", 0.5)), cz(rgb("transmit", 0.5))
        if black(r) and black(t):
            return False, []                                           # :56-58 (Q54)
        kd = cz(rgb("Kd", 0.25))
        if not black(kd):
            if not black(r):
                lobes.append(Lobe("lambert", REFL | DIFFUSE, mul(r, kd)))
            if not black(t):
                lobes.append(Lobe("lambert_t", TRANS | DIFFUSE, mul(t, kd)))
        ks = cz(rgb("Ks", 0.25))
        if not black(ks):
            a = alpha(num(p.get("roughness", 0.1)))                    # one roughness for both (Q56)
            if not black(r):
                lobes.append(Lobe("mf_r", REFL | GLOSSY, mul(r, ks), dist=TR(a, a), fresnel="dielectric", fr_i=one, fr_t=eta))
            if not black(t):
                lobes.append(Lobe("mf_t", TRANS | GLOSSY, mul(t, ks), dist=TR(a, a), eta_a=one, eta_b=eta))
        return True, lobes
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------------------------ bsdf.rs
class Value:
    """f (n, 3) and pdf (n,) with their bounds, and the undecided evaluations."""

    def __init__(self, f, pdf, und):
        self.f = np.stack([c.v for c in f], 1).astype(np.float64)
        self.f_e = np.stack([c.e for c in f], 1)
        self.pdf, self.pdf_e = pdf.v.astype(np.float64), pdf.e
        self.und = und

    def left_out(self):
        """und, or a bound past REL_CAP of its (non-zero) value, or a bound that is not finite."""
        with np.errstate(all="ignore"):
            wide_f = ((self.f_e > REL_CAP * np.abs(self.f)) & (self.f_e > 0)).any(1) | ~np.isfinite(self.f_e).all(1) | ~np.isfinite(self.f).all(1)
            wide_p = ((self.pdf_e > REL_CAP * np.abs(self.pdf)) & (self.pdf_e > 0)) | ~np.isfinite(self.pdf_e) | ~np.isfinite(self.pdf)
        return self.und | wide_f | wide_p


class BSDF:
    """The BSDF of a material's parameters on the canonical frame, in the run's dtype."""

    def __init__(self, params, dtype=np.float64):
        self.dt = np.dtype(dtype).type
        self.has_bsdf, self.lobes = build_lobes(params, self.dt)

    def _in(self, w):
        return w if isinstance(w, list) else vexact(w, self.dt)

    def terms(self, wo, wi):
        """Per lobe (f, pdf, und) at (wo, wi): shared by the flag sets."""
        wo, wi = self._in(wo), self._in(wi)
        out = []
        for l in self.lobes:
            und = np.zeros(len(wo[2].v), bool)
            out.append((lobe_f(l, wo, wi, und), lobe_pdf(l, wo, wi, und), und))
        return wo, wi, out

    def combine(self, wo, wi, terms, flags):
        """BSDF::f (bsdf.rs:208-236) and BSDF::pdf (:238-270) from the per-lobe terms."""
        n = len(wo[2].v)
        und = np.zeros(n, bool)
        like = wo[2] + wi[2]
        dead = (wo[2].v == 0) | ~np.isfinite(wo[0].v + wo[1].v + wo[2].v)          # :214-216
        ur = np.zeros(n, bool)
        refl = same_hemisphere(wi, wo, ur)                             # dot(wi, ng) dot(wo, ng) > 0 on ng = (0,0,1)
        f, pdf, count, sided = None, None, 0, False
        for l, (lf, lp, lu) in zip(self.lobes, terms):
            if not l.matches(flags):
                continue
            count += 1
            pdf = lp if pdf is None else pdf + lp
            und |= lu
            if l.kind in ("spec_r", "spec_t", "fr_spec"):
                continue                                               # f is zero on either side: `reflect` does not enter
            use = (refl & bool(l.type & REFL)) | (~refl & bool(l.type & TRANS))
            sided = True
            term = rgb_where(use, lf, rgb_zero(like))
            f = term if f is None else [f[c] + term[c] for c in range(3)]
        if sided:
            und |= ur
        f = rgb_zero(like) if f is None else f
        pdf = zeros_like(like) if pdf is None else (pdf / float(count) if count > 1 else pdf)
        f = rgb_where(dead, rgb_zero(like), f)
        pdf = where(dead, zeros_like(like), pdf)
        return Value(f, pdf, und & ~dead)

    def eval(self, wo, wi, flags=ALL):
        if not self.has_bsdf:
            z = E(np.zeros(len(wo), self.dt))
            return Value([z, z, z], z, np.zeros(len(wo), bool))
        wo, wi, t = self.terms(wo, wi)
        return self.combine(wo, wi, t, flags)

    def f(self, wo, wi, flags=ALL):
        v = self.eval(wo, wi, flags)
        return v.f, v.f_e

    def pdf(self, wo, wi, flags=ALL):
        v = self.eval(wo, wi, flags)
        return v.pdf, v.pdf_e

    def sample(self, wo, u, flags=ALL):
        """BSDF::sample_f (bsdf.rs:92-206): dict with wi (n, 3) and its bound wi_e, type (n,) uint32 (0 where it returns None), und (n,),
        pick (n,) = index of the chosen lobe in self.lobes, specular (n,) = the chosen lobe is specular, and f / pdf with their
        bounds: a specular pick's closed forms at wo, a non-specular pick's re-summed f and averaged pdf at the sampled wi (whose own
        bound they carry)."""
        n = len(wo)
        dt = self.dt
        out = dict(wi=np.zeros((n, 3)), wi_e=np.zeros((n, 3)), type=np.zeros(n, np.uint32), und=np.zeros(n, bool), pick=np.full(n, -1),
                   specular=np.zeros(n, bool), f=np.zeros((n, 3)), f_e=np.zeros((n, 3)), pdf=np.zeros(n), pdf_e=np.zeros(n))
        match = [i for i, l in enumerate(self.lobes) if l.matches(flags)]
        m = len(match)
        if not self.has_bsdf or m == 0:                                # :100-103
            return out
        wov = vexact(wo, dt)
        u1, u2 = E(np.asarray(u, np.float32)[:, 0].astype(dt)), E(np.asarray(u, np.float32)[:, 1].astype(dt))
        um = u1 * float(m)
        fl = np.floor(um.v)
        und = np.zeros(n, bool)
        for b in range(1, m):                                          # the lobe index floor(u.x matching)
            decide(um, und, float(b))
        comp = np.minimum(fl.astype(np.int64), m - 1)
        remapped = emin(um - E(comp.astype(dt)), ONE_MINUS_EPSILON)    # :134-140
        dead = (wov[2].v == 0) | ~np.isfinite(wov[0].v + wov[1].v + wov[2].v)      # :142-145
        for j, li in enumerate(match):
            sel = (comp == j) & ~dead
            if not sel.any():
                continue
            l = self.lobes[li]
            w = [c.take(sel) for c in wov]
            ul = np.zeros(int(sel.sum()), bool)
            s = lobe_sample(l, w, remapped.take(sel), u2.take(sel), ul)
            some = s["some"].copy()
            up = np.zeros(len(ul), bool)
            decide(s["pdf"], up)                                       # :149-152, pdf <= 0
            ul |= up & some
            some &= ~(s["pdf"].v <= 0)
            spec = bool(l.type & SPECULAR)
            t = np.where(s["type"] != 0, s["type"], l.type).astype(np.uint32)
            idx = np.flatnonzero(sel)
            out["pick"][idx] = li
            out["specular"][idx] = spec
            out["type"][idx] = np.where(some, t, 0)
            out["und"][idx] = ul
            out["wi"][idx] = np.where(some[:, None], np.stack([c.v for c in s["wi"]], 1).astype(np.float64), 0.0)
            out["wi_e"][idx] = np.where(some[:, None], np.stack([c.e for c in s["wi"]], 1), 0.0)
            if spec:
                pdf = s["pdf"] / float(m) if m > 1 else s["pdf"]      # :174-176
                out["f"][idx] = np.where(some[:, None], np.stack([c.v for c in s["f"]], 1).astype(np.float64), 0.0)
                out["f_e"][idx] = np.where(some[:, None], np.stack([c.e for c in s["f"]], 1), 0.0)
                out["pdf"][idx] = np.where(some, pdf.v.astype(np.float64), 0.0)
                out["pdf_e"][idx] = np.where(some, pdf.e, 0.0)
            else:                                                      # :163-197: the other lobes' pdfs, f re-summed, at the sampled wi
                terms = []
                with np.errstate(all="ignore"):
                    for k, l2 in enumerate(self.lobes):
                        u2_ = np.zeros(len(ul), bool)
                        terms.append((lobe_f(l2, w, s["wi"], u2_), s["pdf"] if k == li else lobe_pdf(l2, w, s["wi"], u2_), u2_))
                    val = self.combine(w, s["wi"], terms, flags)
                out["f"][idx], out["f_e"][idx] = np.where(some[:, None], val.f, 0.0), np.where(some[:, None], val.f_e, 0.0)
                out["pdf"][idx], out["pdf_e"][idx] = np.where(some, val.pdf, 0.0), np.where(some, val.pdf_e, 0.0)
        out["und"] |= und & ~dead
        return out

    def eval_at_sampled(self, wo, wi, pick, flags=ALL):
        """(c): f and pdf of sample_f at a RETURNED float32 wi taken as an exact input -- f re-summed (:179-197), pdf averaged over the
        matching lobes (:163-176).  Every lobe's sample_f computes its pdf by calling pdf(wo, wi) on the wi it returns, except
        MicrofacetReflection, which uses the half vector it sampled (microfacet.rs:81): the returned wi is reflect(wo, wh) in float32
        (5 roundings of the dot product at magnitude <= 1, one of its product with 2 wh_i at magnitude <= 2, one of the sum: 8 ulp of 1),
        so for those picks wi enters the pdf with REFLECT_ERR per component.  f is always self.f(wo, wi) on the returned wi."""
        exact = self.eval(wo, wi, flags)
        mfr = np.array([l.kind == "mf_r" for l in self.lobes] + [False])[pick]
        if mfr.any():
            idx = np.flatnonzero(mfr)
            wi_e = [E(np.asarray(wi, np.float32)[idx, i].astype(self.dt), REFLECT_ERR) for i in range(3)]
            wide = self.eval(vexact(np.asarray(wo)[idx], self.dt), wi_e, flags)
            exact.pdf[idx], exact.pdf_e[idx] = wide.pdf, wide.pdf_e
            exact.und[idx] |= wide.und
        return exact


REFLECT_ERR = 8.0 * U
