"""Restatement of Material "disney" in numpy, on top of bsdf_ref (which it imports and leaves alone): create_disney_material and
DisneyMaterial::compute_scattering_functions (materials/disney.rs:644-841), its five BxDFs (:44-323), DisneyFresnel (:330-345) and
DisneyMicrofacetDistribution (:351-378), under BSDF::f / pdf / sample_f (core/reflection/bsdf.rs:92-270) on the canonical frame.  Written
from the reference's text, parameters in and lobes out; independent of the oracle and of the product.

Input is a dict: {"type": "disney", "color": (r, g, b), "metallic": .., ...} with the scene description's parameter names; what is
missing takes create_disney_material's default.

What is restated, as the text has it
  * :17-26    schlick_weight = clamp(1 - cos, 0, 1) multiplied out five times; fr_schlick = lerp(weight, r0, 1); lerp(t, a, b) = (1 - t) a + t b
  * :53-76    DisneyDiffuse: f, and pdf = 0 -- it adds nothing to the averaged pdf, and a pick of it makes BSDF::sample_f return None
  * :95-126   DisneyFakeSS;  :145-175 DisneyRetro;  :193-218 DisneySheen: f as written, sample_f_default / pdf_default (bxdf.rs:74-94)
  * :238-250  gtr1 (ln) and smith_g_ggx;  :253-268 DisneyClearcoat::f;  :269-300 its sample_f (powf, the flip of wh, reflect, None across
              hemispheres);  :303-319 its pdf = dr + |cos wh| / (4 |cos wo|), a sum
  * :341-344  DisneyFresnel::evaluate with schlick_r0_from_eta and r0.y()
  * :368-371  DisneyMicrofacetDistribution::g = g1(wo) g1(wi); d, lambda, sample_wh and pdf are TrowbridgeReitz's
  * :644-804  the lobe list: order, conditions on the evaluated values, c_tint, c_sheen, cspec0, aspect, ax / ay with the 0.001 floor, gloss,
              the thin variants (FakeSS, the plain distribution on the scaled roughness, LambertianTransmission always added)

Run in float64 it is the truth; run in float32 it is the calibration.  Every quantity is bsdf_ref's E with propagated bounds: ln adds
LIBM_ULP, powf adds POW_ULP, sin and cos add their 2 ulp, and no constant is fitted.  Undecided (`und`): wh = 0; both same_hemisphere tests
of the clearcoat's sample_f and the one of its pdf; the max(0, .) under the clearcoat's square root; the side DisneyFresnel is entered
from (face_forward of wh); the lobe pick; pdf <= 0 -- on top of what bsdf_ref decides inside the two microfacet lobes and the Lambertian
transmission.  DisneyDiffuse's pdf is a decided 0, not a value near 0.

The class has the interface bsdf_cases.check_eval / check_sample use: terms, combine, eval, sample, eval_at_sampled, lobes[i].kind /
.matches."""
import numpy as np

import bsdf_ref as R
from bsdf_ref import (E, U, decide, emax, emin, eclamp, elog, where, full_like, zeros_like, bcast, rgb_where, rgb_zero, vexact, vadd, vnorm,
                      vdot, vneg, vwhere, same_hemisphere, reflect, cosine_sample_hemisphere, c32, ecos, esin)

ALL = R.ALL
PI, INV_PI = R.PI, R.INV_PI
DISNEY_KINDS = ("d_diffuse", "d_fakess", "d_retro", "d_sheen", "d_clearcoat")
DEFAULTS = dict(color=(0.5, 0.5, 0.5), metallic=0.0, eta=1.5, roughness=0.5, speculartint=0.0, anisotropic=0.0, sheen=0.0, sheentint=0.5,
                clearcoat=0.0, clearcoatgloss=1.0, spectrans=0.0, scatterdistance=(0.0, 0.0, 0.0), thin=False, flatness=0.0, difftrans=1.0)
YWEIGHT = (c32(0.212671), c32(0.715160), c32(0.072169))            # RGBSpectrum::y (core/spectrum/rgb.rs:60-63)


def lerp(t, a, b):                                  # core lerp: (1 - t) a + t b
    return (1.0 - t) * a + t * b


def schlick_weight(c):                              # :18-21
    m = eclamp(1.0 - c, 0.0, 1.0)
    return m * m * m * m * m


def lum(c):
    return YWEIGHT[0] * c[0] + YWEIGHT[1] * c[1] + YWEIGHT[2] * c[2]


def schlick_r0_from_eta(e):                         # :37-39
    return ((e - 1.0) * (e - 1.0)) / ((e + 1.0) * (e + 1.0))


def powf(x, y):
    """Float::powf(x, y) for x > 0: the exact power, first-order in both arguments, plus POW_ULP."""
    with np.errstate(all="ignore"):
        v = np.power(x.v, y.v)
        x64, y64, v64 = x.v.astype(np.float64), y.v.astype(np.float64), np.abs(np.asarray(v, np.float64))
        e = np.abs(y64) * v64 / x64 * x.e + np.abs(np.log(x64)) * v64 * y.e + R.POW_ULP * U * v64
    return E(v, e)


def gtr1(cos_theta, alpha):                         # :238-242
    alpha2 = alpha * alpha
    c2 = cos_theta * cos_theta
    return (alpha2 - 1.0) / (PI * elog(alpha2) * (1.0 + (alpha2 - 1.0) * c2))


def smith_g_ggx(cos_theta, alpha):                  # :246-250
    alpha2 = alpha * alpha
    c2 = cos_theta * cos_theta
    return 1.0 / (cos_theta + (alpha2 + c2 - alpha2 * c2).sqrt())


class DisneyTR(R.TR):
    """DisneyMicrofacetDistribution: TrowbridgeReitz with the separable masking term."""

    def g(self, wo, wi, und):                       # :368-371
        return self.g1(wo, und) * self.g1(wi, und)


class Lobe(R.Lobe):
    """bsdf_ref's Lobe with DisneyFresnel as a fourth Fresnel object (fresnel = "disney": r0, metallic, eta)."""

    def fresnel_eval(self, cos_i, und):             # :341-344
        if self.fresnel != "disney":
            return R.Lobe.fresnel_eval(self, cos_i, und)
        g = lerp(self.metallic, schlick_r0_from_eta(self.eta), lum(self.r0))
        w = schlick_weight(cos_i)
        return [self.r0[c] + (g - self.r0[c]) * w for c in range(3)]


def _wh(wo, wi, und):
    """wh = wo + wi, where it is (0, 0, 0), and the normalised vector; an evaluation whose wh is zero within its bound is undecided."""
    wh = vadd(wo, wi)
    zero = (wh[0].v == 0) & (wh[1].v == 0) & (wh[2].v == 0)
    und |= np.all([np.abs(c.v.astype(np.float64)) <= c.e for c in wh], 0) & np.any([c.e > 0 for c in wh], 0)
    with np.errstate(all="ignore"):
        return zero, vnorm(wh)


def lobe_f(l, wo, wi, und):
    """BxDF::f of one lobe of the Disney list; the lobes bsdf_ref knows go to bsdf_ref."""
    if l.kind not in DISNEY_KINDS:
        if l.kind == "mf_r" and l.fresnel == "disney":         # face_forward(wh, (0,0,1)): the side DisneyFresnel's cosine is taken on
            s = wo[2] + wi[2]
            side = np.zeros(len(s.v), bool)
            decide(s, side)
            und |= side & ~((wi[2].v == 0) | (wo[2].v == 0))
        return R.lobe_f(l, wo, wi, und)
    like = wo[2] + wi[2]
    ao, ai = wo[2].abs(), wi[2].abs()
    if l.kind == "d_diffuse":                                  # :53-60
        fo, fi = schlick_weight(ao), schlick_weight(ai)
        return [bcast(c, like) * INV_PI * (1.0 - fo / 2.0) * (1.0 - fi / 2.0) for c in l.r]
    zero, wh = _wh(wo, wi, und)
    with np.errstate(all="ignore"):
        if l.kind == "d_fakess":                               # :95-110
            cd = vdot(wi, wh)
            fss90 = cd * cd * l.roughness
            fo, fi = schlick_weight(ao), schlick_weight(ai)
            fss = lerp(fo, 1.0, fss90) * lerp(fi, 1.0, fss90)
            ss = 1.25 * fss * (1.0 / (ao + ai) - 0.5)
            f = [bcast(c, like) * INV_PI * ss for c in l.r]
        elif l.kind == "d_retro":                              # :145-159
            cd = vdot(wi, wh)
            fo, fi = schlick_weight(ao), schlick_weight(ai)
            rr = 2.0 * l.roughness * cd * cd
            f = [bcast(c, like) * INV_PI * rr * (fo + fi + fo * fi * (rr - 1.0)) for c in l.r]
        elif l.kind == "d_sheen":                              # :193-202
            w = schlick_weight(vdot(wi, wh))
            f = [bcast(c, like) * w for c in l.r]
        else:                                                  # d_clearcoat, :253-268
            dr = gtr1(wh[2].abs(), l.gloss)
            fr = lerp(schlick_weight(vdot(wo, wh)), c32(0.04), 1.0)
            q = E(np.asarray(c32(0.25), like.v.dtype))
            gr = smith_g_ggx(ao, q) * smith_g_ggx(ai, q)
            v = l.weight * gr * fr * dr / 4.0
            f = [v, v, v]
    return rgb_where(zero, rgb_zero(like), f)


def lobe_pdf(l, wo, wi, und):
    if l.kind not in DISNEY_KINDS:
        return R.lobe_pdf(l, wo, wi, und)
    like = wo[2] + wi[2]
    zero = zeros_like(like)
    if l.kind == "d_diffuse":                                  # :74-76
        return zero
    same = same_hemisphere(wo, wi, und)
    if l.kind != "d_clearcoat":                                # pdf_default, bxdf.rs:88-94
        return where(same, wi[2].abs() * INV_PI, zero)
    uz = np.zeros(len(same), bool)                             # :303-319
    none, wh = _wh(wo, wi, uz)
    und |= uz & same
    with np.errstate(all="ignore"):
        p = gtr1(wh[2].abs(), l.gloss) + wh[2].abs() / (4.0 * wo[2].abs())
    return where(same & ~none, p, zero)


def lobe_sample(l, wo, u1, u2, und):
    """BxDF::sample_f of one lobe on exact wo: bsdf_ref.lobe_sample's dict."""
    if l.kind not in DISNEY_KINDS:
        return R.lobe_sample(l, wo, u1, u2, und)
    n = len(wo[2].v)
    some = np.ones(n, bool)
    t = np.zeros(n, np.uint32)
    if l.kind != "d_clearcoat":                                # sample_f_default, bxdf.rs:74-86
        wi = cosine_sample_hemisphere(u1, u2)
        wi[2] = where(wo[2].v < 0, -wi[2], wi[2])
        return dict(f=None, wi=wi, pdf=lobe_pdf(l, wo, wi, und), type=t, some=some)
    with np.errstate(all="ignore"):                            # :269-300 (wo.z == 0 never gets here: BSDF::sample_f returns first)
        alpha2 = bcast(l.gloss * l.gloss, u1)
        arg = 1.0 - powf(alpha2, 1.0 - u1) / (1.0 - alpha2)
        decide(arg, und)                                       # the max(0, .) under the square root
        cos_t = emax(arg, 0.0).sqrt()
        sin_t = emax(1.0 - cos_t * cos_t, 0.0).sqrt()
        phi = 2.0 * PI * u2
        wh = [sin_t * ecos(phi), sin_t * esin(phi), cos_t]
        flip = ~same_hemisphere(wo, wh, und)
        wh = vwhere(flip, vneg(wh), wh)
        wi = reflect(wo, wh)
        some &= same_hemisphere(wo, wi, und)
        pdf = lobe_pdf(l, wo, wi, und)
    return dict(f=None, wi=wi, pdf=pdf, type=t, some=some)


def build_lobes(p, dt):
    """DisneyMaterial::compute_scattering_functions for constant parameters p: ([Lobe] in the order the material adds them, and the
    intermediate values c_tint, cspec0, ax, ay, diffuse_weight, gloss as a dict)."""
    if any(float(x) != 0.0 for x in p.get("scatterdistance", (0.0,) * 3)) and not p.get("thin", False):
        raise ValueError("non-black scatterdistance on a surface that is not thin: the reference reaches todo!() (disney.rs:712)")
    q = dict(DEFAULTS, **{k: v for k, v in p.items() if k != "type"})

    def num(x): return E(np.asarray(c32(x), dt))
    c = [emax(num(x), 0.0) for x in q["color"]]                # :661 clamp_zero
    metallic, e, strans = num(q["metallic"]), num(q["eta"]), num(q["spectrans"])
    diffuse_weight = (1.0 - 0.5 * metallic) * (1.0 - strans)
    dt_ = num(q["difftrans"]) * (1.0 / 2.0)
    rough = num(q["roughness"])
    y = lum(c)
    thin = bool(q["thin"])
    one = num(1.0)
    c_tint = [x / y for x in c] if float(y.v) > 0 else [one, one, one]
    sheen_weight = num(q["sheen"])
    if float(sheen_weight.v) > 0:
        stint = num(q["sheentint"])
        c_sheen = [lerp(stint, 1.0, x) for x in c_tint]
    else:
        c_sheen = [num(0.0)] * 3
    lobes = []
    if float(diffuse_weight.v) > 0:
        if thin:
            flat = num(q["flatness"])
            s = diffuse_weight * (1.0 - flat) * (1.0 - dt_)
            lobes.append(Lobe("d_diffuse", R.REFL | R.DIFFUSE, [s * x for x in c]))
            s = diffuse_weight * flat * (1.0 - dt_)
            lobes.append(Lobe("d_fakess", R.REFL | R.DIFFUSE, [s * x for x in c], roughness=rough))
        else:
            lobes.append(Lobe("d_diffuse", R.REFL | R.DIFFUSE, [diffuse_weight * x for x in c]))
        lobes.append(Lobe("d_retro", R.REFL | R.DIFFUSE, [diffuse_weight * x for x in c], roughness=rough))
        if float(sheen_weight.v) > 0:
            s = diffuse_weight * sheen_weight
            lobes.append(Lobe("d_sheen", R.REFL | R.DIFFUSE, [s * x for x in c_sheen]))
    aspect = (1.0 - num(q["anisotropic"]) * c32(0.9)).sqrt()
    floor = c32(0.001)
    ax, ay = emax(rough * rough / aspect, floor), emax(rough * rough * aspect, floor)
    spec_tint = num(q["speculartint"])
    r0e = schlick_r0_from_eta(e)
    cspec0 = [lerp(metallic, r0e * lerp(spec_tint, 1.0, c_tint[i]), c[i]) for i in range(3)]
    lobes.append(Lobe("mf_r", R.REFL | R.GLOSSY, [one, one, one], dist=DisneyTR(ax, ay), fresnel="disney", r0=cspec0, metallic=metallic, eta=e))
    cc = num(q["clearcoat"])
    gloss = None
    if float(cc.v) > 0:
        gloss = lerp(num(q["clearcoatgloss"]), c32(0.1), c32(0.001))
        lobes.append(Lobe("d_clearcoat", R.REFL | R.GLOSSY, [num(0.0)] * 3, weight=cc, gloss=gloss))
    if float(strans.v) > 0:
        t = [strans * x.sqrt() for x in c]
        if thin:
            rscaled = (c32(0.65) * e - c32(0.35)) * rough
            dist = R.TR(emax((rscaled * rscaled) / aspect, floor), emax((rscaled * rscaled) * aspect, floor))
        else:
            dist = DisneyTR(ax, ay)
        lobes.append(Lobe("mf_t", R.TRANS | R.GLOSSY, t, dist=dist, eta_a=one, eta_b=e))
    if thin:
        lobes.append(Lobe("lambert_t", R.TRANS | R.DIFFUSE, [dt_ * x for x in c]))
    return lobes, dict(c_tint=c_tint, cspec0=cspec0, ax=ax, ay=ay, diffuse_weight=diffuse_weight, gloss=gloss)


class BSDF(R.BSDF):
    """The BSDF a Disney material leaves on the canonical frame (allocated with eta 1, disney.rs:658), in the run's dtype."""

    def __init__(self, params, dtype=np.float64):
        self.dt = np.dtype(dtype).type
        self.has_bsdf = True
        self.lobes, self.info = build_lobes(params, self.dt)

    def terms(self, wo, wi):
        wo, wi = self._in(wo), self._in(wi)
        out = []
        for l in self.lobes:
            und = np.zeros(len(wo[2].v), bool)
            out.append((lobe_f(l, wo, wi, und), lobe_pdf(l, wo, wi, und), und))
        return wo, wi, out

    def sample(self, wo, u, flags=ALL):
        """BSDF::sample_f (bsdf.rs:92-206) over the Disney list: bsdf_ref.BSDF.sample with this module's lobes.  A pick of DisneyDiffuse
        gets pdf 0 from sample_f_default and returns None (:149-152): decided, whatever u is."""
        n = len(wo)
        dt = self.dt
        out = dict(wi=np.zeros((n, 3)), wi_e=np.zeros((n, 3)), type=np.zeros(n, np.uint32), und=np.zeros(n, bool), pick=np.full(n, -1),
                   specular=np.zeros(n, bool), f=np.zeros((n, 3)), f_e=np.zeros((n, 3)), pdf=np.zeros(n), pdf_e=np.zeros(n))
        match = [i for i, l in enumerate(self.lobes) if l.matches(flags)]
        m = len(match)
        if m == 0:
            return out
        wov = vexact(wo, dt)
        u1, u2 = E(np.asarray(u, np.float32)[:, 0].astype(dt)), E(np.asarray(u, np.float32)[:, 1].astype(dt))
        um = u1 * float(m)
        fl = np.floor(um.v)
        und = np.zeros(n, bool)
        for b in range(1, m):                                  # the lobe pick
            decide(um, und, float(b))
        comp = np.minimum(fl.astype(np.int64), m - 1)
        remapped = emin(um - E(comp.astype(dt)), R.ONE_MINUS_EPSILON)
        dead = (wov[2].v == 0) | ~np.isfinite(wov[0].v + wov[1].v + wov[2].v)
        for j, li in enumerate(match):
            sel = (comp == j) & ~dead
            if not sel.any():
                continue
            l = self.lobes[li]
            idx = np.flatnonzero(sel)
            out["pick"][idx] = li
            if l.kind == "d_diffuse":                          # pdf = 0: None, and nothing about it is undecided
                continue
            w = [c.take(sel) for c in wov]
            ul = np.zeros(int(sel.sum()), bool)
            s = lobe_sample(l, w, remapped.take(sel), u2.take(sel), ul)
            some = s["some"].copy()
            up = np.zeros(len(ul), bool)
            decide(s["pdf"], up)                               # :149-152, pdf <= 0
            ul |= up & some
            some &= ~(s["pdf"].v <= 0)
            t = np.where(s["type"] != 0, s["type"], l.type).astype(np.uint32)
            out["type"][idx] = np.where(some, t, 0)
            out["und"][idx] = ul
            out["wi"][idx] = np.where(some[:, None], np.stack([c.v for c in s["wi"]], 1).astype(np.float64), 0.0)
            out["wi_e"][idx] = np.where(some[:, None], np.stack([c.e for c in s["wi"]], 1), 0.0)
            terms = []                                         # no lobe of the list is specular: f re-summed, pdf averaged, at the sampled wi
            with np.errstate(all="ignore"):
                for k, l2 in enumerate(self.lobes):
                    u2_ = np.zeros(len(ul), bool)
                    terms.append((lobe_f(l2, w, s["wi"], u2_), s["pdf"] if k == li else lobe_pdf(l2, w, s["wi"], u2_), u2_))
                val = self.combine(w, s["wi"], terms, flags)
            out["f"][idx], out["f_e"][idx] = np.where(some[:, None], val.f, 0.0), np.where(some[:, None], val.f_e, 0.0)
            out["pdf"][idx], out["pdf_e"][idx] = np.where(some, val.pdf, 0.0), np.where(some, val.pdf_e, 0.0)
        out["und"] |= und & ~dead
        return out


class Restatement32:
    """The float32 run behind the hooks' interface (bsdf_cases.Restatement32 for a Disney material)."""

    def __init__(self, params):
        self.b = BSDF(params, np.float32)

    def eval(self, wo, wi, flags):
        v = self.b.eval(wo, wi, flags)
        return v.f.astype(np.float32), v.pdf.astype(np.float32)

    def sample(self, wo, u, flags):
        s = self.b.sample(wo, u, flags)
        return s["f"].astype(np.float32), s["wi"].astype(np.float32), s["pdf"].astype(np.float32), s["type"]
