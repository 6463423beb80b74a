"""The cases of the Material "disney" truths (tests/disney_ref.py): the settings, named after what they switch on, how a SceneBuilder is
given one, and section 4 of bsdf_cases (eval, sampled type and None decisions, wi, f / pdf at the returned wi) with the Disney truth in the
BSDF's place.  Shared by test_disney_host.py (the float32 run of the restatement, no GPU) and test_gpu_disney.py (the device).

Colours are non-grey except where black is the point.  The settings keep sheen, a small-gloss clearcoat and transmission apart, and
`thin_all` -- all eight lobes -- takes clearcoatgloss 0 (gloss alpha 0.1), so that the restatement's own float32 run stays under
bsdf_cases.MAX_LEFT_OUT; clearcoatgloss 1 (alpha 0.001) and roughness 0 (the 0.001 floor) are directed settings held through the sampling
check alone, uncapped, as bsdf_cases.FLOOR_CASES are."""
import functools

import numpy as np

import bsdf_cases as C
import disney_ref as D
from helpers import scenes

COLOR = (0.6, 0.45, 0.3)


def disney(**kw):
    return dict(dict(type="disney", color=COLOR), **kw)


SETTINGS = {
    "default": disney(),
    "metal": disney(metallic=1.0, speculartint=0.7, color=(0.9, 0.6, 0.2)),
    "aniso": disney(anisotropic=0.8, roughness=0.3),
    "sheen": disney(sheen=1.0, sheentint=0.3, color=(0.3, 0.5, 0.7)),
    "clearcoat": disney(clearcoat=0.7, clearcoatgloss=0.8),
    "glass": disney(spectrans=1.0, color=(0.7, 0.8, 0.6)),                   # diffuse_weight 0: the two microfacet lobes alone
    "half_trans": disney(spectrans=0.5, roughness=0.4),
    "black": disney(color=(0.0, 0.0, 0.0)),                                 # lum 0: c_tint is 1
    "eta_one": disney(eta=1.0, metallic=0.3),                                # schlick_r0_from_eta is 0
    "thin": disney(thin=True, flatness=0.4, difftrans=0.6),
    "thin_all": disney(thin=True, flatness=0.3, difftrans=0.8, sheen=0.6, sheentint=0.7, clearcoat=0.5, clearcoatgloss=0.0, spectrans=0.4,
                       metallic=0.2, anisotropic=0.4, roughness=0.45, scatterdistance=(0.5, 0.2, 0.1)),      # (thin: scatterdistance is never evaluated)
}
# directed and uncapped: the clearcoat's alpha at 0.001 and the distribution's alpha at its 0.001 floor
FLOOR_SETTINGS = {
    "gloss_one": disney(clearcoat=1.0, clearcoatgloss=1.0),
    "rough_zero": disney(roughness=0.0, spectrans=0.5),
}
# the lobe list per setting, written by hand from disney.rs:686-801: (kind, BxDFType) in the order the material adds them
_DR, _GR, _GT, _DT = D.R.REFL | D.R.DIFFUSE, D.R.REFL | D.R.GLOSSY, D.R.TRANS | D.R.GLOSSY, D.R.TRANS | D.R.DIFFUSE
_PLAIN = [("d_diffuse", _DR), ("d_retro", _DR), ("mf_r", _GR)]
LOBE_TABLE = {
    "default": _PLAIN,
    "metal": _PLAIN,
    "aniso": _PLAIN,
    "sheen": [("d_diffuse", _DR), ("d_retro", _DR), ("d_sheen", _DR), ("mf_r", _GR)],
    "clearcoat": _PLAIN + [("d_clearcoat", _GR)],
    "glass": [("mf_r", _GR), ("mf_t", _GT)],
    "half_trans": _PLAIN + [("mf_t", _GT)],
    "black": _PLAIN,
    "eta_one": _PLAIN,
    "thin": [("d_diffuse", _DR), ("d_fakess", _DR), ("d_retro", _DR), ("mf_r", _GR), ("lambert_t", _DT)],
    "thin_all": [("d_diffuse", _DR), ("d_fakess", _DR), ("d_retro", _DR), ("d_sheen", _DR), ("mf_r", _GR), ("d_clearcoat", _GR), ("mf_t", _GT),
                 ("lambert_t", _DT)],
    "gloss_one": _PLAIN + [("d_clearcoat", _GR)],
    "rough_zero": _PLAIN + [("mf_t", _GT)],
}


def params(name):
    return FLOOR_SETTINGS[name] if name in FLOOR_SETTINGS else SETTINGS[name]


def apply(sb, p):
    """Adds the material to the builder; returns its index."""
    sb.material_disney(**{k: v for k, v in p.items() if k != "type"})
    return sb.cur_material


def palette(names=None):
    """One small triangle per setting: the scene only carries the material table for the BSDF hooks."""
    sb = scenes.SceneBuilder()
    sb.look_at((0, -4, 3), (0, 0, 0), (0, 0, 1))
    sb.camera_perspective(fov=50.0)
    sb.film(xresolution=8, yresolution=8)
    sb.pixel_filter_box()
    sb.sampler_sobol(pixelsamples=1)
    sb.integrator_path(maxdepth=1)
    index = {}
    for k, name in enumerate(names or (list(SETTINGS) + list(FLOOR_SETTINGS))):
        index[name] = apply(sb, params(name))
        x = -2.0 + 0.1 * k
        sb.shape_trianglemesh([x, 0, 0, x + 0.05, 0, 0, x, 0.05, 0], [0, 1, 2])
    sb.light_distant(L=(1, 1, 1), frm=(0, 0, 1), to=(0, 0, 0))
    sd = sb.build()
    sd.material_index = index
    return sd


@functools.lru_cache(maxsize=None)
def truth(name):
    return D.BSDF(params(name), np.float64)


def inputs(name):
    return C.inputs("disney", name)           # bsdf_cases' generator: N_BULK drawn pairs and its directed ones (the names only seed it)


def run_setting(name, impl_eval, impl_sample, label):
    """bsdf_cases.run_setting with the Disney truth: a list of Stat over bsdf_cases.FLAG_SETS."""
    b = truth(name)
    wo, wi, u, n = inputs(name)
    gwo, gu = C.grazing_inputs("disney", name)
    stats = []
    wov, wiv, terms = b.terms(wo, wi)
    for fname, flags in C.FLAG_SETS:
        tag = "%s disney/%s %s" % (label, name, fname)
        f, pdf = impl_eval(wo, wi, flags)
        stats += C.check_eval(tag, b.combine(wov, wiv, terms, flags), f, pdf)
        stats += C.check_sample(tag, b, wo, u, flags, impl_sample(wo, u, flags))
        stats += C.check_sample(tag + " grazing", b, gwo, gu, flags, impl_sample(gwo, gu, flags), capped=False)
    return stats


def run_floor(name, impl_sample, label):
    """A directed setting: the sampling check alone, bulk and grazing directions, no cap (bsdf_cases.run_floor)."""
    b = truth(name)
    wo, _, u, n = inputs(name)
    gwo, gu = C.grazing_inputs("disney", name)
    stats = []
    for fname, flags in C.FLAG_SETS:
        tag = "%s disney/%s %s" % (label, name, fname)
        stats += C.check_sample(tag, b, wo[:4000], u[:4000], flags, impl_sample(wo[:4000], u[:4000], flags), capped=False)
        stats += C.check_sample(tag + " grazing", b, gwo, gu, flags, impl_sample(gwo, gu, flags), capped=False)
    return stats


@functools.lru_cache(maxsize=None)
def calibration(name):
    """The float32 restatement's own Stats, by `what` without the label: the medians the device is held to 4 x of."""
    r = D.Restatement32(params(name))
    st = run_floor(name, r.sample, "f32") if name in FLOOR_SETTINGS else run_setting(name, r.eval, r.sample, "f32")
    return {s.what[4:]: s for s in st}


def hold_caps_and_medians(stats, name, label, capped=True):
    cal = calibration(name)
    for s in stats:
        print(s)
        assert not capped or s.left <= C.MAX_LEFT_OUT, (s.what, "left out", s.left)
        ref = cal[s.what[len(label) + 1:]]
        assert s.median <= C.MEDIAN_FACTOR * ref.median, (s.what, "median err / bound", s.median, "float32 restatement", ref.median)


# ---- one estimate_direct (core/integrator/sample_lights.rs:330-455) at a Disney surface whose normal is the z axis, under a constant
# environment L = 1 with the identity transform, by quadrature in float64: the moments test_gpu_disney.py holds the path integrator's
# BSDF-sampling leg to.  f and the REPORTED pdf sp (the average over the list, with DisneyDiffuse's 0 and the clearcoat's sum) come from
# disney_ref; the expectation of the BSDF half is taken over the TRUE density of each lobe pick:
#   DisneyDiffuse          the pick returns None (pdf 0): it contributes 0 with probability 1 / m
#   Retro, Sheen, FakeSS   cosine_sample_hemisphere: cos / pi
#   MicrofacetReflection   the visible-normal density, which is the pdf the lobe reports
#   DisneyClearcoat        wh drawn from gtr1(cos_h) cos_h (the inversion cos^2 = (1 - alpha2^(1 - u)) / (1 - alpha2) of its sample_f),
#                          so wi has gtr1(cos_h) cos_h / (4 |wo . wh|) -- not the sum the lobe reports
# Light half: wi ~ lp = 1 / (2 pi^2 sin theta) over the sphere (infinite.rs pdf_li with a constant map), contributes
# A = f cos lp / (lp^2 + sp^2); BSDF half: B = f cos sp / (sp^2 + lp^2).  The two halves draw from separate sample dimensions.
# Grid: polar coordinates about the mirror direction of wo, the polar angle alpha = pi t^3 so that the clearcoat's peak (alpha 0.02) gets
# some forty midpoints across; the lower hemisphere contributes nothing (the settings it serves have reflection lobes only).
MIS_FOV = 20.0


def _mis_at(b, theta_o, na, nb, repaired):
    from aov_ref import E
    m = len(b.lobes)
    assert all(l.type & D.R.REFL for l in b.lobes), "reflection lobes only"
    so, co = np.sin(theta_o), np.cos(theta_o)
    r, e1 = np.array([-so, 0.0, co]), np.array([co, 0.0, so])
    t = (np.arange(na) + 0.5) / na
    al, w_al = np.pi * t ** 3, np.pi * 3.0 * t ** 2 / na
    be = 2.0 * np.pi * (np.arange(nb) + 0.5) / nb
    A_, B_ = np.meshgrid(al, be, indexing="ij")
    dw = (np.sin(A_) * w_al[:, None] * (2.0 * np.pi / nb)).reshape(-1)
    wi = (np.cos(A_)[..., None] * r + np.sin(A_)[..., None] * (np.cos(B_)[..., None] * e1 + np.sin(B_)[..., None] * np.array([0.0, 1.0, 0.0]))).reshape(-1, 3)
    up = wi[:, 2] > 1e-6
    wi, dw = wi[up], dw[up]
    n = len(wi)
    wo_e = [E(np.full(n, c)) for c in (so, 0.0, co)]
    wi_e = [E(wi[:, k].copy()) for k in range(3)]
    v = b.eval(wo_e, wi_e, D.R.NOSPEC)
    cos = wi[:, 2]
    f, sp = v.f, v.pdf
    if repaired:                                   # what a repaired reference would report: DisneyDiffuse's pdf as pdf_default's
        sp = sp + cos / np.pi / m
    lp = 1.0 / (2.0 * np.pi * np.pi * np.sqrt(np.maximum(1.0 - cos * cos, 1e-24)))
    wh = wi + np.array([so, 0.0, co])
    wh /= np.linalg.norm(wh, axis=1, keepdims=True)
    q = np.zeros(n)
    for l in b.lobes:
        if l.kind in ("d_retro", "d_sheen", "d_fakess"):
            q += cos / np.pi
        elif l.kind == "mf_r":
            q += D.R.lobe_pdf(l, wo_e, wi_e, np.zeros(n, bool)).v
        elif l.kind == "d_clearcoat":
            q += D.gtr1(E(wh[:, 2].copy()), l.gloss).v * wh[:, 2] / (4.0 * np.abs(wh @ np.array([so, 0.0, co])))
    q /= m
    with np.errstate(all="ignore"):
        A = f * (cos * lp / (lp * lp + sp * sp))[:, None]
        B = np.where((sp > 0)[:, None], f * (cos * sp / (sp * sp + lp * lp))[:, None], 0.0)
    ea, ea2 = ((lp * dw)[:, None] * A).sum(0), ((lp * dw)[:, None] * A * A).sum(0)
    eb, eb2 = ((q * dw)[:, None] * B).sum(0), ((q * dw)[:, None] * B * B).sum(0)
    return ea, eb, (ea2 - ea * ea) + (eb2 - eb * eb), float((q * dw).sum())


@functools.lru_cache(maxsize=None)
def mis_moments(name, repaired=False, n_theta=7, na=480, nb=160, res=64):
    """(mean, variance) per channel of one estimate_direct averaged over a res x res film of MIS_FOV degrees looking straight down the
    normal: the per-direction moments on n_theta values of theta_o (they depend on nothing else: the settings are isotropic and the
    environment is constant), interpolated over the film's pixel centres.  The variance is that of one sample drawn anywhere on the film."""
    b = truth(name)
    assert float(b.info["ax"].v) == float(b.info["ay"].v), "isotropic settings only"
    tan_h = np.tan(np.radians(MIS_FOV / 2))
    th = np.linspace(0.0, np.arctan(np.sqrt(2.0) * tan_h), n_theta)
    rows = [_mis_at(b, t, na, nb, repaired) for t in th]
    s = ((np.arange(res) + 0.5) / res * 2.0 - 1.0) * tan_h
    th_pix = np.arctan(np.hypot(*np.meshgrid(s, s))).reshape(-1)
    mean_pix = np.stack([np.interp(th_pix, th, [r[0][c] + r[1][c] for r in rows]) for c in range(3)], 1)
    var_pix = np.stack([np.interp(th_pix, th, [r[2][c] for r in rows]) for c in range(3)], 1)
    return mean_pix.mean(0), var_pix.mean(0) + mean_pix.var(0)
