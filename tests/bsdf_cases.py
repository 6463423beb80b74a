"""The cases of the BSDF truths (tests/bsdf_ref.py): every material kind with its settings, the drawn and the directed inputs, and the
comparison of an implementation's pt_bsdf_eval / pt_bsdf_sample (or orc_*) outputs against the float64 truth.  Shared by
test_bsdf_truth_oracle.py (the float32 run of the restatement and the oracle, no GPU) and test_gpu_bsdf_truth.py (the device).

Colours are non-grey with three distinguishable channels and one negative component where the reference clamps.  The bulk draws keep
|cos| >= COS_MIN and alpha >= 0.02, so that the restatement's own float32 run stays under MAX_LEFT_OUT; grazing directions and
alpha = 0.001 are directed cases held through the sampling check (c) only, where the bound is whatever the evaluation gives."""
import functools

import numpy as np

import bsdf_ref as R
from helpers import scenes

MAX_LEFT_OUT = 0.03
MEDIAN_FACTOR = 4.0
COS_MIN = 2e-3
N_BULK = 10000
FLAG_SETS = (("all", R.ALL), ("nospec", R.NOSPEC), ("refl", R.REFL_ONLY))

CU_ETA, CU_K = (0.2, 0.92, 1.1), (3.9, 2.45, 2.14)
# case -> setting -> parameters, named as the scene description names them ("type" = the Material's name)
CASES = {
    "matte": {
        "lambert": dict(type="matte", Kd=(0.6, 0.45, 0.3)),
        "oren_5": dict(type="matte", Kd=(0.6, 0.45, 0.3), sigma=5.0),
        "oren_25": dict(type="matte", Kd=(0.3, 0.5, 0.7), sigma=25.0),
        "oren_90": dict(type="matte", Kd=(0.7, 0.2, 0.4), sigma=120.0),          # clamped to 90
    },
    "plastic": {
        "remap": dict(type="plastic", Kd=(0.3, -0.2, 0.1), Ks=(0.4, 0.5, 0.6), roughness=0.15),
        "noremap": dict(type="plastic", Kd=(0.2, 0.3, 0.1), Ks=(0.6, -0.5, 0.4), roughness=0.2, remaproughness=False),
    },
    "mirror": {"mirror": dict(type="mirror", Kr=(0.9, 0.7, -0.8))},
    "glass": {"smooth": dict(type="glass", Kr=(0.9, 0.8, 0.7), Kt=(0.6, 0.7, 0.8), eta=1.5)},
    "rough_glass": {
        "iso": dict(type="glass", Kr=(0.9, 0.8, 0.7), Kt=(0.6, 0.7, 0.8), eta=1.33, uroughness=0.2, vroughness=0.2),
        "aniso": dict(type="glass", Kr=(0.9, 0.8, 0.7), Kt=(0.6, 0.7, 0.8), eta=1.5, uroughness=0.1, vroughness=0.4),
        "kr_only": dict(type="glass", Kr=(0.9, 0.8, 0.7), Kt=(0.0, 0.0, 0.0), eta=1.5, uroughness=0.15, vroughness=0.15),
        "kt_only": dict(type="glass", Kr=(0.0, 0.0, 0.0), Kt=(0.6, 0.7, 0.8), eta=1.5, uroughness=0.05, vroughness=0.08, remaproughness=False),
    },
    "metal": {
        "iso": dict(type="metal", eta=CU_ETA, k=CU_K, roughness=0.1),
        "aniso_uv": dict(type="metal", eta=CU_ETA, k=CU_K, uroughness=0.05, vroughness=0.4),
        "aniso_vu": dict(type="metal", eta=CU_ETA, k=CU_K, uroughness=0.4, vroughness=0.05),
        "fallback": dict(type="metal", eta=(0.14, 0.37, 1.44), k=(3.98, 2.38, 1.6), roughness=0.3, uroughness=0.05, remaproughness=False),
    },
    "uber": {
        "opaque": dict(type="uber", Kd=(0.3, 0.2, 0.5), Ks=(0.2, 0.3, -0.1), Kr=(0.1, 0.15, 0.2), eta=1.4, roughness=0.1),
        "partly": dict(type="uber", Kd=(0.5, 0.4, 0.3), Ks=(0.3, 0.2, 0.25), opacity=(0.6, 0.7, 0.8), uroughness=0.05, vroughness=0.15),
        "five": dict(type="uber", Kd=(0.3, 0.2, 0.5), Ks=(0.2, 0.3, 0.1), Kr=(0.1, 0.15, -0.2), Kt=(0.25, 0.2, 0.15), opacity=(0.6, 1.2, 0.8),
                     eta=1.4, roughness=0.3, vroughness=0.1),
    },
    "substrate": {
        "iso": dict(type="substrate", Kd=(0.4, 0.2, -0.1), Ks=(0.3, 0.2, 0.1), uroughness=0.1, vroughness=0.1),
        "aniso": dict(type="substrate", Kd=(0.1, 0.3, 0.4), Ks=(0.5, 0.4, 0.3), uroughness=0.05, vroughness=0.3),
    },
    "translucent": {
        "four": dict(type="translucent", Kd=(0.3, 0.25, 0.2), Ks=(0.2, 0.3, 0.25), reflect=(0.5, 0.6, 0.4), transmit=(0.4, -0.3, 0.6), roughness=0.15),
        "lambert_r": dict(type="translucent", Kd=(0.3, 0.25, 0.2), Ks=(0.0, 0.0, 0.0), reflect=(0.5, 0.6, 0.4), transmit=(0.0, 0.0, 0.0)),
        "lambert_t": dict(type="translucent", Kd=(0.3, 0.25, 0.2), Ks=(0.0, 0.0, 0.0), reflect=(0.0, 0.0, 0.0), transmit=(0.4, 0.3, 0.6)),
        "glossy_r": dict(type="translucent", Kd=(0.0, 0.0, 0.0), Ks=(0.2, 0.3, 0.25), reflect=(0.5, 0.6, 0.4), transmit=(0.0, 0.0, 0.0), roughness=0.2),
        "glossy_t": dict(type="translucent", Kd=(0.0, 0.0, 0.0), Ks=(0.2, 0.3, 0.25), reflect=(0.0, 0.0, 0.0), transmit=(0.4, 0.3, 0.6), roughness=0.1,
                         remaproughness=False),
    },
}
# directed: alpha at the 0.001 floor, held through the sampling check (c) only
FLOOR_CASES = {
    "plastic_floor": dict(type="plastic", Kd=(0.2, 0.3, 0.1), Ks=(0.6, 0.5, 0.4), roughness=0.0005, remaproughness=False),
    "glass_floor": dict(type="glass", Kr=(0.9, 0.8, 0.7), Kt=(0.6, 0.7, 0.8), eta=1.5, uroughness=0.001, vroughness=0.0, remaproughness=False),
}
SETTINGS = [(c, s) for c, ss in CASES.items() for s in ss]


def params(case, setting):
    return FLOOR_CASES[setting] if case == "floor" else CASES[case][setting]


def apply(sb, p):
    kw = {k: v for k, v in p.items() if k != "type"}
    getattr(sb, "material_" + p["type"])(**kw)
    return sb.cur_material


@functools.lru_cache(maxsize=None)
def scene():
    """One small triangle per setting: the scene only carries the material table for the BSDF hooks."""
    sb = scenes.SceneBuilder()
    sb.look_at((0, -4, 3), (0, 0, 0), (0, 0, 1))
    sb.camera_perspective(fov=50.0)
    sb.film(xresolution=8, yresolution=8)
    sb.pixel_filter_box()
    sb.sampler_sobol(pixelsamples=1)
    sb.integrator_path(maxdepth=1)
    index = {}
    for k, (c, s) in enumerate(SETTINGS + [("floor", s) for s in FLOOR_CASES]):
        index[(c, s)] = apply(sb, params(c, s))
        x = -2.0 + 0.1 * k
        sb.shape_trianglemesh([x, 0, 0, x + 0.05, 0, 0, x, 0.05, 0], [0, 1, 2])
    sb.light_distant(L=(1, 1, 1), frm=(0, 0, 1), to=(0, 0, 0))
    sd = sb.build()
    sd.material_index = index
    return sd


def sphere_dirs(rng, n):
    """Uniform on the sphere with |cos| >= COS_MIN (the band is redrawn), as float32 unit vectors."""
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    while True:
        bad = np.abs(v[:, 2]) < COS_MIN
        if not bad.any():
            break
        w = rng.standard_normal((int(bad.sum()), 3))
        v[bad] = w / np.linalg.norm(w, axis=1, keepdims=True)
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(case, setting):
    """(wo, wi, u, n_bulk): N_BULK drawn pairs, then the directed ones -- near-normal wo, the mirror direction, wi = -wo, wi across the
    surface near -wo; wo covers both hemispheres throughout.  All of them count under the cap; the grazing block of the sampling check
    is apart, see grazing_inputs()."""
    rng = np.random.default_rng(sum(ord(c) for c in case + "/" + setting))
    n = N_BULK
    wo, wi = sphere_dirs(rng, n + 500), sphere_dirs(rng, n + 500)          # (n + 100 to n + 200 stay as drawn: a hundred more bulk pairs)
    d = slice(n, n + 100)                                              # near-normal incidence (sample_11's special case), both sides:
    r = 10.0 ** rng.uniform(np.log10(3e-3), np.log10(1.5e-2), 100)      # sin(theta_o) between 3e-3 and 1.5e-2
    wo[d, :2] *= (r / np.linalg.norm(wo[d, :2].astype(np.float64), axis=1))[:, None].astype(np.float32)
    wo[d, 2] = np.sign(wo[d, 2])
    wo[d] /= np.linalg.norm(wo[d].astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    m = slice(n + 200, n + 350)
    wi[m] = wo[m] * np.array([-1, -1, 1], np.float32)                  # the mirror direction
    o = slice(n + 350, n + 400)
    wi[o] = -wo[o]                                                     # wh = 0
    t = slice(n + 400, n + 500)
    wi[t] = -wo[t]
    wi[t, :2] *= np.float32(0.5)                                       # straight through, bent: the transmission lobes' neighbourhood
    wi[t] /= np.linalg.norm(wi[t].astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    u = rng.random((n + 500, 2)).astype(np.float32)
    return wo, wi, u, n


@functools.lru_cache(maxsize=None)
def grazing_inputs(case, setting):
    """The directed grazing block of the sampling check: 300 wo at |cos| between 1e-5 and 1e-3, and u at the ends of [0, 1)."""
    rng = np.random.default_rng(7 + sum(ord(c) for c in case + "/" + setting))
    wo = sphere_dirs(rng, 300)
    wo[:, 2] = np.sign(wo[:, 2]) * (10.0 ** rng.uniform(-5, -3, 300)).astype(np.float32)
    wo /= np.linalg.norm(wo.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    u = rng.random((300, 2)).astype(np.float32)
    u[:20, 0] = 0.0
    u[20:40, 1] = 0.0
    u[40:60, 0] = np.float32(0.99999994)
    return wo, u


# ------------------------------------------------------------------------------------------------------------------ comparison
class Stat:
    """err / bound of one comparison: the share left out, the worst and the median ratio over what was held."""

    def __init__(self, what, left, ratio, n):
        self.what, self.n = what, n
        self.left = float(left)
        self.worst = float(ratio.max()) if len(ratio) else 0.0
        self.median = float(np.median(ratio)) if len(ratio) else 0.0

    def __str__(self):
        return "%s n %d left out %.4f worst %.3f median %.4f" % (self.what, self.n, self.left, self.worst, self.median)


def _ratio(got, want, bound):
    """|got - want| / bound where the bound is positive; a zero bound is a decided value: got must equal it."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    exact = bound == 0
    assert np.array_equal(got[exact], want[exact]), ("a decided value is not met", int((got[exact] != want[exact]).sum()))
    with np.errstate(all="ignore"):
        return np.abs(got - want)[~exact] / bound[~exact]


def hold(what, got, want, bound, keep):
    """The values kept are within their bound; returns the ratios."""
    keep = keep if got.ndim == 1 else np.repeat(keep[:, None], got.shape[1], 1)
    r = _ratio(got[keep], want[keep], bound[keep])
    assert (r <= 1.0).all(), (what, "err / bound", float(r.max()), int((r > 1.0).sum()), int(keep.sum()))
    return r


def check_eval(tag, truth, f, pdf, n_capped=None):
    """4. `eval`: f and pdf within bound of the truth (exactly 0 where the truth is a decided 0) outside the left-out evaluations."""
    out = truth.left_out()
    keep = ~out
    rf = hold(tag + " f", np.asarray(f, np.float64), truth.f, truth.f_e, keep)
    rp = hold(tag + " pdf", np.asarray(pdf, np.float64), truth.pdf, truth.pdf_e, keep)
    n = len(out) if n_capped is None else n_capped
    share = out[:n].mean() if n else 0.0
    return [Stat(tag + " eval f", share, rf, int(keep.sum())), Stat(tag + " eval pdf", share, rp, int(keep.sum()))]


def check_sample(tag, bsdf, wo, u, flags, got, capped=True):
    """4. `sample` (a), (b), (c) of one implementation's (f, wi, pdf, type) against the float64 sampler `bsdf`."""
    f, wi, pdf, typ = [np.asarray(a) for a in got]
    s = bsdf.sample(wo, u, flags)
    dec = ~s["und"]
    # (a) the sampled type and the None decisions
    bad = dec & (typ != s["type"])
    assert not bad.any(), (tag, "type / None", int(bad.sum()), typ[bad][:4], s["type"][bad][:4])
    # (b) wi within bound of the float64 sampler's; past REL_CAP the sample counts as left out
    some = dec & (s["type"] != 0)
    wide = (s["wi_e"] > R.REL_CAP).any(1) | ~np.isfinite(s["wi_e"]).all(1)
    kb = some & ~wide
    rb = hold(tag + " wi", wi.astype(np.float64), s["wi"], s["wi_e"], kb)
    left = (s["und"] | (some & wide))
    # specular picks: f and pdf are their closed forms at wo
    sp = kb & s["specular"]
    rsf = hold(tag + " specular f", f.astype(np.float64), s["f"], s["f_e"], sp)
    rsp = hold(tag + " specular pdf", pdf.astype(np.float64), s["pdf"], s["pdf_e"], sp)
    # (c) every returned non-specular sample: the implementation's own wi as an exact input
    ret = (typ != 0) & ((typ & R.SPECULAR) == 0)
    stats = [Stat(tag + " sample wi", left.mean() if capped else 0.0, rb, int(kb.sum())),
             Stat(tag + " sample specular f", 0.0, np.concatenate([rsf, rsp]), int(sp.sum()))]
    if ret.any():
        idx = np.flatnonzero(ret)
        pick = np.where(s["und"][idx], -1, s["pick"][idx])
        at = bsdf.eval_at_sampled(wo[idx], wi[idx], pick, flags)
        if (s["und"][idx]).any():                                      # the pick is not known: any lobe may be the half-vector one
            j = np.flatnonzero(s["und"][idx])
            mf = [i for i, l in enumerate(bsdf.lobes) if l.kind == "mf_r" and l.matches(flags)]
            if mf:
                w = bsdf.eval_at_sampled(wo[idx][j], wi[idx][j], np.full(len(j), mf[0]), flags)
                at.pdf_e[j] = np.maximum(at.pdf_e[j], w.pdf_e) + np.abs(at.pdf[j] - w.pdf)
                at.und[j] |= w.und
        ok = ~at.und & np.isfinite(at.f_e).all(1) & np.isfinite(at.pdf_e) & np.isfinite(at.f).all(1) & np.isfinite(at.pdf)
        rcf = hold(tag + " (c) f", f[idx].astype(np.float64), at.f, at.f_e, ok)
        rcp = hold(tag + " (c) pdf", pdf[idx].astype(np.float64), at.pdf, at.pdf_e, ok)
        stats += [Stat(tag + " sample (c) f", (~ok).mean() if capped else 0.0, rcf, int(ok.sum())),
                  Stat(tag + " sample (c) pdf", (~ok).mean() if capped else 0.0, rcp, int(ok.sum()))]
    return stats


def summary(label, case, setting, stats):
    """One line of profiles/bsdf_truth.txt: per quantity the worst and the largest median err / bound over the three flag sets, and the
    largest share left out (the grazing block, which has no cap, is reported apart by its (c) figures)."""
    def agg(key, grazing=False):
        sel = [s for s in stats if s.what.endswith(key) and (" grazing " in s.what) == grazing and s.n]
        return "%s worst %.3f median %.4f" % (key, max(s.worst for s in sel), max(s.median for s in sel)) if sel else "%s -" % key
    left = max(s.left for s in stats)
    keys = ["eval f", "eval pdf", "sample wi", "sample specular f", "sample (c) f", "sample (c) pdf"]
    return "%-3s %-24s left out %.4f | %s | grazing: %s | %s" % (label, case + "/" + setting, left, " | ".join(agg(k) for k in keys if case != "floor" or "eval" not in k),
                                                                agg("sample (c) f", True), agg("sample (c) pdf", True))


class Restatement32:
    """The float32 run of the restatement behind the hooks' interface: the calibration, and an implementation like the others."""

    def __init__(self, p):
        self.b = R.BSDF(p, np.float32)

    def eval(self, wo, wi, flags):
        v = self.b.eval(wo, wi, flags)
        return v.f.astype(np.float32), v.pdf.astype(np.float32)

    def sample(self, wo, u, flags):
        s = self.b.sample(wo, u, flags)
        f, pdf = s["f"], s["pdf"]
        return f.astype(np.float32), s["wi"].astype(np.float32), pdf.astype(np.float32), s["type"]


@functools.lru_cache(maxsize=None)
def truth(case, setting):
    return R.BSDF(params(case, setting), np.float64)


def run_setting(case, setting, impl_eval, impl_sample, label):
    """All of section 4 for one setting and every flag set: a list of Stat.  impl_eval(wo, wi, flags) -> (f, pdf);
    impl_sample(wo, u, flags) -> (f, wi, pdf, type)."""
    b = truth(case, setting)
    wo, wi, u, n = inputs(case, setting)
    gwo, gu = grazing_inputs(case, setting)
    stats = []
    wov, wiv, terms = b.terms(wo, wi)
    for fname, flags in FLAG_SETS:
        tag = "%s %s/%s %s" % (label, case, setting, fname)
        f, pdf = impl_eval(wo, wi, flags)
        stats += check_eval(tag, b.combine(wov, wiv, terms, flags), f, pdf)
        stats += check_sample(tag, b, wo, u, flags, impl_sample(wo, u, flags))
        stats += check_sample(tag + " grazing", b, gwo, gu, flags, impl_sample(gwo, gu, flags), capped=False)
    return stats


def run_floor(setting, impl_sample, label):
    """alpha = 0.001: the sampling check alone, bulk and grazing directions, no cap."""
    b = truth("floor", setting)
    wo, _, u, n = inputs("floor", setting)
    gwo, gu = grazing_inputs("floor", setting)
    stats = []
    for fname, flags in FLAG_SETS:
        tag = "%s floor/%s %s" % (label, setting, fname)
        stats += check_sample(tag, b, wo[:4000], u[:4000], flags, impl_sample(wo[:4000], u[:4000], flags), capped=False)
        stats += check_sample(tag + " grazing", b, gwo, gu, flags, impl_sample(gwo, gu, flags), capped=False)
    return stats


@functools.lru_cache(maxsize=None)
def calibration(case, setting):
    """The float32 restatement's own Stats for a setting, by `what` without the label: the medians the others are held to 4 x of."""
    r = Restatement32(params(case, setting))
    st = run_floor(setting, r.sample, "f32") if case == "floor" else run_setting(case, setting, r.eval, r.sample, "f32")
    return {s.what[4:]: s for s in st}


def hold_caps_and_medians(stats, case, setting, label, capped=True):
    """capped=False: the directed settings (alpha at its floor), whose shares are reported and not capped; the medians hold all the same."""
    cal = calibration(case, setting)
    for s in stats:
        assert not capped or s.left <= MAX_LEFT_OUT, (s.what, "left out", s.left)
        ref = cal[s.what[len(label) + 1:]]
        assert s.median <= MEDIAN_FACTOR * ref.median, (s.what, "median err / bound", s.median, "float32 restatement", ref.median)
