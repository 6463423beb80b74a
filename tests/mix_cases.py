"""The cases of the Material "mix" truths (tests/mix_ref.py): the trees, how a SceneBuilder is given one, and section 4 of bsdf_cases
(eval, sampled type and None decisions, wi, f / pdf at the returned wi) with the mix truth in the BSDF's place.  Shared by
test_mix_host.py (the float32 run of the restatement, no GPU) and test_gpu_mix.py (the device)."""
import functools

import numpy as np

import bsdf_cases as C
import mix_ref as M
from helpers import pkg, scenes

P = C.params
BLACK = dict(type="matte", Kd=(0.0, 0.0, 0.0))          # Kd black: MatteMaterial adds no BxDF (matte.rs:44-51), the BSDF exists


def mix(m1, m2, amount):
    return dict(type="mix", m1=m1, m2=m2, amount=tuple(amount) if isinstance(amount, (tuple, list)) else (amount,) * 3)


LOBE_CAP = pkg.capi.PT_MIX_MAX_LOBES
# the settings of the hook tests (device and float32 restatement alike)
SETTINGS = {
    "plastic_matte": mix(P("plastic", "remap"), P("matte", "lambert"), 0.3),
    "glass_metal": mix(P("rough_glass", "aniso"), P("metal", "aniso_uv"), (0.2, 0.5, 0.8)),
    "mirror_substrate": mix(P("mirror", "mirror"), P("substrate", "iso"), 0.5),
    "nested": mix(mix(P("matte", "oren_25"), P("plastic", "noremap"), 0.25), P("translucent", "four"), 0.6),           # 1 + 2 + 4 lobes
    "at_cap": mix(mix(P("uber", "five"), dict(P("uber", "five"), Kd=(0.2, 0.4, 0.1), roughness=0.2), 0.4),            # 5 + 5 + 4 + 2 = the cap
                  mix(P("translucent", "four"), P("plastic", "remap"), 0.7), (0.5, 0.35, 0.65)),
    "beyond_01": mix(P("plastic", "remap"), P("matte", "oren_5"), (1.5, -0.25, 0.5)),                                  # s1 not clamped above 1; s2 clamps
}


def n_lobes(tree):
    return len(M.flatten(tree, np.float64))


assert n_lobes(SETTINGS["at_cap"]) == LOBE_CAP and n_lobes(SETTINGS["nested"]) >= 5


def apply(sb, tree):
    """Adds the tree's materials to the builder, children first; returns the root's material index."""
    if tree["type"] != "mix":
        return C.apply(sb, tree)
    m1, m2 = apply(sb, tree["m1"]), apply(sb, tree["m2"])
    sb.material_mix(m1, m2, tree.get("amount", (0.5, 0.5, 0.5)))
    return sb.cur_material


def palette(trees):
    """One small triangle per tree: the scene only carries the material table for the BSDF hooks.  trees: {name: tree}."""
    sb = scenes.SceneBuilder()
    sb.look_at((0, -4, 3), (0, 0, 0), (0, 0, 1))
    sb.camera_perspective(fov=50.0)
    sb.film(xresolution=8, yresolution=8)
    sb.pixel_filter_box()
    sb.sampler_sobol(pixelsamples=1)
    sb.integrator_path(maxdepth=1)
    index = {}
    for k, (name, tree) in enumerate(trees.items()):
        index[name] = apply(sb, tree)
        x = -2.0 + 0.1 * k
        sb.shape_trianglemesh([x, 0, 0, x + 0.05, 0, 0, x, 0.05, 0], [0, 1, 2])
    sb.light_distant(L=(1, 1, 1), frm=(0, 0, 1), to=(0, 0, 0))
    sd = sb.build()
    sd.material_index = index
    return sd


@functools.lru_cache(maxsize=None)
def truth(name):
    return M.BSDF(SETTINGS[name], np.float64)


def inputs(name):
    return C.inputs("mix", name)          # bsdf_cases' generator: N_BULK drawn pairs and its directed ones (the names only seed it)


def run_setting(name, impl_eval, impl_sample, label):
    """bsdf_cases.run_setting with the mix truth: a list of Stat over bsdf_cases.FLAG_SETS."""
    b = truth(name)
    wo, wi, u, n = inputs(name)
    gwo, gu = C.grazing_inputs("mix", name)
    stats = []
    wov, wiv, terms = b.terms(wo, wi)
    for fname, flags in C.FLAG_SETS:
        tag = "%s mix/%s %s" % (label, name, fname)
        f, pdf = impl_eval(wo, wi, flags)
        stats += C.check_eval(tag, b.combine(wov, wiv, terms, flags), f, pdf)
        stats += C.check_sample(tag, b, wo, u, flags, impl_sample(wo, u, flags))
        stats += C.check_sample(tag + " grazing", b, gwo, gu, flags, impl_sample(gwo, gu, flags), capped=False)
    return stats


@functools.lru_cache(maxsize=None)
def calibration(name):
    """The float32 restatement's own Stats, by `what` without the label."""
    r = M.Restatement32(SETTINGS[name])
    return {s.what[4:]: s for s in run_setting(name, r.eval, r.sample, "f32")}


def hold_caps_and_medians(stats, name, label):
    cal = calibration(name)
    for s in stats:
        print(s)
        assert s.left <= C.MAX_LEFT_OUT, (s.what, "left out", s.left)
        ref = cal[s.what[len(label) + 1:]]
        assert s.median <= C.MEDIAN_FACTOR * ref.median, (s.what, "median err / bound", s.median, "float32 restatement", ref.median)


# ---- the lit quad whose "amount" is a checkerboard (test_gpu_mix.py): amounts per cell, cells per uv unit, and how near a cell edge a
# sample's cell is not decided.  The hit point is known to p_err (plane_hit's bound), the quad is `width` wide, so u = (x - x0) / width is
# known to p_err / width plus three float32 roundings of values <= 1 (the uv interpolation), and s = scale * u to scale times that plus one.
LIT_AMOUNTS = ((0.85, 0.7, 0.9), (0.1, 0.25, 0.15))
LIT_SCALE = 4.0


def lit_uv_margin(p_err, width):
    return LIT_SCALE * (p_err / width + 3 * 2.0 ** -24) + LIT_SCALE * 2.0 ** -24
