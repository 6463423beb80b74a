"""The device's BSDF layer held to the float64 truth of tests/bsdf_ref.py with no oracle on its side: pt_bsdf_eval / pt_bsdf_sample per
material setting and flag set (tests/bsdf_cases.py: eval within bound, sampled type and None decisions, sampled wi within bound, the
returned f and pdf at the returned wi, left-out shares under 3 %, medians within 4 x the float32 restatement's), and one rendered
observable: a quad that cannot see itself under a distant light renders f(wo, wi) L |cos| per camera sample, with f from the truth on
the frame the truth computes from the quad's positions and uvs -- through k_shade_delta / k_shade_delta_inst, which the hooks do not run.

BSDF_TRUTH_WRITE=1 prints the lines of profiles/bsdf_truth.txt."""
import os

import numpy as np
import pytest

import bsdf_cases as C
import bsdf_ref as R
import delta_light_ref as dref
from aov_ref import E
from helpers import scenes
from test_gpu_delta_light import EPS, P_ERR, Run, add_distant, base, check_closed_form, delta_terms, plane_hit

pytestmark = pytest.mark.gpu


def report(label, case, setting, stats):
    if os.environ.get("BSDF_TRUTH_WRITE"):
        print("\n" + C.summary(label, case, setting, stats))


@pytest.fixture(autouse=True)
def counters_left_clean(gpu_ctx):
    """The context is the session's: tests after this file read its counters without resetting them first."""
    yield
    gpu_ctx.reset_counters()


@pytest.fixture
def hooks(gpu_ctx):
    """The context is shared with the lit-quad tests and the rest of the session: every hook test uploads the material table itself."""
    sd = C.scene()
    gpu_ctx.upload(sd)
    return gpu_ctx, sd


# ------------------------------------------------------------------------------------------------------------------ the hooks
@pytest.mark.parametrize("case,setting", C.SETTINGS, ids=["%s-%s" % cs for cs in C.SETTINGS])
def test_device_meets_the_truth(hooks, case, setting):
    ctx, sd = hooks
    mat = sd.material_index[(case, setting)]
    stats = C.run_setting(case, setting, lambda wo, wi, fl: ctx.bsdf_eval(mat, wo, wi, fl), lambda wo, u, fl: ctx.bsdf_sample(mat, wo, u, fl), "gpu")
    report("gpu", case, setting, stats)
    C.hold_caps_and_medians(stats, case, setting, "gpu")


@pytest.mark.parametrize("setting", list(C.FLOOR_CASES))
def test_device_alpha_floor_is_held_through_the_sampling_check(hooks, setting):
    ctx, sd = hooks
    mat = sd.material_index[("floor", setting)]
    stats = C.run_floor(setting, lambda wo, u, fl: ctx.bsdf_sample(mat, wo, u, fl), "gpu")
    report("gpu", "floor", setting, stats)
    C.hold_caps_and_medians(stats, "floor", setting, "gpu", capped=False)
    assert sum(s.n for s in stats if "(c) f" in s.what) > 1000


# ------------------------------------------------------------------------------------------------------------------ the lit quad
QUAD = (-2.0, 2.0, -2.0, 2.0)
UV_X = [0, 0, 1, 0, 1, 1, 0, 1]                 # dpdu along +x
UV_ROT = [0, 0, 0, 1, -1, 1, -1, 0]             # the same uvs turned by 90 degrees: dpdu along +y
CAM_ABOVE, CAM_BELOW = (0, -4, 3), (0, -4, -3)
LIGHT = dict(frm=(0.2, 3.0, 2.5))               # above and beyond the quad: its mirror image and what the quad transmits both head for a camera

LIT = {
    # name: (parameters, camera, what must be reached)
    "plastic": (dict(type="plastic", Kd=(0.3, 0.2, 0.1), Ks=(0.4, 0.5, 0.6), roughness=0.3), CAM_ABOVE),
    "metal_aniso": (dict(type="metal", eta=C.CU_ETA, k=C.CU_K, uroughness=0.15, vroughness=0.6), CAM_ABOVE),
    "substrate_aniso": (dict(type="substrate", Kd=(0.1, 0.3, 0.4), Ks=(0.5, 0.4, 0.3), uroughness=0.15, vroughness=0.6), CAM_ABOVE),
    "uber_kr": (dict(type="uber", Kd=(0.3, 0.2, 0.5), Ks=(0.2, 0.3, 0.1), Kr=(0.3, 0.4, 0.5), eta=1.4, roughness=0.3), CAM_ABOVE),
    "translucent": (dict(type="translucent", Kd=(0.3, 0.25, 0.2), Ks=(0.2, 0.3, 0.25), reflect=(0.5, 0.6, 0.4), transmit=(0.4, 0.3, 0.6),
                         roughness=0.4), CAM_BELOW),
    "rough_glass": (dict(type="glass", Kr=(0.9, 0.8, 0.7), Kt=(0.6, 0.7, 0.8), eta=1.5, uroughness=0.4, vroughness=0.6), CAM_BELOW),
}
ROWS = [("plastic", "x", "plain"), ("metal_aniso", "x", "plain"), ("metal_aniso", "rot", "plain"), ("substrate_aniso", "x", "plain"),
        ("substrate_aniso", "rot", "plain"), ("uber_kr", "x", "plain"), ("translucent", "x", "plain"), ("rough_glass", "rot", "plain"),
        ("plastic", "x", "textured"), ("plastic", "rot", "instance")]


def quad_frame(uv):
    """Triangle::intersect's frame for the quad's first triangle (triangle.rs:349-449, :132-186): ng = ns = normalize(cross(dp02, dp12))
    with no N given, dpdu from the uv differences; then BSDF::new (bsdf.rs:40-53): ss = normalize(dpdu), ts = cross(ns, ss).  The quad's
    two triangles are coplanar and its uvs affine, so both have this frame."""
    x0, x1, y0, y1 = QUAD
    p = np.array([[x0, y0, 0.0], [x1, y0, 0.0], [x1, y1, 0.0]])
    t = np.array(uv, np.float64).reshape(4, 2)[:3]
    dp02, dp12 = p[0] - p[2], p[1] - p[2]
    duv02, duv12 = t[0] - t[2], t[1] - t[2]
    det = duv02[0] * duv12[1] - duv02[1] * duv12[0]
    dpdu = (duv12[1] * dp02 - duv02[1] * dp12) / det
    ns = np.cross(dp02, dp12)
    ns /= np.linalg.norm(ns)
    ss = dpdu / np.linalg.norm(dpdu)
    return ss, np.cross(ns, ss), ns


def lit_scene(name, uvs, route, integ, sampler):
    p, cam = LIT[name]
    sb = base("path" if integ == "path" else "all", sampler, maxdepth=1 if integ == "path" else 5)
    sb.look_at(cam, (0, 0, 0), (0, 0, 1))
    uv = UV_X if uvs == "x" else UV_ROT
    pts = [QUAD[0], QUAD[2], 0.0, QUAD[1], QUAD[2], 0.0, QUAD[1], QUAD[3], 0.0, QUAD[0], QUAD[3], 0.0]
    if route == "textured":                      # "roughness" bound to an image map of one value: the lobes are built on the device at the hit
        img = np.full((4, 4, 1), p["roughness"], np.float32)
        C.apply(sb, dict(p, roughness=sb.texture_imagemap(sb.image_pyramid(img))))
    else:
        C.apply(sb, p)
    if route == "instance":
        sb.object_begin("q")                     # the quad built half a unit away and brought back by the instance's transform
        off = [0.5, -0.25, 0.25]
        sb.shape_trianglemesh([c - off[i % 3] for i, c in enumerate(pts)], [0, 1, 2, 0, 2, 3], uv=uv)
        sb.object_end()
        sb.object_instance("q", to_world=scenes.transform_translate(*off))
    else:
        sb.shape_trianglemesh(pts, [0, 1, 2, 0, 2, 3], uv=uv)
    add_distant(sb, **LIGHT)
    return sb.build()


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("integ", ["path", "all"])
@pytest.mark.parametrize("name,uvs,route", ROWS, ids=["%s-%s-%s" % r for r in ROWS])
def test_lit_quad_renders_the_truths_f(gpu_ctx, name, uvs, route, integ, sampler):
    """Per camera sample the radiance is f(wo, wi) L |cos| with the truth's f on the quad's frame, over its non-specular lobes (next-event
    estimation leaves the specular ones out: uber's Kr changes nothing).  The camera behind the quad reaches the transmission lobes."""
    run = Run(gpu_ctx, lit_scene(name, uvs, route, integ, sampler))
    p, hit, edge = plane_hit(run.o, run.d, 0.0, QUAD, P_ERR)
    ss, ts, ns = quad_frame(UV_X if uvs == "x" else UV_ROT)
    b = R.BSDF(LIT[name][0], np.float64)
    n = len(p)
    d = run.d / np.linalg.norm(run.d, axis=1, keepdims=True)
    # wo = -d of a float32 unit vector (known to 2 roundings of its length), brought to the frame by three dot products on exact axes
    wo = [E(-(d @ a), 6 * EPS) for a in (ss, ts, ns)]
    state = {}

    def brdf(wi_w):
        wi_err = state["wi_err"]
        wi = [E(wi_w @ a, wi_err + 4 * EPS) for a in (ss, ts, ns)]
        v = b.eval(wo, wi, R.NOSPEC)
        state["v"] = v
        return v.f
    lt = run.lights[0]
    state["wi_err"] = dref.sample_li(lt, p, P_ERR)["wi_err"]
    (c, rel, near, lit), = delta_terms(run, p, brdf=brdf)
    v = state["v"]
    with np.errstate(all="ignore"):
        f_rel = np.where(v.f > 0, v.f_e / v.f, 0.0).max(1)
    wide = v.left_out()
    want = np.where(hit[:, None], c, 0.0)
    skip = edge | (hit & (near | wide))
    n_lit, n_zero = check_closed_form(run, want, rel + f_rel + 2 * EPS, skip)
    assert n_lit > 300, n_lit
    assert len(np.unique(np.round(want[hit & ~skip], 6), axis=0)) > 50          # f varies over the film: not one constant
