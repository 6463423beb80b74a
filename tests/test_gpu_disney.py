"""Material "disney" on the device (materials/disney.rs).

The hooks are held to the float64 truth tests/disney_ref.py with bsdf_cases' checks, and bit for bit to the device's own evaluations
through a mix.  The rendering kernels of a scene with a Disney material (the _mix family of the build that knows Disney's BxDFs) are held
per pixel to the closed form f Li |cos| with the truth's f, constant and per-hit, and bit for bit to one another: mix(D, matte(Kd 0), 1)
scales D's lobes by exactly 1 and adds nothing."""
import os
import subprocess

import numpy as np
import pytest

import bsdf_cases as C
import bsdf_ref as R
import delta_light_ref as dref
import disney_cases as DC
import disney_ref as D
import feature_scenes as fs
from aov_ref import E
from helpers import bits, pkg, scenes
from test_gpu_bsdf_truth import LIGHT, QUAD, UV_X, CAM_ABOVE, CAM_BELOW, quad_frame
from test_gpu_delta_light import EPS, P_ERR, Run, add_distant, base, check_closed_form, delta_terms, plane_hit
from test_gpu_translucent import INTEGRATORS, RAY_COUNTERS, assert_same_render, hook_inputs, render_everything, room_scene

pytestmark = pytest.mark.gpu
capi = pkg.capi
f32 = np.float32
Z3, O3 = (0.0,) * 3, (1.0,) * 3
FLAGS = [fl for _, fl in C.FLAG_SETS]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def counters_left_clean(gpu_ctx):
    yield
    gpu_ctx.reset_counters()


def with_black_mix(sb, p):
    """mix(D, matte(Kd 0), amount 1): D's lobes scaled by exactly 1, through a mix tree."""
    d = DC.apply(sb, p)
    sb.material_matte(Kd=Z3)
    sb.material_mix(d, sb.cur_material, O3)
    return sb.cur_material


# ---------------------------------------------------------------- 1. hooks against the truth
@pytest.mark.parametrize("name", list(DC.SETTINGS))
def test_hooks_meet_the_truth(gpu_ctx, name):
    sd = DC.palette()
    gpu_ctx.upload(sd)
    mat = sd.material_index[name]
    stats = DC.run_setting(name, lambda wo, wi, fl: gpu_ctx.bsdf_eval(mat, wo, wi, fl), lambda wo, u, fl: gpu_ctx.bsdf_sample(mat, wo, u, fl), "gpu")
    DC.hold_caps_and_medians(stats, name, "gpu")


@pytest.mark.parametrize("name", list(DC.FLOOR_SETTINGS))
def test_hooks_meet_the_truth_at_the_floors(gpu_ctx, name):
    """clearcoatgloss 1 (alpha 0.001) and roughness 0 (the 0.001 floor): the sampling check alone, uncapped."""
    sd = DC.palette()
    gpu_ctx.upload(sd)
    mat = sd.material_index[name]
    stats = DC.run_floor(name, lambda wo, u, fl: gpu_ctx.bsdf_sample(mat, wo, u, fl), "gpu")
    DC.hold_caps_and_medians(stats, name, "gpu", capped=False)


# ---------------------------------------------------------------- 2. hooks, bit for bit, device against device
def _pairs_palette(names, extra=None):
    sb = scenes.SceneBuilder()
    sb.look_at((0, -4, 3), (0, 0, 0), (0, 0, 1))
    sb.camera_perspective(fov=50.0)
    sb.film(xresolution=8, yresolution=8)
    sb.pixel_filter_box()
    sb.sampler_sobol(pixelsamples=1)
    sb.integrator_path(maxdepth=1)
    index = {}
    k = 0

    def tri():
        nonlocal k
        x = -2.0 + 0.1 * k
        k += 1
        sb.shape_trianglemesh([x, 0, 0, x + 0.05, 0, 0, x, 0.05, 0], [0, 1, 2])
    for name in names:
        index[name] = DC.apply(sb, DC.params(name)); tri()
        index[name + "/mix"] = with_black_mix(sb, DC.params(name)); tri()
    if extra:
        extra(sb, index, tri)
    sb.light_distant(L=(1, 1, 1), frm=(0, 0, 1), to=(0, 0, 0))
    sd = sb.build()
    sd.material_index = index
    return sd


def test_hooks_lobeless_sibling_leaves_the_material(gpu_ctx):
    """mix(D, matte(Kd 0), amount 1) returns what D returns: f, pdf and all four outputs of sample_f, every setting and flag set."""
    names = list(DC.SETTINGS) + list(DC.FLOOR_SETTINGS)
    sd = _pairs_palette(names)
    gpu_ctx.upload(sd)
    ix = sd.material_index
    wo, wi, u = hook_inputs(np.random.default_rng(61))
    for k in names:
        for fl in FLAGS:
            ea, em = gpu_ctx.bsdf_eval(ix[k], wo, wi, fl), gpu_ctx.bsdf_eval(ix[k + "/mix"], wo, wi, fl)
            assert np.array_equal(bits(ea[0]), bits(em[0])) and np.array_equal(bits(ea[1]), bits(em[1])), (k, fl)
            sa, sm = gpu_ctx.bsdf_sample(ix[k], wo, u, fl), gpu_ctx.bsdf_sample(ix[k + "/mix"], wo, u, fl)
            assert np.array_equal(sa[3], sm[3]), (k, fl, "type")
            for j in range(3):
                assert np.array_equal(bits(sa[j]), bits(sm[j])), (k, fl, j)
        assert (gpu_ctx.bsdf_eval(ix[k], wo, wi, R.ALL)[0] != 0).any(), k


def test_hooks_compose_the_childrens_own_evaluations(gpu_ctx):
    """mix(D, matte, amount) with D = `glass`, whose two lobes lie on opposite sides, so that at most one of them enters f at any pair of
    directions: f_mix = fl32(fl32(s1 f_D) + fl32(s2 f_M)) and pdf_mix = fl32(fl32(n_D p_D + p_M) / (n_D + 1)) with n_D the matching lobes of
    D (n_D p_D is exact for n_D = 1, 2), formed in numpy float32 from the device's evaluations of D and of the matte."""
    amount = (0.3, 0.65, 0.9)
    matte = C.params("matte", "lambert")

    def extra(sb, index, tri):
        index["m"] = C.apply(sb, matte); tri()
        d = DC.apply(sb, DC.params("glass"))
        sb.material_mix(d, index["m"], amount)
        index["mix"] = sb.cur_material; tri()
    sd = _pairs_palette(["glass"], extra)
    gpu_ctx.upload(sd)
    ix = sd.material_index
    wo, wi, u = hook_inputs(np.random.default_rng(62))
    s1 = np.array(amount, f32)
    s2 = (f32(1) - s1).astype(f32)
    for fl in FLAGS:
        n_d = sum(1 for _, t in DC.LOBE_TABLE["glass"] if (t & fl) == t)
        (fa, pa), (fb, pb), (fm, pm) = [gpu_ctx.bsdf_eval(ix[k], wo, wi, fl) for k in ("glass", "m", "mix")]
        want_f = ((s1 * fa).astype(f32) + (s2 * fb).astype(f32)).astype(f32)
        want_p = (((pa * f32(n_d)).astype(f32) + pb).astype(f32) / f32(n_d + 1)).astype(f32)
        ok = np.isfinite(fa).all(1) & np.isfinite(pa)
        assert ok.mean() > 0.9
        assert np.array_equal(bits(fm[ok]), bits(want_f[ok])), fl
        assert np.array_equal(bits(pm[ok]), bits(want_p[ok])), fl
        assert (fm != 0).any()


def test_hooks_scale_every_disney_lobe_by_powers_of_two(gpu_ctx):
    """mix(D, matte(Kd 0), (1/2, 1/4, 1/8)): every lobe of D -- the five new BxDFs among them -- is multiplied by a scale that is not 1.  A
    power of two multiplies exactly and commutes with the roundings of the sum over the lobes (no value here is near the subnormals), so
    f_mix is (1/2, 1/4, 1/8) f_D bit for bit, the spectrum of sample_f likewise, and pdf, wi and type are D's.  (It does not tell a scale
    applied per lobe from one applied to the sum: only the composition test above, with one lobe per side, does.)"""
    amount = (0.5, 0.25, 0.125)
    names = ["sheen", "clearcoat", "thin_all", "half_trans"]           # together: every kind of lobe a Disney list can hold

    def extra(sb, index, tri):
        for name in names:
            d = DC.apply(sb, DC.params(name))
            sb.material_matte(Kd=Z3)
            sb.material_mix(d, sb.cur_material, amount)
            index[name + "/scaled"] = sb.cur_material; tri()
    sd = _pairs_palette(names, extra)
    gpu_ctx.upload(sd)
    ix = sd.material_index
    wo, wi, u = hook_inputs(np.random.default_rng(66))
    s1 = np.array(amount, f32)
    kinds = set()
    for k in names:
        kinds |= {kind for kind, _ in DC.LOBE_TABLE[k]}
        for fl in FLAGS:
            (fa, pa), (fm, pm) = gpu_ctx.bsdf_eval(ix[k], wo, wi, fl), gpu_ctx.bsdf_eval(ix[k + "/scaled"], wo, wi, fl)
            ok = np.isfinite(fa).all(1) & ((np.abs(fa) > 1e-30) | (fa == 0)).all(1)
            assert ok.mean() > 0.9
            assert np.array_equal(bits(fm[ok]), bits((s1 * fa).astype(f32)[ok])), (k, fl)
            assert np.array_equal(bits(pm), bits(pa)), (k, fl)
            sa, sm = gpu_ctx.bsdf_sample(ix[k], wo, u, fl), gpu_ctx.bsdf_sample(ix[k + "/scaled"], wo, u, fl)
            ok = np.isfinite(sa[0]).all(1) & ((np.abs(sa[0]) > 1e-30) | (sa[0] == 0)).all(1)
            assert np.array_equal(bits(sm[0][ok]), bits((s1 * sa[0]).astype(f32)[ok])), (k, fl, "f")
            assert np.array_equal(bits(sm[1]), bits(sa[1])) and np.array_equal(bits(sm[2]), bits(sa[2])) and np.array_equal(sm[3], sa[3]), (k, fl)
        assert (gpu_ctx.bsdf_eval(ix[k + "/scaled"], wo, wi, R.ALL)[0] != 0).any()
    assert kinds == {"d_diffuse", "d_fakess", "d_retro", "d_sheen", "d_clearcoat", "mf_r", "mf_t", "lambert_t"}


# ---------------------------------------------------------------- 3. the sampling quirk on the device
def test_default_samples_nothing_below_one_third(gpu_ctx):
    """diffuse, retro, microfacet: u.x < 1/3 picks DisneyDiffuse, whose pdf is 0 -- type 0 (None) whatever wo and u.y are."""
    sd = DC.palette(["default"])
    gpu_ctx.upload(sd)
    mat = sd.material_index["default"]
    rng = np.random.default_rng(63)
    wo, _, u = hook_inputs(rng)
    u[:, 0] = (rng.integers(0, 1366, len(u)) / 4096.0).astype(f32)          # a 2^-12 grid below 1/3 (1365 / 4096 < 1 / 3)
    f, wi, pdf, t = gpu_ctx.bsdf_sample(mat, wo, u, R.ALL)
    assert (t == 0).all()
    u[:, 0] = (f32(1365) / f32(4096) + rng.integers(6, 2700, len(u)) / 4096.0).astype(f32)          # above: Retro and the microfacet lobe sample
    t = gpu_ctx.bsdf_sample(mat, wo, u, R.ALL)[3]
    assert (t != 0).mean() > 0.8 and set(np.unique(t)) <= {0, R.REFL | R.DIFFUSE, R.REFL | R.GLOSSY}


# ---------------------------------------------------------------- 4. closed form per pixel
def _lit_run(ctx, integ, cam, material):
    sb = base(integ, "sobol", res=16, spp=1, maxdepth=1 if integ == "path" else 5)
    sb.look_at(cam, (0, 0, 0), (0, 0, 1))
    material(sb)
    sb.shape_trianglemesh([QUAD[0], QUAD[2], 0.0, QUAD[1], QUAD[2], 0.0, QUAD[1], QUAD[3], 0.0, QUAD[0], QUAD[3], 0.0], [0, 1, 2, 0, 2, 3], uv=UV_X)
    add_distant(sb, **LIGHT)
    return Run(ctx, sb.build())


def _closed_form(run, select):
    """run.rad against f Li |cos| with f from the truths select(p) -> [(BSDF, mask)] picks per sample; returns (samples held lit, skip, hit).
    Every decided sample is held to its own propagated bound, also where that bound passes bsdf_ref.REL_CAP of f: around the mirror
    direction of a clearcoat of alpha 0.02 the 6 ulp the directions are known to become 2e-3 of f, and that is the part of the film that
    shows the lobe.  Left out: the undecided evaluations and bounds that are not finite."""
    p, hit, edge = plane_hit(run.o, run.d, 0.0, QUAD, P_ERR)
    ss, ts, ns = quad_frame(UV_X)
    d = run.d / np.linalg.norm(run.d, axis=1, keepdims=True)
    wo = [E(-(d @ a), 6 * EPS) for a in (ss, ts, ns)]
    picks, undecided = select(p)
    state = {}

    def brdf(wi_w):
        wi = [E(wi_w @ a, state["wi_err"] + 4 * EPS) for a in (ss, ts, ns)]
        f, f_e, out = np.zeros((len(p), 3)), np.zeros((len(p), 3)), np.zeros(len(p), bool)
        for bsdf, mask in picks:
            v = bsdf.eval(wo, wi, R.NOSPEC)
            bad = v.und | ~np.isfinite(v.f_e).all(1) | ~np.isfinite(v.f).all(1)
            f, f_e, out = np.where(mask[:, None], v.f, f), np.where(mask[:, None], v.f_e, f_e), np.where(mask, bad, out)
        state.update(f=f, f_e=f_e, out=out)
        return f
    state["wi_err"] = dref.sample_li(run.lights[0], p, P_ERR)["wi_err"]
    (c, rel, near, lit), = delta_terms(run, p, brdf=brdf)
    with np.errstate(all="ignore"):
        f_rel = np.where(state["f"] > 0, state["f_e"] / state["f"], 0.0).max(1)
    want = np.where(hit[:, None], c, 0.0)
    skip = edge | (hit & (near | state["out"] | undecided))
    n_lit, n_zero = check_closed_form(run, want, rel + f_rel + 2 * EPS, skip)
    return n_lit, skip, hit


@pytest.mark.parametrize("integ", ["path", "all", "whitted"])
@pytest.mark.parametrize("name", ["default", "clearcoat", "thin_all", "glass"])
def test_lit_quad_renders_the_truths_f(gpu_ctx, name, integ):
    """Per camera sample the radiance is f(wo, wi) L |cos| with disney_ref's f on the quad's frame, within the bound check_closed_form
    derives.  `glass` is lit from behind: the camera below the quad sees what the transmission lobe passes."""
    run = _lit_run(gpu_ctx, integ, CAM_BELOW if name == "glass" else CAM_ABOVE, lambda sb: DC.apply(sb, DC.params(name)))
    truth = DC.truth(name)
    n_lit, skip, hit = _closed_form(run, lambda p: ([(truth, np.ones(len(p), bool))], np.zeros(len(p), bool)))
    assert n_lit > 60, n_lit
    assert skip.mean() <= C.MAX_LEFT_OUT


# ---------------------------------------------------------------- 5. the per-hit route
CHECK_SCALE = 4.0
CELLS = (dict(metallic=0.1, roughness=0.6, color=(0.7, 0.3, 0.2)), dict(metallic=0.8, roughness=0.3, color=(0.2, 0.5, 0.8)))


def _uv_margin(p_err, width):          # mix_cases.lit_uv_margin's reasoning for this scale
    return CHECK_SCALE * (p_err / width + 3 * 2.0 ** -24) + CHECK_SCALE * 2.0 ** -24


@pytest.mark.parametrize("integ", ["path", "all", "whitted"])
def test_lit_quad_with_checkerboard_parameters(gpu_ctx, integ):
    """metallic, roughness and color behind aamode "none" checkerboards of one scale: the lobes are built at every hit, and every pixel
    meets the closed form of the constant material its check selects (checkerboard.rs:50-57: tex1 where floor(s) + floor(t) is even)."""
    a, b = CELLS

    def material(sb):
        kw = dict(uscale=CHECK_SCALE, vscale=CHECK_SCALE, aamode="none")
        sb.material_disney(metallic=sb.texture_checkerboard(a["metallic"], b["metallic"], **kw), roughness=sb.texture_checkerboard(a["roughness"], b["roughness"], **kw),
                           color=sb.texture_checkerboard(a["color"], b["color"], **kw), sheen=0.5, clearcoat=0.3, clearcoatgloss=0.5)
    run = _lit_run(gpu_ctx, integ, CAM_ABOVE, material)
    truths = [D.BSDF(DC.disney(sheen=0.5, clearcoat=0.3, clearcoatgloss=0.5, **c), np.float64) for c in CELLS]

    def select(p):
        st = np.stack([(p[:, 0] - QUAD[0]) / (QUAD[1] - QUAD[0]), (p[:, 1] - QUAD[2]) / (QUAD[3] - QUAD[2])], 1) * CHECK_SCALE
        near_edge = (np.abs(st - np.round(st)) <= _uv_margin(P_ERR, QUAD[1] - QUAD[0])).any(1)
        even = (np.floor(st).sum(1) % 2) == 0
        select.even = even
        return [(truths[0], even), (truths[1], ~even)], near_edge
    n_lit, skip, hit = _closed_form(run, select)
    assert n_lit > 60 and skip.mean() <= C.MAX_LEFT_OUT
    assert (select.even & hit & ~skip).sum() > 20 and (~select.even & hit & ~skip).sum() > 20          # both cells were rendered


def test_constant_textures_render_the_constant_material(gpu_ctx):
    """Every parameter behind checkerboard(c, c): the per-hit route must render what the constant material renders, bit for bit, in every
    kernel family member the room reaches; two different values render something else."""
    p = DC.params("thin_all")

    def textured(two=False):
        def mat(b):
            kw = dict(uscale=4.0, vscale=4.0, aamode="none")
            tex = {k: b.texture_checkerboard(v, (0.9 * v if two else v) if not isinstance(v, tuple) else (tuple(0.5 * x for x in v) if two else v), **kw)
                   for k, v in p.items() if k not in ("type", "thin", "scatterdistance")}
            b.material_disney(thin=True, **tex)
        return mat
    for integ in ("path_sobol", "directlighting_all", "whitted"):
        const = render_everything(gpu_ctx, room_scene(lambda b: DC.apply(b, p), "plain", integ, res=16))
        same = render_everything(gpu_ctx, room_scene(textured(), "plain", integ, res=16))
        assert np.array_equal(bits(const[0]), bits(same[0])) and np.array_equal(bits(const[2]), bits(same[2])) and const[0].sum() > 0, integ
        other = render_everything(gpu_ctx, room_scene(textured(True), "plain", integ, res=16))
        assert not np.array_equal(bits(const[0]), bits(other[0])), integ


def _aov_ns(ctx, mat):
    b = fs.base(res=16, spp=1, depth=5)
    b.integrator_aov(target="ns")
    fs.room(b)
    mat(b)
    P, N, UV, idx = fs.uv_sphere((-0.7, -0.9, 0.0), 0.9, 8, 12)
    b.shape_trianglemesh(P, idx, N=N, uv=UV)
    b.shape_trianglemesh([(0.2, -1.8, -0.8), (1.8, -1.8, -0.8), (1.8, 0.3, 0.9), (0.2, 0.3, 0.9)], [0, 1, 2, 0, 2, 3], uv=[(0, 0), (1, 0), (1, 1), (0, 1)])
    ctx.upload(b.build())
    ctx.film_clear(); ctx.render()
    return ctx.film_xyzw()


def test_bumped_disney_has_the_bumped_mattes_shading_normal(gpu_ctx):
    """material_bump comes first in either material (disney.rs:652-655, matte.rs): aov's ns is bit-equal; without the bump map it is not."""
    bump = lambda b: b.texture_checkerboard(0.0, 0.03, uscale=6.0, vscale=6.0)
    d = _aov_ns(gpu_ctx, lambda b: b.material_disney(color=(0.6, 0.45, 0.3), sheen=0.4, bumpmap=bump(b)))
    m = _aov_ns(gpu_ctx, lambda b: b.material_matte(Kd=(0.6, 0.45, 0.3), bumpmap=bump(b)))
    flat = _aov_ns(gpu_ctx, lambda b: b.material_disney(color=(0.6, 0.45, 0.3), sheen=0.4))
    assert np.array_equal(bits(d), bits(m)) and d.max() > 0
    assert not np.array_equal(bits(d), bits(flat))


# ---------------------------------------------------------------- 6. the BSDF-sampling leg under MIS
@pytest.mark.parametrize("name", ["sheen", "clearcoat"])
def test_path_mis_carries_the_reported_pdfs(gpu_ctx, name):
    """A Disney quad under a constant environment of radiance 1, `path` at maxdepth 1: every camera sample is one estimate_direct, whose
    light half weighs by the REPORTED pdf (DisneyDiffuse's 0 inside the average, Q84; the clearcoat's sum, Q85) and whose BSDF half draws
    from the lobes' true densities, a quarter of the picks returning None.  Mean and variance come from disney_ref by quadrature in
    float64 (disney_cases.mis_moments, held to the restatement's own sampler in test_disney_host.py); the frame's mean must lie within
    five standard errors.  The size is test_path_mis_carries_the_pdf_without_inv_pi's."""
    n = 64 * 64 * 16
    mean, var = DC.mis_moments(name)
    bound = 5.0 * np.sqrt(var / n)              # five standard errors: a condition on the false-alarm rate (the Sobol' points do better)
    repaired, _ = DC.mis_moments(name, True)
    assert (np.abs(repaired - mean) > bound).all(), "the test could not tell the quirk"
    b = scenes.SceneBuilder()
    b.look_at((0, 0, 1), (0, 0, 0), (0, 1, 0))
    b.camera_perspective(fov=DC.MIS_FOV)
    b.film(xresolution=64, yresolution=64)
    b.pixel_filter_box()
    b.sampler_sobol(16)
    b.integrator_path(maxdepth=1)
    DC.apply(b, DC.params(name))
    b.shape_trianglemesh([-1000, -1000, 0, 1000, -1000, 0, 1000, 1000, 0, -1000, 1000, 0], [0, 1, 2, 0, 2, 3])
    b.light_infinite(L=(1.0, 1.0, 1.0))
    gpu_ctx.upload(b.build())
    g = gpu_ctx.radiance_samples((0, 0, 64, 64)).reshape(-1, 3).astype(np.float64)       # the film's own pixels
    assert len(g) == n
    got = g.mean(0)
    print("\npath under MIS, %s: mean %s, quadrature %s (DisneyDiffuse's pdf repaired %s), bound %s" % (name, got, mean, repaired, bound))
    assert (np.abs(got - mean) <= bound).all(), (got, mean, bound)


# ---------------------------------------------------------------- 7. the kernel families
def _family_pair(name, cylinder):
    p = DC.params(name)

    def shapes_first(b):
        if cylinder:
            b.material_matte((0.6, 0.6, 0.7))
            t = scenes.transform_translate(0.6, 1.0, 0.2)
            b.shape_cylinder(radius=0.4, zmin=-0.5, zmax=0.6, object_to_world=t[0], world_to_object=t[1])

    def alone(b):
        shapes_first(b)
        DC.apply(b, p)

    def mixed(b):
        shapes_first(b)
        with_black_mix(b, p)
    return mixed, alone


@pytest.mark.parametrize("variant", ["plain", "env", "inst", "sphere", "cylinder"])
@pytest.mark.parametrize("name", ["thin_all", "clearcoat"])
def test_render_equals_the_material_under_a_mix(gpu_ctx, name, variant):
    """D alone and mix(D, matte(Kd 0), 1) render bit-equal in every integrator: k_shade_mix, k_shade_mix_inst, k_rec_enter_mix /
    k_rec_next_mix and k_aov_mix of the Disney build, with spheres, a cylinder, instances and an environment light beside them.  The
    render differs from the same room with a matte in D's place, and the counters are finite and non-zero."""
    room = "plain" if variant == "cylinder" else variant
    pair = _family_pair(name, variant == "cylinder")
    assert_same_render(gpu_ctx, pair, room, res=16, tag="%s %s" % (name, variant))
    for integ in ("path_sobol", "whitted"):
        g, cnt, film = render_everything(gpu_ctx, room_scene(pair[1], room, integ, res=16))
        gm = render_everything(gpu_ctx, room_scene(lambda b: b.material_matte(DC.params(name)["color"]), room, integ, res=16))[0]
        assert not np.array_equal(bits(g), bits(gm)), (name, variant, integ)
        assert np.isfinite(g).all() and np.isfinite(film).all() and g.sum() > 0
        assert cnt["camera_rays"] > 0 and cnt["shadow_rays"] > 0 and cnt["nodes_visited"] > 0
        if integ == "path_sobol":
            for k in RAY_COUNTERS:
                assert cnt[k] > 0, (k, cnt[k])


def test_aov_of_a_disney_scene(gpu_ctx):
    a = _aov_ns(gpu_ctx, lambda b: DC.apply(b, DC.params("sheen")))
    m = _aov_ns(gpu_ctx, lambda b: with_black_mix(b, DC.params("sheen")))
    assert np.array_equal(bits(a), bits(m)) and a.max() > 0


# ---------------------------------------------------------------- 8. command line
def test_cli_renders_a_disney_scene(tmp_path):
    """`pbrt_gpu -i` on a ten-line scene with Material "disney" writes the image the SceneBuilder scene renders."""
    text = """LookAt 0 -4 3  0 0 0  0 0 1
Camera "perspective" "float fov" [50]
Film "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" "o.pfm"
PixelFilter "box"
Sampler "sobol" "integer pixelsamples" [4]
Integrator "path" "integer maxdepth" [3]
WorldBegin
LightSource "distant" "rgb L" [3 3 3] "point from" [0.2 3 2.5] "point to" [0 0 0]
Material "disney" "rgb color" [0.6 0.45 0.3] "float sheen" [0.5] "float clearcoat" [0.7] "float clearcoatgloss" [0.8] "float metallic" [0.2]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -2 0 2 -2 0 2 2 0 -2 2 0] "float uv" [0 0 1 0 1 1 0 1]
WorldEnd
"""
    (tmp_path / "s.pbrt").write_text(text)

    def render(scene):
        ctx = pkg.Context(0)
        try:
            ctx.upload(scene)
            ctx.film_clear(); ctx.render()
            return ctx.film_rgb()
        finally:
            ctx.close()
    sb = scenes.SceneBuilder()
    sb.look_at((0, -4, 3), (0, 0, 0), (0, 0, 1))
    sb.camera_perspective(fov=50.0)
    sb.film(xresolution=16, yresolution=16)
    sb.pixel_filter_box()
    sb.sampler_sobol(pixelsamples=4)
    sb.integrator_path(maxdepth=3)
    sb.light_distant(L=(3, 3, 3), frm=(0.2, 3, 2.5), to=(0, 0, 0))
    sb.material_disney(color=(0.6, 0.45, 0.3), sheen=0.5, clearcoat=0.7, clearcoatgloss=0.8, metallic=0.2)
    sb.shape_trianglemesh([-2, -2, 0, 2, -2, 0, 2, 2, 0, -2, 2, 0], [0, 1, 2, 0, 2, 3], uv=UV_X)
    want = render(sb.build())
    parsed = render(capi.ParsedScene(filename=str(tmp_path / "s.pbrt"), disney_materials=True, delta_lights=True))
    assert np.array_equal(bits(parsed), bits(want)) and want.max() > 0
    exe = os.path.join(ROOT, "pbrt-r3_amd", "csrc", "pbrt_gpu")
    out = tmp_path / "cli.pfm"
    r = subprocess.run([exe, "-i", str(tmp_path / "s.pbrt"), "--outfile", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer(out.read_bytes().split(b"\n", 3)[3], "<f4").reshape(16, 16, 3)[::-1]
    assert np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------- refusals and the hooks' limits
def _tiny(fill):
    b = fs.base(res=8, spp=1)
    fs.room(b)
    fill(b)
    b.shape_trianglemesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [0, 1, 2])
    return b


def _refused(ctx, sd, status):
    with pytest.raises(capi.PtError) as e:
        ctx.upload(sd)
    assert e.value.status == status, str(e.value)
    return str(e.value)


def test_upload_refuses_bad_records(gpu_ctx):
    b = _tiny(lambda b: b.material_disney())
    sd = b.build()
    sd.disney[0].material = 1000
    assert "index" in _refused(gpu_ctx, sd, 1)
    sd = b.build()
    sd.disney[0].material = 0                                   # the room's matte
    assert "not a Disney" in _refused(gpu_ctx, sd, 1)
    sd = b.build()
    sd.disney[0].tex[capi.PT_DISNEY_SHEEN] = 1000
    _refused(gpu_ctx, sd, 1)
    b = _tiny(lambda b: b.material_disney(metallic=b.texture_checkerboard((0.9, 0.1, 0.1), (0.1, 0.9, 0.2), uscale=4.0, vscale=4.0)))
    assert "colour texture" in _refused(gpu_ctx, b.build(), 1)
    b = _tiny(lambda b: b.material_disney(scatterdistance=(0.1, 0.0, 0.0)))
    msg = _refused(gpu_ctx, b.build(), 4)
    assert "scatterdistance" in msg and "thin" in msg
    b = _tiny(lambda b: b.material_disney(scatterdistance=(0.1, 0.0, 0.0), thin=True))
    gpu_ctx.upload(b.build())                                    # thin: never evaluated, accepted and ignored
    sd = _tiny(lambda b: b.material_disney()).build()
    sd.disney = []                                               # no record: the reference's defaults
    gpu_ctx.upload(sd)
    wo, wi, u = hook_inputs(np.random.default_rng(64))
    mat = sd.desc.n_materials - 1
    got = gpu_ctx.bsdf_eval(mat, wo, wi)
    gpu_ctx.upload(_tiny(lambda b: b.material_disney()).build())
    want = gpu_ctx.bsdf_eval(mat, wo, wi)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])) and (got[0] != 0).any()


def test_hooks_refuse_a_per_hit_material(gpu_ctx):
    b = _tiny(lambda b: b.material_disney(roughness=b.texture_checkerboard(0.2, 0.6, uscale=4.0, vscale=4.0, aamode="none")))
    gpu_ctx.upload(b.build())
    wo, wi, u = hook_inputs(np.random.default_rng(65))
    for call in (lambda: gpu_ctx.bsdf_eval(b.cur_material, wo, wi), lambda: gpu_ctx.bsdf_sample(b.cur_material, wo, u)):
        with pytest.raises(capi.PtError) as e:
            call()
        assert e.value.status == 4 and "Disney" in str(e.value)


def test_a_mix_counts_a_per_hit_disney_leaf_at_eight(gpu_ctx):
    """Two per-hit Disney leaves fill the 16 lobes of a mix tree; a third leaf of one lobe is refused with the counts."""
    tex = lambda b: b.texture_checkerboard(0.2, 0.6, uscale=4.0, vscale=4.0, aamode="none")

    def two(b):
        b.material_disney(roughness=tex(b)); i = b.cur_material
        b.material_disney(sheen=tex(b)); j = b.cur_material
        b.material_mix(i, j, 0.4)
    g = render_everything(gpu_ctx, _tiny(two).build())[0]
    assert np.isfinite(g).all() and g.sum() > 0

    def three(b):
        two(b); k = b.cur_material
        b.material_matte((0.5, 0.5, 0.5))
        b.material_mix(k, b.cur_material, 0.5)
    msg = _refused(gpu_ctx, _tiny(three).build(), 4)
    assert "3 leaves" in msg and "17 lobes" in msg, msg
