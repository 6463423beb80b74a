"""Material "mix" on the device (materials/mix.rs:53-96, core/reflection/scaled.rs).

The hooks are held to the float64 truth tests/mix_ref.py with bsdf_cases' checks, and bit for bit to the device's own evaluations of the
children.  The rendering kernels of a scene with a mix (k_shade_mix, k_shade_mix_inst, k_rec_enter_mix / k_rec_next_mix, k_aov_mix) are
held bit for bit to the kernels the oracle pins: mix(A, matte(Kd 0), amount 1) scales A's lobes by exactly 1 and adds nothing, so the
scene renders what the scene with A alone renders -- through another kernel family."""
import numpy as np
import pytest

import bsdf_cases as C
import bsdf_ref as R
import delta_light_ref as dref
import feature_scenes as fs
import mix_cases as MC
import mix_ref as M
from aov_ref import E
from helpers import bits, pkg, scenes
from test_gpu_bsdf_truth import LIGHT, QUAD, UV_X, CAM_ABOVE, quad_frame
from test_gpu_delta_light import EPS, P_ERR, Run, add_distant, base, check_closed_form, delta_terms, plane_hit
from test_gpu_translucent import INTEGRATORS, assert_same_render, hook_inputs, mis_moments, render_everything, room_scene, whitted_scene

pytestmark = pytest.mark.gpu
capi = pkg.capi
f32 = np.float32
Z3, O3 = (0.0,) * 3, (1.0,) * 3
FLAGS = [fl for _, fl in C.FLAG_SETS]


@pytest.fixture(autouse=True)
def counters_left_clean(gpu_ctx):
    yield
    gpu_ctx.reset_counters()


# ---------------------------------------------------------------- 1. hooks against the truth
@pytest.mark.parametrize("name", list(MC.SETTINGS))
def test_hooks_meet_the_truth(gpu_ctx, name):
    sd = MC.palette(MC.SETTINGS)
    gpu_ctx.upload(sd)
    mat = sd.material_index[name]
    stats = MC.run_setting(name, lambda wo, wi, fl: gpu_ctx.bsdf_eval(mat, wo, wi, fl), lambda wo, u, fl: gpu_ctx.bsdf_sample(mat, wo, u, fl), "gpu")
    MC.hold_caps_and_medians(stats, name, "gpu")


# ---------------------------------------------------------------- 2. hooks, bit for bit, device against device
EIGHT = {"matte": ("matte", "oren_25"), "plastic": ("plastic", "remap"), "mirror": ("mirror", "mirror"), "glass": ("glass", "smooth"),
         "metal": ("metal", "aniso_uv"), "uber": ("uber", "five"), "substrate": ("substrate", "aniso"), "translucent": ("translucent", "four")}


def test_hooks_compose_the_childrens_own_evaluations(gpu_ctx):
    """Single-lobe reflection children A and B: f_mix = fl32(fl32(s1 f_A) + fl32(s2 f_B)), pdf_mix = fl32(fl32(p_A + p_B) / 2), formed in
    numpy float32 from the device's evaluations of A and B."""
    a, b = C.params("matte", "oren_25"), C.params("metal", "iso")
    amount = (0.3, 0.65, 0.9)
    sd = MC.palette({"a": a, "b": b, "mix": MC.mix(a, b, amount)})
    gpu_ctx.upload(sd)
    ix = sd.material_index
    wo, wi, u = hook_inputs(np.random.default_rng(51))
    s1 = np.array(amount, f32)
    s2 = (f32(1) - s1).astype(f32)
    for fl in FLAGS:
        (fa, pa), (fb, pb), (fm, pm) = [gpu_ctx.bsdf_eval(ix[k], wo, wi, fl) for k in ("a", "b", "mix")]
        want_f = ((s1 * fa).astype(f32) + (s2 * fb).astype(f32)).astype(f32)
        want_p = ((pa + pb).astype(f32) / f32(2)).astype(f32)
        assert np.array_equal(bits(fm), bits(want_f)), fl
        assert np.array_equal(bits(pm), bits(want_p)), fl
        assert (fm != 0).any()


def test_hooks_sampling_picks_a_child_by_half_of_u(gpu_ctx):
    """u.x on a 2^-12 grid: (u.x / 2, u.y) is child A's sample at (u.x, u.y), (u.x / 2 + 1 / 2, u.y) child B's -- wi and type are the inner lobe's."""
    a, b = C.params("matte", "lambert"), C.params("metal", "iso")
    sd = MC.palette({"a": a, "b": b, "mix": MC.mix(a, b, (0.3, 0.65, 0.9))})
    gpu_ctx.upload(sd)
    ix = sd.material_index
    rng = np.random.default_rng(52)
    wo, _, u = hook_inputs(rng)
    u[:, 0] = (rng.integers(0, 4096, len(u)) / 4096.0).astype(f32)
    for child, off in (("a", 0.0), ("b", 0.5)):
        um = u.copy()
        um[:, 0] = (u[:, 0] / f32(2) + f32(off)).astype(f32)
        _, wi_c, _, t_c = gpu_ctx.bsdf_sample(ix[child], wo, u, R.ALL)
        _, wi_m, _, t_m = gpu_ctx.bsdf_sample(ix["mix"], wo, um, R.ALL)
        assert np.array_equal(t_c, t_m), child
        assert np.array_equal(bits(wi_c), bits(wi_m)), child
        assert (t_m != 0).sum() > len(u) // 2


def test_hooks_lobeless_sibling_leaves_the_child(gpu_ctx):
    """mix(A, matte(Kd 0), amount 1) is A: f, pdf and every output of sample_f, for the eight materials and the three flag sets."""
    trees = {}
    for k, cs in EIGHT.items():
        trees[k] = C.params(*cs)
        trees[k + "/mix"] = MC.mix(C.params(*cs), MC.BLACK, 1.0)
    sd = MC.palette(trees)
    gpu_ctx.upload(sd)
    ix = sd.material_index
    wo, wi, u = hook_inputs(np.random.default_rng(53))
    for k in EIGHT:
        for fl in FLAGS:
            ea, em = gpu_ctx.bsdf_eval(ix[k], wo, wi, fl), gpu_ctx.bsdf_eval(ix[k + "/mix"], wo, wi, fl)
            assert np.array_equal(bits(ea[0]), bits(em[0])) and np.array_equal(bits(ea[1]), bits(em[1])), (k, fl)
            sa, sm = gpu_ctx.bsdf_sample(ix[k], wo, u, fl), gpu_ctx.bsdf_sample(ix[k + "/mix"], wo, u, fl)
            assert np.array_equal(sa[3], sm[3]), (k, fl, "type")
            for j in range(3):
                assert np.array_equal(bits(sa[j]), bits(sm[j])), (k, fl, j)


# ---------------------------------------------------------------- 3. renders, bit for bit against oracle-pinned kernels
def mixed(mat, first=True):
    """mat alone, and mix(mat, matte(Kd 0), 1) (first) or mix(matte(Kd 0), mat, 0): the same BSDF through the mix kernels."""
    def m(b):
        mat(b)
        a = b.cur_material
        b.material_matte(Kd=Z3)
        k = b.cur_material
        if first:
            b.material_mix(a, k, O3)
        else:
            b.material_mix(k, a, Z3)
    return m, mat


def textured_plastic(b):
    b.material_plastic(Kd=b.texture_checkerboard((0.8, 0.3, 0.2), (0.1, 0.3, 0.7), uscale=5.0, vscale=5.0), Ks=(0.4, 0.4, 0.4),
                       roughness=b.texture_checkerboard(0.05, 0.4, uscale=3.0, vscale=3.0, aamode="none"))


RENDERED = {
    "matte": lambda b: b.material_matte(Kd=(0.5, 0.3, 0.2), sigma=20.0),
    "plastic": lambda b: b.material_plastic(Kd=(0.5, 0.3, 0.2), Ks=(0.3, 0.4, 0.5), roughness=0.15),
    "glass_rough": lambda b: b.material_glass(Kr=(0.8, 0.7, 0.6), Kt=(0.6, 0.9, 0.8), eta=1.5, uroughness=0.2, vroughness=0.1),
    "glass_smooth": lambda b: b.material_glass(Kr=(0.9, 0.8, 0.7), Kt=(0.6, 0.7, 0.8), eta=1.5),
    "uber": lambda b: b.material_uber(Kd=(0.3, 0.2, 0.5), Ks=(0.2, 0.3, 0.1), Kr=(0.1, 0.15, 0.2), Kt=(0.25, 0.2, 0.15), opacity=(0.6, 0.9, 0.8), eta=1.4, roughness=0.3),
    "translucent": lambda b: b.material_translucent(Kd=(0.3, 0.25, 0.2), Ks=(0.2, 0.3, 0.25), reflect=(0.5, 0.6, 0.4), transmit=(0.4, 0.3, 0.6), roughness=0.15),
    "textured": textured_plastic,                       # the per-hit route: the tree's lobes are built at every hit
}


@pytest.mark.parametrize("variant", ["plain", "env", "inst", "sphere"])
@pytest.mark.parametrize("name", list(RENDERED))
def test_render_equals_the_child_alone(gpu_ctx, name, variant):
    assert_same_render(gpu_ctx, mixed(RENDERED[name]), variant, tag=name)


@pytest.mark.parametrize("k", range(6))
def test_render_equals_the_child_alone_drawn(gpu_ctx, k):
    """Drawn children, either side of the mix, 16 x 16."""
    rng = np.random.default_rng(200 + k)
    c = lambda: tuple(float(x) for x in rng.uniform(0.1, 0.9, 3))
    kd, ks, kr, kt, ro = c(), c(), c(), c(), float(rng.uniform(0.02, 1.0))
    mat = [lambda b: b.material_plastic(Kd=kd, Ks=ks, roughness=ro), lambda b: b.material_glass(Kr=kr, Kt=kt, eta=1.3, uroughness=ro, vroughness=ro),
           lambda b: b.material_uber(Kd=kd, Ks=ks, Kr=kr, opacity=kt, roughness=ro)][k % 3]
    assert_same_render(gpu_ctx, mixed(mat, first=k % 2 == 0), "plain", res=16, tag="drawn %d" % k)


# ---------------------------------------------------------------- 4. frame and eta (mix.rs:83)
def bump(b):
    return b.texture_checkerboard(0.0, 0.03, uscale=6.0, vscale=6.0)


def _pairs_frame():
    A = lambda b, t=None: b.material_plastic(Kd=(0.5, 0.3, 0.2), Ks=(0.3, 0.4, 0.5), roughness=0.2, bumpmap=t)

    def first(b):          # mix(A with bump T, black, 1) == A with bump T
        A(b, bump(b)); a = b.cur_material
        b.material_matte(Kd=Z3); k = b.cur_material
        b.material_mix(a, k, O3)

    def black_first(b):    # mix(black matte with bump T, A, 0) == A with bump T: the frame is child 1's (A's bsdf_eta is 1)
        b.material_matte(Kd=Z3, bumpmap=bump(b)); k = b.cur_material
        A(b); a = b.cur_material
        b.material_mix(k, a, Z3)

    def bump_second(b):    # mix(A, black matte with bump T, 1) == A without a bump: child 2's bump map never reaches the BSDF
        A(b); a = b.cur_material
        b.material_matte(Kd=Z3, bumpmap=bump(b)); k = b.cur_material
        b.material_mix(a, k, O3)
    return {"first": (first, lambda b: A(b, bump(b))), "black_first": (black_first, lambda b: A(b, bump(b))), "bump_second": (bump_second, lambda b: A(b))}


@pytest.mark.parametrize("which", ["first", "black_first", "bump_second"])
def test_frame_is_child_ones(gpu_ctx, which):
    """The three identities of Q75, bit for bit, in `path` and in aov's ns / shading dpdu: mix(A with bump T, black, 1) is A with bump T;
    mix(black matte with bump T, A, 0) is A with bump T (the frame is child 1's); mix(A, black matte with bump T, 1) is A without a bump."""
    pair = _pairs_frame()[which]
    assert_same_render(gpu_ctx, pair, "plain", integrators=["path_sobol"], tag=which)
    for target in ("ns", "dpdus"):
        films = []
        for mat in pair:
            films.append(_aov_film(gpu_ctx, mat, target))
        assert np.array_equal(bits(films[0]), bits(films[1])), (which, target)
        assert films[0].max() > 0


def _aov_film(ctx, mat, target):
    b = fs.base(res=32, spp=4, depth=5)
    b.integrator_aov(target=target)
    fs.room(b)
    mat(b)
    P, N, UV, idx = fs.uv_sphere((-0.7, -0.9, 0.0), 0.9, 8, 12)
    b.shape_trianglemesh(P, idx, N=N, uv=UV)
    b.shape_trianglemesh([(0.2, -1.8, -0.8), (1.8, -1.8, -0.8), (1.8, 0.3, 0.9), (0.2, 0.3, 0.9)], [0, 1, 2, 0, 2, 3], uv=[(0, 0), (1, 0), (1, 1), (0, 1)])
    ctx.upload(b.build())
    ctx.film_clear(); ctx.render()
    return ctx.film_xyzw()


def test_aov_sees_the_bump(gpu_ctx):
    """(the frame tests can tell: the bump map changes ns)"""
    A = lambda b, t=None: b.material_plastic(Kd=(0.5, 0.3, 0.2), roughness=0.2, bumpmap=t)
    assert not np.array_equal(_aov_film(gpu_ctx, lambda b: A(b, bump(b)), "ns"), _aov_film(gpu_ctx, lambda b: A(b), "ns"))


def _eta_scene(glass_first, maxdepth):
    def mat(b):
        if glass_first:
            b.material_glass(Kr=(0.9,) * 3, Kt=(0.95,) * 3, eta=1.5); g = b.cur_material
            b.material_matte(Kd=Z3); k = b.cur_material
            b.material_mix(g, k, O3)
        else:
            b.material_matte(Kd=Z3); k = b.cur_material
            b.material_glass(Kr=(0.9,) * 3, Kt=(0.95,) * 3, eta=1.5); g = b.cur_material
            b.material_mix(k, g, Z3)
    b = fs.base(res=32, spp=4, depth=maxdepth)
    fs.room(b)
    mat(b)
    for c, r in (((-0.7, -0.9, 0.0), 0.9), ((0.9, -0.6, 0.3), 0.7), ((0.1, 0.8, -0.6), 0.6)):          # enough glass that paths pass several interfaces
        P, N, UV, idx = fs.uv_sphere(c, r, 8, 12)
        b.shape_trianglemesh(P, idx, N=N, uv=UV)
    return b.build()


def test_eta_is_child_ones(gpu_ctx):
    """BSDF::eta is child 1's: 1 for mix(black matte, glass, 0), 1.5 for mix(glass, black matte, 1).  Only path's eta_scale reads it, and
    only the Russian roulette reads that: `bounces > 3` (path.rs:218-229), so up to maxdepth 4 the two scenes render alike."""
    lo = [render_everything(gpu_ctx, _eta_scene(gf, 4))[0] for gf in (True, False)]
    assert np.array_equal(bits(lo[0]), bits(lo[1])) and lo[0].sum() > 0
    hi = [render_everything(gpu_ctx, _eta_scene(gf, 8)) for gf in (True, False)]
    # The two renders can differ only where a roulette read another eta_scale, which takes a path past bounce 3 that crossed glass: their
    # inequality is the evidence that one survived that long.  (More vertices than at maxdepth 4 shows the longer paths exist at all.)
    lo_vertices = render_everything(gpu_ctx, _eta_scene(True, 4))[1]["path_vertices"]
    assert hi[0][1]["path_vertices"] > lo_vertices
    assert not np.array_equal(bits(hi[0][0]), bits(hi[1][0]))


# ---------------------------------------------------------------- 5. whitted's direct term, path under MIS
def test_whitted_direct_term_is_the_weighted_sum(gpu_ctx):
    """mix(matte a, matte b, s) against matte(s a + (1 - s) b).  rtol 1e-4 by test_whitted_sees_the_light_through_the_square's reasoning:
    cosines >= 0.3, the light at least 1 unit away, float32 rounding near 1e-7 per operation; a swapped weight is an error of order 1."""
    a, bb, s = (0.8, 0.2, 0.4), (0.1, 0.7, 0.3), 0.25
    both = tuple(s * x + (1 - s) * y for x, y in zip(a, bb))
    swapped = tuple((1 - s) * x + s * y for x, y in zip(a, bb))

    def mx(b):
        b.material_matte(a); i = b.cur_material
        b.material_matte(bb); j = b.cur_material
        b.material_mix(i, j, (s,) * 3)
    got = render_everything(gpu_ctx, whitted_scene(mx, 2.0))[0].astype(np.float64)
    want = render_everything(gpu_ctx, whitted_scene(lambda b: b.material_matte(both), 2.0))[0].astype(np.float64)
    wrong = render_everything(gpu_ctx, whitted_scene(lambda b: b.material_matte(swapped), 2.0))[0].astype(np.float64)
    assert (want > 0).all()
    rel = np.abs(got - want) / want
    print("\nwhitted, mix of two mattes against the matte of the weighted colour: max relative difference %.3e" % rel.max())
    assert rel.max() <= 1e-4
    assert (np.abs(got - wrong) / wrong).min() > 1e-4, "the test could not tell s from 1 - s"


def test_path_mis_of_a_lambertian_mix(gpu_ctx):
    """A reflecting mix of two Lambertian lobes under a constant environment: f = (s a + (1 - s) b) / pi, pdf = cos / pi (the average of two
    equal pdfs), so one estimate_direct has the moments of test_gpu_translucent's quadrature with that colour and the pdf cos / pi."""
    a, bb, s = (0.9, 0.2, 0.5), (0.1, 0.8, 0.3), 0.3
    col = lambda w: tuple(w * x + (1 - w) * y for x, y in zip(a, bb))
    n = 64 * 64 * 16
    mean, var = mis_moments(col(s), v3_pdf=True)
    bound = 5.0 * np.sqrt(var / n)              # five standard errors: a condition on the false-alarm rate
    mean_sw, _ = mis_moments(col(1 - s), v3_pdf=True)
    assert (np.abs(mean_sw - mean) > bound).all(), "the test could not tell s from 1 - s"
    b = scenes.SceneBuilder()
    b.look_at((0, 0, 1), (0, 0, 0), (0, 1, 0))
    b.camera_perspective(fov=20.0)
    b.film(xresolution=64, yresolution=64)
    b.pixel_filter_box()
    b.sampler_sobol(16)
    b.integrator_path(maxdepth=3)
    b.material_matte(a); i = b.cur_material
    b.material_matte(bb); j = b.cur_material
    b.material_mix(i, j, (s,) * 3)
    b.shape_trianglemesh([-1000, -1000, 0, 1000, -1000, 0, 1000, 1000, 0, -1000, 1000, 0], [0, 1, 2, 0, 2, 3])
    b.light_infinite(L=(1.0, 1.0, 1.0))
    gpu_ctx.upload(b.build())
    g = gpu_ctx.radiance_samples((0, 0, 64, 64)).reshape(-1, 3).astype(np.float64)
    assert len(g) == n
    got = g.mean(0)
    print("\npath under MIS: mean %s, quadrature %s (weights swapped %s), bound %s" % (got, mean, mean_sw, bound))
    assert (np.abs(got - mean) <= bound).all(), (got, mean, bound)


# ---------------------------------------------------------------- 6. the lit quad: rendered radiance against the truth's f
LIT_TREE = MC.mix(dict(type="plastic", Kd=(0.3, 0.2, 0.1), Ks=(0.4, 0.5, 0.6), roughness=0.3), dict(type="matte", Kd=(0.2, 0.5, 0.7), sigma=15.0), (0.3, 0.6, 0.8))


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("integ", ["path", "all"])
def test_lit_quad_renders_the_truths_f(gpu_ctx, integ, sampler):
    """Per camera sample the radiance is f(wo, wi) L |cos| with mix_ref's f on the quad's frame, within its bound (a constant mix)."""
    sb = base("path" if integ == "path" else "all", sampler, maxdepth=1 if integ == "path" else 5)
    sb.look_at(CAM_ABOVE, (0, 0, 0), (0, 0, 1))
    MC.apply(sb, LIT_TREE)
    sb.shape_trianglemesh([QUAD[0], QUAD[2], 0.0, QUAD[1], QUAD[2], 0.0, QUAD[1], QUAD[3], 0.0, QUAD[0], QUAD[3], 0.0], [0, 1, 2, 0, 2, 3], uv=UV_X)
    add_distant(sb, **LIGHT)
    run = Run(gpu_ctx, sb.build())
    p, hit, edge = plane_hit(run.o, run.d, 0.0, QUAD, P_ERR)
    ss, ts, ns = quad_frame(UV_X)
    bsdf = M.BSDF(LIT_TREE, np.float64)
    d = run.d / np.linalg.norm(run.d, axis=1, keepdims=True)
    wo = [E(-(d @ a), 6 * EPS) for a in (ss, ts, ns)]
    state = {}

    def brdf(wi_w):
        wi = [E(wi_w @ a, state["wi_err"] + 4 * EPS) for a in (ss, ts, ns)]
        state["v"] = bsdf.eval(wo, wi, R.NOSPEC)
        return state["v"].f
    state["wi_err"] = dref.sample_li(run.lights[0], p, P_ERR)["wi_err"]
    (c, rel, near, lit), = delta_terms(run, p, brdf=brdf)
    v = state["v"]
    with np.errstate(all="ignore"):
        f_rel = np.where(v.f > 0, v.f_e / v.f, 0.0).max(1)
    want = np.where(hit[:, None], c, 0.0)
    skip = edge | (hit & (near | v.left_out()))
    n_lit, n_zero = check_closed_form(run, want, rel + f_rel + 2 * EPS, skip)
    assert n_lit > 300, n_lit
    assert skip.mean() <= C.MAX_LEFT_OUT


def test_lit_quad_with_a_checkerboard_amount(gpu_ctx):
    """amount = checkerboard(c0, c1), aamode "none": the cell of the sample's uv decides its amount (checkerboard.rs:50-57: tex1 where
    floor(s) + floor(t) is even).  The truth is mix_ref at c0 or at c1 by cell; samples within the uv bound of a cell edge are left out."""
    c0, c1 = MC.LIT_AMOUNTS
    sb = base("path", "sobol", maxdepth=1)
    sb.look_at(CAM_ABOVE, (0, 0, 0), (0, 0, 1))
    p_, m_ = MC.apply(sb, LIT_TREE["m1"]), MC.apply(sb, LIT_TREE["m2"])
    sb.material_mix(p_, m_, sb.texture_checkerboard(c0, c1, uscale=MC.LIT_SCALE, vscale=MC.LIT_SCALE, aamode="none"))
    sb.shape_trianglemesh([QUAD[0], QUAD[2], 0.0, QUAD[1], QUAD[2], 0.0, QUAD[1], QUAD[3], 0.0, QUAD[0], QUAD[3], 0.0], [0, 1, 2, 0, 2, 3], uv=UV_X)
    add_distant(sb, **LIGHT)
    run = Run(gpu_ctx, sb.build())
    p, hit, edge = plane_hit(run.o, run.d, 0.0, QUAD, P_ERR)
    st_ = np.stack([(p[:, 0] - QUAD[0]) / (QUAD[1] - QUAD[0]), (p[:, 1] - QUAD[2]) / (QUAD[3] - QUAD[2])], 1) * MC.LIT_SCALE
    near_edge = (np.abs(st_ - np.round(st_)) <= MC.lit_uv_margin(P_ERR, QUAD[1] - QUAD[0])).any(1)
    even = (np.floor(st_).sum(1) % 2) == 0
    ss, ts, ns = quad_frame(UV_X)
    bs = [M.BSDF(MC.mix(LIT_TREE["m1"], LIT_TREE["m2"], c), np.float64) for c in (c0, c1)]
    d = run.d / np.linalg.norm(run.d, axis=1, keepdims=True)
    wo = [E(-(d @ a), 6 * EPS) for a in (ss, ts, ns)]
    state = {}

    def brdf(wi_w):
        wi = [E(wi_w @ a, state["wi_err"] + 4 * EPS) for a in (ss, ts, ns)]
        v = [b.eval(wo, wi, R.NOSPEC) for b in bs]
        state["f_e"] = np.where(even[:, None], v[0].f_e, v[1].f_e)
        state["out"] = np.where(even, v[0].left_out(), v[1].left_out())
        state["f"] = np.where(even[:, None], v[0].f, v[1].f)
        return state["f"]
    state["wi_err"] = dref.sample_li(run.lights[0], p, P_ERR)["wi_err"]
    (c, rel, near, lit), = delta_terms(run, p, brdf=brdf)
    with np.errstate(all="ignore"):
        f_rel = np.where(state["f"] > 0, state["f_e"] / state["f"], 0.0).max(1)
    want = np.where(hit[:, None], c, 0.0)
    skip = edge | (hit & (near | state["out"] | near_edge))
    n_lit, n_zero = check_closed_form(run, want, rel + f_rel + 2 * EPS, skip)
    assert n_lit > 300 and skip.mean() <= C.MAX_LEFT_OUT
    assert (even & hit & ~skip).sum() > 100 and (~even & hit & ~skip).sum() > 100          # both amounts were rendered


def test_cli_renders_a_nested_textured_mix(tmp_path):
    """`pbrt_gpu -i` against the library's render of the same text parsed with mix_materials=True: bit-equal PFM; "amount" matters."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = """LookAt 0 -3 2.5  0 0 0.4  0 0 1
Camera "perspective" "float fov" [50]
Film "image" "integer xresolution" [32] "integer yresolution" [32] "string filename" "o.pfm"
Sampler "sobol" "integer pixelsamples" [4]
Integrator "path" "integer maxdepth" [4]
WorldBegin
AttributeBegin
AreaLightSource "diffuse" "rgb L" [12 12 10]
Shape "trianglemesh" "integer indices" [0 2 1 0 3 2] "point P" [-0.5 -0.5 3 0.5 -0.5 3 0.5 0.5 3 -0.5 0.5 3]
AttributeEnd
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 -3 0 3 -3 0 3 3 0 -3 3 0]
Texture "mask" "spectrum" "checkerboard" "rgb tex1" [0.9 0.8 0.7] "rgb tex2" [0.1 0.2 0.3] "float uscale" [6] "float vscale" [6] "string aamode" "none"
MakeNamedMaterial "paint" "string type" "plastic" "rgb Kd" [0.7 0.1 0.1] "rgb Ks" [0.3 0.3 0.3] "float roughness" [0.1]
MakeNamedMaterial "rust" "string type" "matte" "rgb Kd" [0.4 0.2 0.1] "float sigma" [20]
MakeNamedMaterial "metal" "string type" "mirror"
MakeNamedMaterial "rusty" "string type" "mix" "string namedmaterial1" "paint" "string namedmaterial2" "rust" "texture amount" "mask"
MakeNamedMaterial "car" "string type" "mix" "string namedmaterial1" "rusty" "string namedmaterial2" "metal"
NamedMaterial "car"
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 1 1 -1 1 1 1 1.4 -1 1 1.4] "float uv" [0 0 1 0 1 1 0 1] "rgb amount" [0.6 0.7 0.8]
WorldEnd
"""
    (tmp_path / "s.pbrt").write_text(text)
    ps = capi.ParsedScene(filename=str(tmp_path / "s.pbrt"), mix_materials=True)
    types = [ps.desc.materials[i].type for i in range(ps.desc.n_materials)]
    assert types.count(capi.PT_MATERIAL_MIX) == 2
    top = ps.desc.materials[ps.desc.meshes[ps.desc.n_meshes - 1].material]
    assert [f32(v) for v in top.kd] == [f32(0.6), f32(0.7), f32(0.8)]          # the shape's parameter: "car" gives no amount of its own (a constant is looked up in the material first, texture_params.rs:75-83)

    def render(scene):
        ctx = pkg.Context(0)
        try:
            ctx.upload(scene)
            ctx.film_clear(); ctx.render()
            return ctx.film_rgb()
        finally:
            ctx.close()
    want = render(ps)
    exe = os.path.join(root, "pbrt-r3_amd", "csrc", "pbrt_gpu")
    out = tmp_path / "cli.pfm"
    r = subprocess.run([exe, "-i", str(tmp_path / "s.pbrt"), "--outfile", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer(out.read_bytes().split(b"\n", 3)[3], "<f4").reshape(32, 32, 3)[::-1]
    assert np.array_equal(bits(got), bits(want)) and want.max() > 0
    assert '"rgb amount" [0.6 0.7 0.8]' in text
    other = render(capi.ParsedScene(text=text.replace('"rgb amount" [0.6 0.7 0.8]', '"rgb amount" [0.1 0.1 0.1]'), work_dir=str(tmp_path), mix_materials=True))
    assert not np.array_equal(other, want)


# ---------------------------------------------------------------- 7. refusals, lights, the hooks' limits
def _tiny(fill):
    b = fs.base(res=8, spp=1)
    fs.room(b)
    fill(b)
    b.shape_trianglemesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [0, 1, 2])
    return b


def _refused(ctx, b, status):
    with pytest.raises(capi.PtError) as e:
        ctx.upload(b.build())
    assert e.value.status == status, str(e.value)
    return str(e.value)


def test_upload_refuses_what_the_reference_asserts_on(gpu_ctx):
    def no_bsdf(b):
        b.material_glass(Kr=Z3, Kt=Z3); g = b.cur_material
        b.material_matte(); m = b.cur_material
        b.material_mix(m, g)
    b = _tiny(no_bsdf)
    msg = _refused(gpu_ctx, b, 4)
    mix_i, child_i = b.cur_material, b.cur_material - 2
    assert "material %d (mix)" % mix_i in msg and "child material %d" % child_i in msg, msg

    def none_child(b):
        n = b._add_material(capi.PT_MATERIAL_NONE)
        b.material_matte(); m = b.cur_material
        b.material_mix(n, m)
    b = _tiny(none_child)
    msg = _refused(gpu_ctx, b, 4)
    assert "material %d (mix)" % b.cur_material in msg and "child material %d" % (b.cur_material - 2) in msg and "none" in msg, msg


def test_upload_refuses_a_tree_past_the_caps_with_its_counts(gpu_ctx):
    def five_leaves(b):
        ids = []
        for k in range(5):
            b.material_matte(Kd=(0.1 * (k + 1),) * 3); ids.append(b.cur_material)
        cur = ids[0]
        for k in ids[1:]:
            b.material_mix(cur, k); cur = b.cur_material
    msg = _refused(gpu_ctx, _tiny(five_leaves), 4)
    assert "5 leaves" in msg and "5 lobes" in msg and "%d leaves" % capi.PT_MIX_MAX_LEAVES in msg and "%d lobes" % capi.PT_MIX_MAX_LOBES in msg, msg
    over = MC.mix(MC.mix(C.params("uber", "five"), C.params("uber", "five"), 0.4), MC.mix(C.params("translucent", "four"), C.params("uber", "five"), 0.7), 0.5)
    msg = _refused(gpu_ctx, _tiny(lambda b: MC.apply(b, over)), 4)
    assert "4 leaves" in msg and "19 lobes" in msg, msg


def test_upload_refuses_a_child_that_does_not_precede_the_mix(gpu_ctx):
    def fill(b):
        b.material_matte(); m = b.cur_material
        b.material_mix(m, m)
        b.materials[b.cur_material].tex_kt = b.cur_material + 1          # itself
    assert "smaller" in _refused(gpu_ctx, _tiny(fill), 1)

    def zero(b):
        b.material_matte(); m = b.cur_material
        b.material_mix(m, m)
        b.materials[b.cur_material].tex_kr = 0                           # no child at all
    _refused(gpu_ctx, _tiny(zero), 1)


def test_hooks_refuse_a_per_hit_tree(gpu_ctx):
    def fill(b):
        b.material_matte((0.8, 0.1, 0.1)); i = b.cur_material
        b.material_matte((0.1, 0.1, 0.8)); j = b.cur_material
        b.material_mix(i, j, b.texture_checkerboard(0.2, 0.9, uscale=4.0, vscale=4.0, aamode="none"))
    b = _tiny(fill)
    gpu_ctx.upload(b.build())
    wo, wi, u = hook_inputs(np.random.default_rng(3))
    for call in (lambda: gpu_ctx.bsdf_eval(b.cur_material, wo, wi), lambda: gpu_ctx.bsdf_sample(b.cur_material, wo, u)):
        with pytest.raises(capi.PtError) as e:
            call()
        assert e.value.status == 4


def _amount_scene(amount_of, integ="path_sobol", variant="plain"):
    def mat(b):
        b.material_plastic(Kd=(0.8, 0.1, 0.1), Ks=(0.3,) * 3, roughness=0.2); i = b.cur_material
        b.material_matte((0.1, 0.2, 0.8)); j = b.cur_material
        b.material_mix(i, j, amount_of(b))
    return room_scene(mat, variant, integ)


@pytest.mark.parametrize("integ", ["path_sobol", "directlighting_all", "whitted"])
def test_textured_amount_of_one_value_is_the_constant(gpu_ctx, integ):
    """amount = checkerboard(c, c): the per-hit route evaluates c at every hit and must render what the constant tree renders, bit for bit;
    a checkerboard of two values renders something else."""
    c = (0.3, 0.6, 0.8)
    const = render_everything(gpu_ctx, _amount_scene(lambda b: c, integ))
    same = render_everything(gpu_ctx, _amount_scene(lambda b: b.texture_checkerboard(c, c, uscale=4.0, vscale=4.0, aamode="none"), integ))
    assert np.array_equal(bits(const[0]), bits(same[0])) and np.array_equal(bits(const[2]), bits(same[2])) and const[0].sum() > 0
    two = render_everything(gpu_ctx, _amount_scene(lambda b: b.texture_checkerboard(c, (0.9, 0.1, 0.2), uscale=4.0, vscale=4.0, aamode="none"), integ))
    assert not np.array_equal(bits(const[0]), bits(two[0]))


def test_mix_beside_spot_distant_and_environment_lights_instanced(gpu_ctx):
    """One render through k_shade_mix_inst: an instanced object carrying a mix, a spot, a distant and an infinite light."""
    def mat(b):
        b.material_plastic(Kd=(0.8, 0.1, 0.1), Ks=(0.3,) * 3, roughness=0.2); i = b.cur_material
        b.material_glass(uroughness=0.3, vroughness=0.3); j = b.cur_material
        b.material_mix(i, j, (0.4, 0.5, 0.6))
    b = fs.base(res=32, spp=4)
    fs.room(b, open_top=True)
    b.light_infinite(L=(0.8, 0.9, 1.0))
    b.light_spot(I=(20, 20, 20), frm=(0, 1.5, -3), to=(0, 0, 0), coneangle=40.0, conedelta=10.0)
    b.light_distant(L=(2, 2, 2), frm=(1, 2, -1), to=(0, 0, 0))
    b.object_begin("things")
    mat(b)
    P, N, UV, idx = fs.uv_sphere((-0.7, -0.9, 0.0), 0.9, 8, 12)
    b.shape_trianglemesh(P, idx, N=N, uv=UV)
    b.object_end()
    b.object_instance("things", scenes.transform_translate(0.0, 0.0, 0.0))
    b.object_instance("things", scenes.transform_translate(1.2, 0.6, 0.5))
    g, cnt, film = render_everything(gpu_ctx, b.build())
    assert np.isfinite(film).all() and film[..., :3].max() > 0 and g.sum() > 0
