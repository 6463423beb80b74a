"""Material "fourier" on the device (materials/fourier.rs, core/reflection/fourier.rs).

The hooks are held to the float64 truth tests/fourier_ref.py on four tables -- evaluation within derived bounds, sampling by inversion
-- and to the reference's own recorded numbers.  The rendering kernels of a scene with such a material (the build that knows FourierBSDF,
PT_KERNELS_FOURIER) are held per camera sample to the closed form f Li |cos| with the truth's f, and bit for bit to one another: mix(F,
matte(Kd 0), 1) scales F's lobe by exactly 1 and adds nothing.  After every test the iteration-cap counter of the uploaded scene is 0."""
import numpy as np
import pytest

import bsdf_cases as C
import bsdf_ref as R
import feature_scenes as fs
import fourier_cases as FC
import fourier_ref as FR
from helpers import bits, pkg, scenes
from test_gpu_bsdf_truth import LIGHT, QUAD, UV_X, CAM_ABOVE, CAM_BELOW
from test_gpu_delta_light import Run, add_distant, base
from test_gpu_disney import _closed_form
from test_gpu_translucent import RAY_COUNTERS, assert_same_render, hook_inputs, render_everything, room_scene

pytestmark = pytest.mark.gpu
capi = pkg.capi
Z3, O3 = (0.0,) * 3, (1.0,) * 3


@pytest.fixture(autouse=True)
def no_sample_reached_an_iteration_cap(gpu_ctx):
    """pt_scene_info.fourier_capped of whatever scene the test left uploaded: the device's two inversion loops never ran into their caps."""
    yield
    info = capi.pt_scene_info()
    if gpu_ctx.lib.pt_scene_info_get(gpu_ctx.h, info) == 0:          # (a test that ends on a refused upload leaves no scene)
        assert info.fourier_capped == 0, info.fourier_capped
    gpu_ctx.reset_counters()


def capped(ctx):
    info = capi.pt_scene_info()
    assert ctx.lib.pt_scene_info_get(ctx.h, info) == 0
    return info.fourier_capped


def fourier(name):
    return lambda b: b.material_fourier(table=FC.table(name))


def with_black_mix(b, name):
    """mix(F, matte(Kd 0), amount 1): F's lobe scaled by exactly 1, through a mix tree."""
    b.material_fourier(table=FC.table(name))
    f = b.cur_material
    b.material_matte(Kd=Z3)
    b.material_mix(f, b.cur_material, O3)
    return b.cur_material


# ---------------------------------------------------------------- 1. hooks against the truth
@pytest.mark.parametrize("name", FC.TABLES)
def test_hooks_meet_the_truth(gpu_ctx, name):
    sd = FC.palette()
    gpu_ctx.upload(sd)
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_FOURIER
    mat = sd.material_index[name]
    stats = FC.run_table(name, lambda wo, wi, fl: gpu_ctx.bsdf_eval(mat, wo, wi, fl), lambda wo, u, fl: gpu_ctx.bsdf_sample(mat, wo, u, fl), "gpu")
    print(FC.summary("gpu", name, stats))
    FC.hold_caps_and_medians(stats, name, "gpu")
    assert capped(gpu_ctx) == 0


def test_hooks_meet_the_eight_recorded_numbers(gpu_ctx):
    """tests/fourierbsdf.rs of the reference through pt_bsdf_eval / pt_bsdf_sample, at its own 1e-3 relative."""
    rec = FC.RECORDED
    sd = FC.palette()
    gpu_ctx.upload(sd)
    mat = sd.material_index["roughgold"]
    rel = lambda a, b: abs(float(a) - b) / abs(b)
    wo, wi = FC.normalize32(rec["wo"])[None], FC.normalize32(rec["wi"])[None]
    f, pdf = gpu_ctx.bsdf_eval(mat, wo, wi, R.ALL)
    assert rel(FC.luminance(f)[0], rec["f_y"]) < FC.RECORDED_REL and rel(pdf[0], rec["pdf"]) < FC.RECORDED_REL
    assert rel(gpu_ctx.bsdf_eval(mat, wi, wo, R.ALL)[1][0], rec["pdf_swapped"]) < FC.RECORDED_REL
    f, swi, pdf, typ = gpu_ctx.bsdf_sample(mat, wo, np.array([rec["u"]], np.float32), R.ALL)
    assert typ[0] == FR.TYPE                                                     # the returned type is 0: BSDF::sample_f reports the lobe's own
    assert rel(FC.luminance(f)[0], rec["sample_f_y"]) < FC.RECORDED_REL and rel(pdf[0], rec["sample_pdf"]) < FC.RECORDED_REL
    for k in range(3):
        assert rel(swi[0, k], rec["sample_wi"][k]) < FC.RECORDED_REL


def test_hooks_through_a_mix_are_the_lobes_own(gpu_ctx):
    """mix(F, matte(Kd 0), 1) returns what F returns, bit for bit: f, pdf and all four outputs of sample_f."""
    b = fs.base(res=8, spp=1)
    fs.room(b)
    index = {}
    for k, name in enumerate(("roughgold", "two_sided", "rgb_long")):
        b.material_fourier(table=FC.table(name)); index[name] = b.cur_material
        b.shape_trianglemesh([(0.1 * k, 0, 0), (0.1 * k + 0.05, 0, 0), (0.1 * k, 0.05, 0)], [0, 1, 2])
        index[name + "/mix"] = with_black_mix(b, name)
        b.shape_trianglemesh([(0.1 * k, 0.1, 0), (0.1 * k + 0.05, 0.1, 0), (0.1 * k, 0.15, 0)], [0, 1, 2])
    sd = b.build()
    assert len(sd.fourier_tables) == 3 and len(sd.fourier) == 6            # tables are shared: two materials name each
    gpu_ctx.upload(sd)
    wo, wi, u = hook_inputs(np.random.default_rng(71))
    for name in ("roughgold", "two_sided", "rgb_long"):
        for _, fl in C.FLAG_SETS:
            ea, em = gpu_ctx.bsdf_eval(index[name], wo, wi, fl), gpu_ctx.bsdf_eval(index[name + "/mix"], wo, wi, fl)
            assert np.array_equal(bits(ea[0]), bits(em[0])) and np.array_equal(bits(ea[1]), bits(em[1])), (name, fl)
            sa, sm = gpu_ctx.bsdf_sample(index[name], wo, u, fl), gpu_ctx.bsdf_sample(index[name + "/mix"], wo, u, fl)
            assert np.array_equal(sa[3], sm[3]) and all(np.array_equal(bits(sa[j]), bits(sm[j])) for j in range(3)), (name, fl)
        assert (gpu_ctx.bsdf_eval(index[name], wo, wi, R.ALL)[0] != 0).any(), name


# ---------------------------------------------------------------- 2. closed form per camera sample
def _lit_run(ctx, integ, cam, material):
    """test_gpu_bsdf_truth's quad under the distant light, 32 x 32 at one sample per pixel."""
    sb = base(integ, "sobol", res=32, spp=1, maxdepth=1 if integ == "path" else 5)
    sb.look_at(cam, (0, 0, 0), (0, 0, 1))
    material(sb)
    sb.shape_trianglemesh([QUAD[0], QUAD[2], 0.0, QUAD[1], QUAD[2], 0.0, QUAD[1], QUAD[3], 0.0, QUAD[0], QUAD[3], 0.0], [0, 1, 2, 0, 2, 3], uv=UV_X)
    add_distant(sb, **LIGHT)
    return Run(ctx, sb.build())


@pytest.mark.parametrize("integ", ["path", "all", "whitted"])
@pytest.mark.parametrize("name", ["roughgold", "two_sided"])
def test_lit_quad_renders_the_truths_f(gpu_ctx, name, integ):
    """Per camera sample the radiance is f(wo, wi) L |cos| with fourier_ref's f on the quad's frame, within the bound check_closed_form
    derives.  Rough gold is seen from above; two_sided from below, lit from behind: what the table transmits.  In whitted the lobe matches
    neither specular request, so direct lighting is all there is."""
    run = _lit_run(gpu_ctx, integ, CAM_BELOW if name == "two_sided" else CAM_ABOVE, fourier(name))
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_FOURIER
    truth = FR.FrameTruth(FC.truth(name))
    n_lit, skip, hit = _closed_form(run, lambda p: ([(truth, np.ones(len(p), bool))], np.zeros(len(p), bool)))
    assert n_lit > 300, n_lit
    assert len(np.unique(bits(run.rad[(run.rad > 0).any(1)]))) > 50
    assert skip.mean() <= C.MAX_LEFT_OUT


# ---------------------------------------------------------------- 3. the kernel families
def _family_pair(name, cylinder):
    def shapes_first(b):
        if cylinder:
            b.material_matte((0.6, 0.6, 0.7))
            t = scenes.transform_translate(0.6, 1.0, 0.2)
            b.shape_cylinder(radius=0.4, zmin=-0.5, zmax=0.6, object_to_world=t[0], world_to_object=t[1])

    def alone(b):
        shapes_first(b)
        b.material_fourier(table=FC.table(name))

    def mixed(b):
        shapes_first(b)
        with_black_mix(b, name)
    return mixed, alone


@pytest.mark.parametrize("variant", ["plain", "inst", "cylinder"])
@pytest.mark.parametrize("name", ["roughgold", "two_sided"])
def test_render_equals_the_material_under_a_mix(gpu_ctx, name, variant):
    """F alone and mix(F, matte(Kd 0), 1) render bit-equal in every integrator, in a world scene, an instanced scene and a scene with a
    cylinder.  The render differs from the same room with a matte in F's place, and the counters are finite and non-zero."""
    room = "plain" if variant == "cylinder" else variant
    pair = _family_pair(name, variant == "cylinder")
    assert_same_render(gpu_ctx, pair, room, res=16, tag="%s %s" % (name, variant))
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_FOURIER
    for integ in ("path_sobol", "whitted"):
        g, cnt, film = render_everything(gpu_ctx, room_scene(pair[1], room, integ, res=16))
        gm = render_everything(gpu_ctx, room_scene(lambda b: b.material_matte((0.6, 0.45, 0.3)), room, integ, res=16))[0]
        assert not np.array_equal(bits(g), bits(gm)), (name, variant, integ)
        assert np.isfinite(g).all() and np.isfinite(film).all() and g.sum() > 0
        assert cnt["camera_rays"] > 0 and cnt["shadow_rays"] > 0 and cnt["nodes_visited"] > 0
        if integ == "path_sobol":
            for k in RAY_COUNTERS:
                assert cnt[k] > 0, (k, cnt[k])


def test_a_moving_scene_renders_and_a_still_one_equals_its_motionless_twin(gpu_ctx):
    """The sixth build contains the fifth: a camera that does not actually move renders what the scene without motion renders, one that
    does renders something else, both through PT_KERNELS_FOURIER."""
    def scene(end):
        b = fs.base(res=16, spp=4, depth=3)
        fs.room(b)
        b.material_fourier(table=FC.table("roughgold"))
        b.shape_trianglemesh([(-1.2, -1.2, -0.5), (1.2, -1.2, -0.5), (1.2, 1.2, -0.2), (-1.2, 1.2, -0.2)], [0, 1, 2, 0, 2, 3], uv=[(0, 0), (1, 0), (1, 1), (0, 1)])
        if end is not None:
            b.camera_to_world_end_m = np.asarray(b.camera_to_world, np.float32).copy()
            b.camera_to_world_end_m[3] += np.float32(end)
        return b.build()
    tile = (0, 0, 16, 16)
    gpu_ctx.upload(scene(None))
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_FOURIER
    still = gpu_ctx.radiance_samples(tile)
    gpu_ctx.upload(scene(0.0))
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_FOURIER
    assert np.array_equal(bits(gpu_ctx.radiance_samples(tile)), bits(still)) and still.sum() > 0
    gpu_ctx.upload(scene(0.3))
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_FOURIER
    moved = gpu_ctx.radiance_samples(tile)
    assert np.isfinite(moved).all() and not np.array_equal(bits(moved), bits(still))


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


def test_bumped_fourier_has_the_bumped_mattes_shading_normal(gpu_ctx):
    """material_bump comes first in either material (fourier.rs:30-33, matte.rs): aov's ns is bit-equal; without the bump map it is not."""
    bump = lambda b: b.texture_checkerboard(0.0, 0.03, uscale=6.0, vscale=6.0)
    f = _aov_ns(gpu_ctx, lambda b: b.material_fourier(table=FC.table("rgb_long"), bumpmap=bump(b)))
    m = _aov_ns(gpu_ctx, lambda b: b.material_matte(Kd=(0.6, 0.45, 0.3), bumpmap=bump(b)))
    flat = _aov_ns(gpu_ctx, lambda b: b.material_fourier(table=FC.table("rgb_long")))
    assert np.array_equal(bits(f), bits(m)) and f.max() > 0
    assert not np.array_equal(bits(f), bits(flat))


def test_a_bumped_fourier_surface_is_shaded_with_its_lobe(gpu_ctx):
    """The per-hit route (a bump map makes the material texture-driven): a bump map of height 0 everywhere renders what the material
    without one renders, in path, directlighting and whitted, alone and under a mix; a real one renders something else."""
    flat_bump = lambda b: b.texture_checkerboard(0.0, 0.0, uscale=6.0, vscale=6.0)
    real_bump = lambda b: b.texture_checkerboard(0.0, 0.05, uscale=6.0, vscale=6.0)
    for integ in ("path_sobol", "directlighting_all", "whitted"):
        plain = render_everything(gpu_ctx, room_scene(fourier("rgb_long"), "plain", integ, res=16))[0]
        zero = render_everything(gpu_ctx, room_scene(lambda b: b.material_fourier(table=FC.table("rgb_long"), bumpmap=flat_bump(b)), "plain", integ, res=16))[0]
        bent = render_everything(gpu_ctx, room_scene(lambda b: b.material_fourier(table=FC.table("rgb_long"), bumpmap=real_bump(b)), "plain", integ, res=16))[0]
        assert plain.sum() > 0 and np.array_equal(bits(plain), bits(zero)), integ
        assert np.isfinite(bent).all() and not np.array_equal(bits(plain), bits(bent)), integ

    def mixed(b):
        b.material_fourier(table=FC.table("rgb_long"), bumpmap=real_bump(b)); f = b.cur_material
        b.material_matte(Kd=Z3)
        b.material_mix(f, b.cur_material, O3)
    a = render_everything(gpu_ctx, room_scene(mixed, "plain", "path_sobol", res=16))[0]
    c = render_everything(gpu_ctx, room_scene(lambda b: b.material_fourier(table=FC.table("rgb_long"), bumpmap=real_bump(b)), "plain", "path_sobol", res=16))[0]
    assert np.array_equal(bits(a), bits(c))


# ---------------------------------------------------------------- the two halves under MIS
def test_path_mis_carries_the_reported_pdfs(gpu_ctx, name="roughgold"):
    """A rough-gold plane under one triangle light around the mirror direction (the lobe's pdf there is of the light's own magnitude, so the
    weights matter; under a smooth table they would not, and the check could not tell), `path` at maxdepth 1: every camera sample is one estimate_direct, whose light half weighs by
    the lobe's reported pdf and whose BSDF half draws from it and divides by it.  Mean and variance come from fourier_ref by quadrature in
    float64 (fourier_cases.mis_moments); the frame's mean must lie within five standard errors, and a pdf that were off by a factor of 2
    (or 1/2) in the weights would not."""
    res, spp = 4, 256                           # few pixels: the quadrature is per pixel centre, and the view is 20 degrees wide
    n = res * res * spp
    mean, var = FC.mis_moments(name, res=res)
    bound = 5.0 * np.sqrt(var / n)              # five standard errors: a condition on the false-alarm rate (the Sobol' points do better)
    for factor in (2.0, 0.5):
        assert (np.abs(FC.mis_moments(name, factor, res=res)[0] - mean) > bound).all(), "the test could not tell another pdf"
    b = scenes.SceneBuilder()
    b.look_at((0, 0, 1), (0, 0, 0), (0, 1, 0))
    b.camera_perspective(fov=FC.MIS_FOV)
    b.film(xresolution=res, yresolution=res)
    b.pixel_filter_box()
    b.sampler_sobol(spp)
    b.integrator_path(maxdepth=1)
    b.material_fourier(table=FC.table(name))
    b.shape_trianglemesh([-1000, -1000, 0, 1000, -1000, 0, 1000, 1000, 0, -1000, 1000, 0], [0, 1, 2, 0, 2, 3])
    b.material_matte(Kd=Z3)
    b.area_light_source_diffuse(L=(1.0, 1.0, 1.0), twosided=True)
    b.shape_trianglemesh([c for v in FC.MIS_LIGHT for c in v], [0, 1, 2])
    gpu_ctx.upload(b.build())
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_FOURIER
    g = gpu_ctx.radiance_samples((0, 0, res, res)).reshape(-1, 3).astype(np.float64)
    assert len(g) == n
    got = g.mean(0)
    print("\npath under MIS, %s: mean %s, quadrature %s, bound %s" % (name, got, mean, bound))
    assert (np.abs(got - mean) <= bound).all(), (got, mean, bound)


# ---------------------------------------------------------------- 4. which build runs what
def test_every_other_scene_reports_its_old_build_set(gpu_ctx):
    def mat_scene(fill):
        return room_scene(fill, "plain", "path_sobol", res=8)
    gpu_ctx.upload(mat_scene(lambda b: b.material_matte((0.5, 0.4, 0.3))))
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_BASE

    def cyl(b):
        b.material_matte((0.6, 0.6, 0.7))
        t = scenes.transform_translate(0.6, 1.0, 0.2)
        b.shape_cylinder(radius=0.4, zmin=-0.5, zmax=0.6, object_to_world=t[0], world_to_object=t[1])
    gpu_ctx.upload(mat_scene(cyl))
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_QUADRIC
    gpu_ctx.upload(mat_scene(lambda b: b.material_disney(sheen=0.5)))
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_DISNEY

    def gonio(b):
        b.material_matte((0.5, 0.4, 0.3))
        b.light_goniometric(L=(2.0, 2.0, 2.0))
    gpu_ctx.upload(mat_scene(gonio))
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_MAP_LIGHT

    def moving(end):
        def fill(b):
            b.material_matte((0.5, 0.4, 0.3))
            m = np.asarray(b.camera_to_world, np.float32).copy()
            m[3] += np.float32(end)
            b.camera_to_world_end(m)
        return fill
    gpu_ctx.upload(mat_scene(moving(0.3)))                    # a camera that moves, no table: the fifth build, as before
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_MOTION
    moved = gpu_ctx.radiance_samples((0, 0, 8, 8))
    gpu_ctx.upload(mat_scene(moving(0.0)))                    # motion records whose ends are equal: not a moving scene, the first build
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_BASE
    still = gpu_ctx.radiance_samples((0, 0, 8, 8))
    gpu_ctx.upload(mat_scene(lambda b: b.material_matte((0.5, 0.4, 0.3))))
    assert np.array_equal(bits(gpu_ctx.radiance_samples((0, 0, 8, 8))), bits(still)) and not np.array_equal(bits(moved), bits(still))
    gpu_ctx.upload(mat_scene(fourier("two_sided")))
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_FOURIER
    gpu_ctx.upload(mat_scene(lambda b: b.material_matte((0.5, 0.4, 0.3))))          # and back: nothing of the table scene stays behind
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_BASE and capped(gpu_ctx) == 0


# ---------------------------------------------------------------- 5. refusals
def _tiny(fill):
    b = fs.base(res=8, spp=1)
    fs.room(b)
    fill(b)
    b.shape_trianglemesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [0, 1, 2])
    return b


def _refused(ctx, sd, status=1):
    with pytest.raises(capi.PtError) as e:
        ctx.upload(sd)
    assert e.value.status == status, str(e.value)
    return str(e.value)


def _edited(name, **kw):
    """A copy of a table with some header fields or arrays replaced."""
    t = FC.table(name)
    f = dict(mu=t.mu.copy(), cdf=t.cdf.copy(), offset_and_length=t.offset_and_length.copy(), a=t.a.copy(), n_channels=t.n_channels, m_max=t.m_max, eta=t.eta)
    edit = kw.pop("edit", None)
    f.update(kw)
    if edit:
        edit(f)
    return capi.FourierTable(**f)


def test_upload_refuses_bad_records_and_bad_tables(gpu_ctx):
    fresh = lambda: _tiny(fourier("two_sided")).build()            # (a build hands out the builder's own record objects: a new builder per edit)
    sd = fresh()
    sd.fourier[0].material = 1000
    assert "material index" in _refused(gpu_ctx, sd)
    sd = fresh()
    sd.fourier[0].table = 7
    assert "table index" in _refused(gpu_ctx, sd)
    sd = fresh()
    sd.fourier[0].material = 0                                   # the room's matte
    assert "not a Fourier" in _refused(gpu_ctx, sd)
    sd = fresh()
    sd.fourier = sd.fourier + [capi.pt_fourier.from_buffer_copy(bytes(memoryview(sd.fourier[0]).cast("B")))]
    assert "two records" in _refused(gpu_ctx, sd)
    b2 = _tiny(fourier("two_sided"))
    b2.material_fourier(table=FC.table("dark"))
    b2.shape_trianglemesh([(0, 0, 1), (1, 0, 1), (0, 1, 1)], [0, 1, 2])
    sd = b2.build()
    sd.fourier = sd.fourier[:1]                                  # a PT_MATERIAL_FOURIER material without a record
    assert "no record" in _refused(gpu_ctx, sd)
    # tables that never were a file: the upload runs the reader's validation
    L = lambda f, pair, col, v: f["offset_and_length"].__setitem__(2 * pair + col, v)
    n_coeffs = FC.table("two_sided").n_coeffs
    bad = {
        "n_channels is 2": _edited("two_sided", n_channels=2),
        "n_mu is 1": _edited("two_sided", n_mu=1),
        "mu steps back": _edited("two_sided", edit=lambda f: f["mu"].__setitem__(2, -0.7)),
        "mu repeats at node 2 and the cdf columns": _edited("two_sided", edit=lambda f: f["mu"].__setitem__(2, -0.6)),
        "not finite": _edited("two_sided", edit=lambda f: f["mu"].__setitem__(1, np.inf)),
        "negative length": _edited("two_sided", edit=lambda f: L(f, 3, 1, -1)),
        "above m_max": _edited("two_sided", edit=lambda f: L(f, 3, 1, 6)),
        "negative offset": _edited("two_sided", edit=lambda f: L(f, 3, 0, -1)),
        "past the end": _edited("two_sided", edit=lambda f: L(f, 3, 0, n_coeffs - 1)),
    }
    for phrase, table in bad.items():
        msg = _refused(gpu_ctx, _tiny(lambda b: b.material_fourier(table=table)).build())
        assert phrase in msg and "table 0" in msg, (phrase, msg)
    gpu_ctx.upload(fresh())                                      # and the context is usable afterwards
    assert gpu_ctx.kernel_set() == capi.PT_KERNELS_FOURIER
