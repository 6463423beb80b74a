"""Material "translucent" on the device (materials/translucent.rs, core/reflection/lambertian.rs:49-99).

Three of its four lobes are lobe kinds `uber` and `glass` already produce, and the oracle pins those two bit for bit
(tests/test_materials.py), so configurations of translucent are held bit for bit to their uber / glass equivalents -- through the
BSDF hooks and through every integrator, kernel family and parameter route.  The fourth lobe, LambertianTransmission, is held to
tests/translucent_ref.py: bit for bit through the hooks, through Whitted's direct term against a mirrored matte scene, and under
MIS against a quadrature that carries the reference's pdf without INV_PI."""
import os
import subprocess

import numpy as np
import pytest

import feature_scenes as fs
import translucent_ref as tr
from helpers import bits, pkg, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ALL, NOSPEC, REFL_ONLY = 31, 31 & ~16, 1 | 4 | 8 | 16
Z3, O3 = (0.0,) * 3, (1.0,) * 3


def prod32(a, b):
    """The colour build_lobes forms: a float32 product per channel."""
    return tuple(float(f32(x) * f32(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------- the two equivalence families, and "no BSDF"
def pair_uber(kd, ks, rho, remap):
    """translucent(Kd, Ks, reflect 1, transmit 0) == uber(Kd, Ks, Kr 0, Kt 0, opacity 1, index 1.5): LambertianReflection(1 * Kd) and
    MicrofacetReflection(1 * Ks, FresnelDielectric(1, 1.5), TrowbridgeReitz(rough, rough)), BSDF eta 1.5."""
    return (lambda b: b.material_translucent(Kd=kd, Ks=ks, reflect=O3, transmit=Z3, roughness=rho, remaproughness=remap),
            lambda b: b.material_uber(Kd=kd, Ks=ks, Kr=Z3, Kt=Z3, opacity=O3, eta=1.5, roughness=rho, remaproughness=remap))


def pair_glass(s, a, t, rho, remap):
    """translucent(Kd 0, Ks s, reflect a, transmit t, roughness rho != 0) == glass(Kr a * s, Kt t * s, uroughness = vroughness = rho, index 1.5)."""
    return (lambda b: b.material_translucent(Kd=Z3, Ks=s, reflect=a, transmit=t, roughness=rho, remaproughness=remap),
            lambda b: b.material_glass(Kr=prod32(a, s), Kt=prod32(t, s), eta=1.5, uroughness=rho, vroughness=rho, remaproughness=remap))


def pair_no_bsdf():
    return (lambda b: b.material_translucent(Kd=(0.5, 0.4, 0.3), reflect=Z3, transmit=Z3), lambda b: b.material_glass(Kr=Z3, Kt=Z3))


def pair_textured_uber():
    """Kd and roughness behind checkerboards: the per-hit route (k_tex_resolve + k_shade_general_res, textured_lobes elsewhere)."""
    def tex(b):
        return (b.texture_checkerboard((0.8, 0.3, 0.2), (0.1, 0.3, 0.7), uscale=5.0, vscale=5.0),
                b.texture_checkerboard(0.05, 0.4, uscale=3.0, vscale=3.0, aamode="none"))

    def a(b):
        kd, ro = tex(b)
        b.material_translucent(Kd=kd, Ks=(0.4, 0.4, 0.4), reflect=O3, transmit=Z3, roughness=ro)

    def c(b):
        kd, ro = tex(b)
        b.material_uber(Kd=kd, Ks=(0.4, 0.4, 0.4), Kr=Z3, Kt=Z3, opacity=O3, eta=1.5, roughness=ro)
    return a, c


def pair_textured_no_bsdf():
    """reflect = checkerboard(1, 0) with transmit 0: "no BSDF" alternates from hit to hit, as glass with Kr = checkerboard(s, 0) does.
    (aamode none: the checks are exactly tex1 or tex2, so 1 * s and s are the same float.)"""
    s = (0.7, 0.6, 0.5)

    def a(b):
        b.material_translucent(Kd=Z3, Ks=s, reflect=b.texture_checkerboard(O3, Z3, uscale=4.0, vscale=4.0, aamode="none"), transmit=Z3, roughness=0.2)

    def c(b):
        b.material_glass(Kr=b.texture_checkerboard(s, Z3, uscale=4.0, vscale=4.0, aamode="none"), Kt=Z3, eta=1.5, uroughness=0.2, vroughness=0.2)
    return a, c


PAIRS = {
    "uber": lambda: pair_uber((0.5, 0.3, 0.2), (0.3, 0.4, 0.5), 0.15, True),
    "glass": lambda: pair_glass((0.8, 0.7, 0.6), (0.9, 0.5, 0.7), (0.6, 0.9, 0.8), 0.2, True),
    "no_bsdf": pair_no_bsdf,
}
RAY_COUNTERS = ("camera_rays", "regular_rays", "shadow_rays", "path_vertices", "nodes_visited", "tris_tested")
INTEGRATORS = ["path_sobol", "path_halton", "directlighting_all", "directlighting_one", "whitted", "ao"]


def room_scene(mat, variant="plain", integrator="path_sobol", res=32, spp=4):
    """The room of feature_scenes with a smooth-shaded blob and a slab carrying `mat` (both with uvs).  variant: "env" opens the top under an
    environment light (the _env kernels), "inst" puts the objects into an object instanced twice (_inst), "sphere" adds analytic spheres."""
    T = scenes
    b = fs.base(res=res, spp=spp, depth=5)
    if integrator == "path_halton":
        b.sampler_halton(spp)
    if integrator.startswith("directlighting"):
        b.integrator_directlighting(maxdepth=4, strategy=integrator.split("_")[1])
    elif integrator == "whitted":
        b.integrator_whitted(maxdepth=4)
    elif integrator == "ao":
        b.integrator_ao(nsamples=8)
    fs.room(b, open_top=variant == "env")
    if variant == "env":
        b.light_infinite(L=(0.8, 0.9, 1.0))

    def objects():
        mat(b)
        P, N, UV, idx = fs.uv_sphere((-0.7, -0.9, 0.0), 0.9, 8, 12)
        b.shape_trianglemesh(P, idx, N=N, uv=UV)
        b.shape_trianglemesh([(0.2, -1.8, -0.8), (1.8, -1.8, -0.8), (1.8, 0.3, 0.9), (0.2, 0.3, 0.9)], [0, 1, 2, 0, 2, 3], uv=[(0, 0), (1, 0), (1, 1), (0, 1)])
    if variant == "inst":
        b.object_begin("things")
        objects()
        b.object_end()
        b.object_instance("things", T.transform_translate(0.0, 0.0, 0.0))
        b.object_instance("things", T.transform_mul(T.transform_translate(0.3, 1.2, 1.0), T.transform_scale(0.5, -0.5, 0.5)))
    else:
        objects()
    if variant == "sphere":
        t = T.transform_translate(0.6, 1.0, 0.4)
        b.shape_sphere(radius=0.55, object_to_world=t[0], world_to_object=t[1])
        b.material_matte((0.6, 0.6, 0.7))
        t = T.transform_translate(-1.2, 1.0, 0.8)
        b.shape_sphere(radius=0.4, object_to_world=t[0], world_to_object=t[1])
    return b.build()


def render_everything(ctx, sd):
    info = ctx.upload(sd)
    g = ctx.radiance_samples(tuple(info.sample_bounds))
    ctx.film_clear(); ctx.reset_counters(); ctx.render()
    return g, ctx.counters(), ctx.film_xyzw()


def assert_same_render(ctx, pair, variant, integrators=INTEGRATORS, res=32, tag=""):
    a, c = pair
    for integ in integrators:
        ga, ca, fa = render_everything(ctx, room_scene(a, variant, integ, res=res))
        gc, cc, fc = render_everything(ctx, room_scene(c, variant, integ, res=res))
        assert ga.sum() > 0, (tag, variant, integ)
        bad = (bits(ga) != bits(gc)).any(axis=-1)
        assert not bad.any(), (tag, variant, integ, "per-sample radiance", int(bad.sum()), bad.size)
        for k in RAY_COUNTERS:         # (the other entries are timings and how many node fetches LDS served, which depends on scheduling)
            assert ca[k] == cc[k], (tag, variant, integ, k, ca[k], cc[k])
        assert np.array_equal(bits(fa), bits(fc)), (tag, variant, integ, "film")


# ---------------------------------------------------------------- 1. hooks: oracle-backed equivalences, bit for bit
def hook_inputs(rng, n=4096):
    """The inputs of test_materials.py::test_gpu_bsdf_eval_and_sample_bit_exact: near-normal, grazing, wo.z == 0, the mirror direction, wh = 0,
    u at 0 and just below 1."""
    def dirs(k):
        v = rng.standard_normal((k, 3)).astype(np.float32)
        return (v / np.linalg.norm(v, axis=1, keepdims=True).astype(np.float32)).astype(np.float32)
    wo, wi = dirs(n), dirs(n)
    wo[:200, 2] = 1.0; wo[:200, :2] *= 1e-3
    wo[:200] /= np.linalg.norm(wo[:200], axis=1, keepdims=True)
    wo[200:300, 2] *= 1e-4
    wo[300] = (1, 0, 0)
    wi[:100] = wo[:100] * np.array([-1, -1, 1], np.float32)
    wi[100:150] = -wo[100:150]
    u = rng.random((n, 2), dtype=np.float32)
    u[:50, 0] = 0.0; u[50:100, 1] = 0.0; u[100:150, 0] = np.float32(0.99999994)
    return wo, wi, u


def palette(entries):
    """One small triangle per material: the scene only carries the material table for the BSDF hooks."""
    b = fs.base(res=16, spp=1)
    fs.room(b)
    index = {}
    for k, (name, fn) in enumerate(entries):
        fn(b)
        index[name] = b.cur_material
        x = -1.9 + 0.15 * k
        b.shape_trianglemesh([(x, -1.9, 0), (x + 0.1, -1.9, 0), (x, -1.8, 0)], [0, 1, 2])
    return b.build(), index


def test_hooks_equal_uber_and_glass_bit_for_bit(gpu_ctx):
    kd, ks, s = (0.5, 0.3, 0.2), (0.3, 0.4, 0.5), (0.8, 0.7, 0.6)
    pos_a, pos_t = (0.9, 0.5, 0.7), (0.6, 0.9, 0.8)
    entries, names = [], []
    for remap in (True, False):
        cases = [("uber", pair_uber(kd, ks, 0.15, remap))]
        cases += [("glass_%d%d" % (bool(any(a)), bool(any(t))), pair_glass(s, a, t, 0.2, remap)) for a, t in ((pos_a, Z3), (Z3, pos_t), (pos_a, pos_t))]
        for name, (a, c) in cases:
            n = "%s_remap%d" % (name, remap)
            entries += [(n + "/translucent", a), (n + "/equivalent", c)]
            names.append(n)
    sd, index = palette(entries)
    gpu_ctx.upload(sd)
    wo, wi, u = hook_inputs(np.random.default_rng(31))
    for n in names:
        ma, mc = index[n + "/translucent"], index[n + "/equivalent"]
        assert ma != mc
        for flags in (ALL, NOSPEC, REFL_ONLY):
            fa, pa = gpu_ctx.bsdf_eval(ma, wo, wi, flags)
            fc, pc = gpu_ctx.bsdf_eval(mc, wo, wi, flags)
            assert np.array_equal(bits(fa), bits(fc)) and np.array_equal(bits(pa), bits(pc)), (n, flags)
            sa = gpu_ctx.bsdf_sample(ma, wo, u, flags)
            sc = gpu_ctx.bsdf_sample(mc, wo, u, flags)
            assert np.array_equal(sa[3], sc[3]), (n, flags, "sampled type")
            for x, y, what in zip(sa[:3], sc[:3], ("f", "wi", "pdf")):
                assert np.array_equal(bits(x), bits(y)), (n, flags, what)
        assert (gpu_ctx.bsdf_sample(ma, wo, u, ALL)[3] != 0).mean() > 0.5, n           # and it does scatter


# ---------------------------------------------------------------- 2. hooks: the new lobe against the float32 restatement
DIFFUSE_ONLY = [("transmit_only", (0.6, 0.5, 0.4), Z3, O3), ("half_half_coloured", (0.7, 0.2, 0.45), (0.5,) * 3, (0.5,) * 3)]


def test_hooks_lambertian_transmission_bit_for_bit(gpu_ctx):
    sd, index = palette([(n, (lambda kd, r, t: lambda b: b.material_translucent(Kd=kd, Ks=Z3, reflect=r, transmit=t))(kd, r, t)) for n, kd, r, t in DIFFUSE_ONLY])
    gpu_ctx.upload(sd)
    wo, wi, u = hook_inputs(np.random.default_rng(37))
    for n, kd, r, t in DIFFUSE_ONLY:
        ls = tr.diffuse_f32_lobes(kd, r, t)
        for flags in (ALL, NOSPEC, REFL_ONLY):
            gf, gp = gpu_ctx.bsdf_eval(index[n], wo, wi, flags)
            wf, wp = tr.diffuse_f32_eval(ls, wo, wi, flags)
            assert np.array_equal(bits(gf), bits(wf)), (n, flags, "f", int((bits(gf) != bits(wf)).any(axis=1).sum()))
            assert np.array_equal(bits(gp), bits(wp)), (n, flags, "pdf", int((bits(gp) != bits(wp)).sum()))
        # the quirk itself, through the device: the transmission pdf is |cos|, not |cos| / pi
        far = (wo[:, 2] * wi[:, 2] < 0)
        gf, gp = gpu_ctx.bsdf_eval(index[n], wo, wi, ALL)
        n_match = len(ls)
        assert np.array_equal(bits(gp[far]), bits((np.abs(wi[far, 2]) / f32(n_match)).astype(f32)))
        # sample_f
        sf, swi, sp, st = gpu_ctx.bsdf_sample(index[n], wo, u, ALL)
        ok = st != 0
        assert ok.mean() > 0.9 and not ok[300]                      # wo.z == 0 returns None
        wf, wp = tr.diffuse_f32_eval(ls, wo, swi, ALL)
        assert np.array_equal(bits(sf[ok]), bits(wf[ok])) and np.array_equal(bits(sp[ok]), bits(wp[ok])), n
        rf, rwi, rp, rt = tr.bsdf_sample_f(tr.lobes(Kd=kd, Ks=Z3, reflect=r, transmit=t), wo, u, ALL)
        cmp = ok & (rt != 0)            # (u.x times a matching count of 1 or 2 is exact in float32 and float64 alike: the same lobe, the same remapped u)
        assert cmp.sum() > 0.9 * len(u)
        assert np.array_equal(st[cmp], rt[cmp]), n
        # x, y: about eight float32 roundings of a value <= 1 against the float64 concentric map
        assert np.abs(swi[cmp, :2].astype(np.float64) - rwi[cmp, :2]).max() <= 1e-6, n
        # z from the returned x, y, in float32 (the square root is ill-conditioned at grazing angles: checked from its own inputs)
        x, y = swi[:, 0], swi[:, 1]
        z = np.sqrt(np.maximum(f32(0), ((f32(1) - x * x).astype(f32) - (y * y).astype(f32)).astype(f32))).astype(f32)
        trans = (st & tr.TRANS) != 0
        sign = np.where(trans, -np.sign(wo[:, 2]), np.sign(wo[:, 2])).astype(f32)
        assert np.array_equal(bits(swi[ok, 2]), bits((sign * z)[ok])), n
        assert (swi[ok & trans, 2] * wo[ok & trans, 2] < 0).all()
        if n == "transmit_only":
            assert (st[ok] == (tr.TRANS | tr.DIFFUSE)).all()
        else:
            assert set(np.unique(st[ok])) == {tr.TRANS | tr.DIFFUSE, tr.REFL | tr.DIFFUSE}
            assert (trans[ok] == (u[ok, 0] >= 0.5)).all()              # lobe order: reflection first (translucent.rs:63-70)


def test_hooks_four_lobes_compose_bit_for_bit(gpu_ctx):
    """All four lobes in one list: BSDF::f sums, in the order the material adds them, the lobes on the side the geometric normal selects, and
    BSDF::pdf averages all four.  Each single lobe comes from a material that has only that lobe; the sums are formed in float32."""
    kd, ks, a, t, rho = (0.5, 0.3, 0.2), (0.3, 0.4, 0.5), (0.9, 0.5, 0.7), (0.6, 0.9, 0.8), 0.25
    sd, index = palette([
        ("all", lambda b: b.material_translucent(Kd=kd, Ks=ks, reflect=a, transmit=t, roughness=rho)),
        ("refl", lambda b: b.material_uber(Kd=prod32(a, kd), Ks=prod32(a, ks), eta=1.5, roughness=rho)),
        ("lr", lambda b: b.material_uber(Kd=prod32(a, kd), Ks=Z3, eta=1.5, roughness=rho)),
        ("lt", lambda b: b.material_translucent(Kd=kd, Ks=Z3, reflect=Z3, transmit=t)),
        ("mr", lambda b: b.material_glass(Kr=prod32(a, ks), Kt=Z3, eta=1.5, uroughness=rho, vroughness=rho)),
        ("mt", lambda b: b.material_glass(Kr=Z3, Kt=prod32(t, ks), eta=1.5, uroughness=rho, vroughness=rho))])
    gpu_ctx.upload(sd)
    wo, wi, u = hook_inputs(np.random.default_rng(41))
    ev = {k: gpu_ctx.bsdf_eval(m, wo, wi, ALL) for k, m in index.items()}
    reflect = (wo[:, 2] * wi[:, 2] > 0)[:, None]
    want_f = np.where(reflect, ev["refl"][0], (ev["lt"][0] + ev["mt"][0]).astype(f32))
    want_p = ((((ev["lr"][1] + ev["lt"][1]).astype(f32) + ev["mr"][1]).astype(f32) + ev["mt"][1]).astype(f32) / f32(4)).astype(f32)
    assert np.array_equal(bits(ev["all"][0]), bits(want_f))
    assert np.array_equal(bits(ev["all"][1]), bits(want_p))
    st = gpu_ctx.bsdf_sample(index["all"], wo, u, ALL)[3]
    assert set(np.unique(st)) == {0, 1 | 4, 2 | 4, 1 | 8, 2 | 8}
    # whitted's question to the material: no specular lobe in either direction
    assert (gpu_ctx.bsdf_sample(index["all"], wo, u, 16 | 1)[3] == 0).all() and (gpu_ctx.bsdf_sample(index["all"], wo, u, 16 | 2)[3] == 0).all()


# ---------------------------------------------------------------- 3. renders, bit for bit against the equivalents
@pytest.mark.parametrize("variant", ["plain", "env", "inst", "sphere"])
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_render_equals_equivalent(gpu_ctx, pair, variant):
    assert_same_render(gpu_ctx, PAIRS[pair](), variant, tag=pair)


@pytest.mark.parametrize("variant", ["plain", "env", "inst", "sphere"])
@pytest.mark.parametrize("pair", ["textured_uber", "textured_no_bsdf"])
def test_render_equals_equivalent_textured(gpu_ctx, pair, variant):
    assert_same_render(gpu_ctx, {"textured_uber": pair_textured_uber, "textured_no_bsdf": pair_textured_no_bsdf}[pair](), variant, tag=pair)


def test_textured_no_bsdf_alternates(gpu_ctx):
    """The scene of the textured "no BSDF" pair does both: some hits scatter, others pass on (the render differs from all-scatter and all-pass)."""
    a, _ = pair_textured_no_bsdf()
    g = render_everything(gpu_ctx, room_scene(a))[0]
    s = (0.7, 0.6, 0.5)
    g1 = render_everything(gpu_ctx, room_scene(lambda b: b.material_translucent(Kd=Z3, Ks=s, reflect=O3, transmit=Z3, roughness=0.2)))[0]
    g0 = render_everything(gpu_ctx, room_scene(lambda b: b.material_translucent(Kd=Z3, Ks=s, reflect=Z3, transmit=Z3, roughness=0.2)))[0]
    assert not np.array_equal(g, g1) and not np.array_equal(g, g0)


def drawn_pair(k):
    rng = np.random.default_rng(1000 + k)
    col = lambda: tuple(float(x) for x in rng.uniform(0.1, 0.9, 3).astype(np.float32))
    rho, remap = float(f32(rng.uniform(0.02, 1.0))), bool(rng.integers(0, 2))
    if k % 2 == 0:
        return pair_uber(col(), col(), rho, remap)
    a, t = [(col(), Z3), (Z3, col()), (col(), col())][(k // 2) % 3]
    return pair_glass(col(), a, t, rho, remap)


@pytest.mark.parametrize("k", range(16))
def test_render_equals_equivalent_drawn(gpu_ctx, k):
    """Sixteen configurations drawn from a seed, inside the two equivalence families, roughness in [0.02, 1]."""
    assert_same_render(gpu_ctx, drawn_pair(k), "plain", res=16, tag="drawn %d" % k)


# ---------------------------------------------------------------- 4. whitted: the transmission lobe in BSDF::f
def whitted_scene(material, light_z):
    """A square in the plane z = 0 seen from z > 0 (it fills the view), a two-sided quad light at z = light_z."""
    b = scenes.SceneBuilder()
    b.look_at((0.0, -1.2, 2.5), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    b.camera_perspective(fov=15.0)
    b.film(xresolution=16, yresolution=16)
    b.pixel_filter_box()
    b.sampler_sobol(4)
    b.integrator_whitted(maxdepth=3)
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=(5.0, 4.0, 3.0), twosided=True)
    b.shape_trianglemesh([(-0.5, -0.5, light_z), (0.5, -0.5, light_z), (0.5, 0.5, light_z), (-0.5, 0.5, light_z)], [0, 1, 2, 0, 2, 3])
    b.no_area_light()
    material(b)
    b.shape_trianglemesh([(-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.5, 0.5, 0.0), (-0.5, 0.5, 0.0)], [0, 1, 2, 0, 2, 3])
    return b.build()


def test_whitted_sees_the_light_through_the_square(gpu_ctx):
    """Whitted's direct term has no MIS and no BSDF sample: f * Li * |cos| / pdf over the lights.  A translucent(Kd c, reflect 0, transmit 1)
    square lit from behind returns what a matte(Kd c) square lit from the front returns.  rtol 1e-4: the light is >= 1 unit away and every
    cosine >= 0.3, so float32 rounding stays near 1e-7 per operation; a missing lobe, the wrong side or a stray pi are errors of order 1."""
    c = (0.6, 0.5, 0.4)
    trans = lambda b: b.material_translucent(Kd=c, Ks=Z3, reflect=Z3, transmit=O3)
    front = render_everything(gpu_ctx, whitted_scene(lambda b: b.material_matte(c), 2.0))[0].astype(np.float64)
    assert (front > 0).all()                                             # every camera sample lands on the lit square
    behind = render_everything(gpu_ctx, whitted_scene(trans, -2.0))[0].astype(np.float64)
    rel = np.abs(behind - front) / front
    print("\nwhitted, translucent lit from behind against matte lit from the front: max relative difference %.3e" % rel.max())
    assert rel.max() <= 1e-4
    same_side = render_everything(gpu_ctx, whitted_scene(trans, 2.0))[0]
    assert (same_side == 0).all()


# ---------------------------------------------------------------- 5. path: the transmission lobe under MIS, with the quirk
def mis_moments(c, v3_pdf=False, nt=4000):
    """Mean and variance per channel of one estimate_direct (core/integrator/sampler.rs) at a translucent(Kd c, reflect 0, transmit 1) surface
    whose normal is the z axis, under a constant environment L = 1 with the identity transform.  theta is measured from the far side's axis.
    Light half: wi ~ lp, contributes f cos lp / (lp^2 + sp^2) on the far hemisphere, 0 on the near one.  BSDF half: wi ~ cos / pi on the far
    hemisphere, REPORTED as sp = cos (lambertian.rs:80-86; v3_pdf: cos / pi as pbrt-v3 has it), contributes f cos sp / (sp^2 + lp^2)."""
    from test_gpu_infinite_light import dist2d
    func, m_int = dist2d(np.ones((1, 1, 3), np.float32))
    assert np.allclose(func / m_int, 1.0)                                # a constant map: Distribution2D's pdf is 1 in every cell
    th = (np.arange(nt) + 0.5) / nt * (np.pi / 2)
    dw = 2 * np.pi * np.sin(th) * (np.pi / 2 / nt)                       # the integrands do not depend on phi
    cos = np.cos(th)
    lp = (func[0, 0] / m_int) / (2 * np.pi * np.pi * np.sin(th))         # infinite.rs pdf_li: map pdf / (2 pi^2 sin theta)
    sp = cos / np.pi if v3_pdf else cos
    c = np.asarray(c, np.float64)[:, None]
    A = c / np.pi * cos * lp / (lp * lp + sp * sp)
    B = c / np.pi * cos * sp / (sp * sp + lp * lp)
    ea, ea2 = (lp * A * dw).sum(1), (lp * A * A * dw).sum(1)
    eb, eb2 = (cos / np.pi * B * dw).sum(1), (cos / np.pi * B * B * dw).sum(1)
    mean = ea + eb
    var = (ea2 - ea * ea) + (eb2 - eb * eb)                               # the two halves draw from separate sample dimensions
    return mean, var


def test_path_mis_carries_the_pdf_without_inv_pi(gpu_ctx):
    c = (0.8, 0.6, 0.4)
    n = 64 * 64 * 16
    mean, var = mis_moments(c)
    bound = 5.0 * np.sqrt(var / n)              # five standard errors: a condition on the false-alarm rate (the Sobol' points do better)
    mean_v3, _ = mis_moments(c, v3_pdf=True)
    assert (np.abs(mean_v3 - mean) > bound).all(), "the test could not tell the quirk"
    b = scenes.SceneBuilder()
    b.look_at((0, 0, 1), (0, 0, 0), (0, 1, 0))
    b.camera_perspective(fov=20.0)
    b.film(xresolution=64, yresolution=64)
    b.pixel_filter_box()
    b.sampler_sobol(16)
    b.integrator_path(maxdepth=3)
    b.material_translucent(Kd=c, Ks=Z3, reflect=Z3, transmit=O3)
    b.shape_trianglemesh([-1000, -1000, 0, 1000, -1000, 0, 1000, 1000, 0, -1000, 1000, 0], [0, 1, 2, 0, 2, 3])
    b.light_infinite(L=(1.0, 1.0, 1.0))
    gpu_ctx.upload(b.build())
    g = gpu_ctx.radiance_samples((0, 0, 64, 64)).reshape(-1, 3).astype(np.float64)       # the film's own pixels (the sample bounds reach a pixel further)
    assert len(g) == n
    got = g.mean(0)
    print("\npath under MIS: mean %s, quadrature %s (with pbrt-v3's pdf %s), bound %s" % (got, mean, mean_v3, bound))
    assert (np.abs(got - mean) <= bound).all(), (got, mean, bound)


# ---------------------------------------------------------------- 6. command line
def test_cli_translucent_masked_leaf(tmp_path):
    (tmp_path / "s.pbrt").write_text("""LookAt 0 -3 2.5  0 0 0.4  0 0 1
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
Texture "holes" "float" "checkerboard" "float tex1" [1] "float tex2" [0] "float uscale" [6] "float vscale" [6] "string aamode" "none"
MakeNamedMaterial "leaf" "string type" "translucent" "rgb Kd" [0.3 0.7 0.2] "rgb Ks" [0.2 0.2 0.2] "rgb reflect" [0.4 0.4 0.4]
                  "rgb transmit" [0.6 0.6 0.6] "float roughness" [0.2]
NamedMaterial "leaf"
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 1 1 -1 1 1 1 1.4 -1 1 1.4] "float uv" [0 0 1 0 1 1 0 1] "texture alpha" "holes"
WorldEnd
""")
    ps = pkg.capi.ParsedScene(filename=str(tmp_path / "s.pbrt"))
    d = ps.desc
    assert [d.materials[i].type for i in range(d.n_materials)].count(pkg.capi.PT_MATERIAL_TRANSLUCENT) == 1 and len(ps.alpha_masks) == 1
    ctx = pkg.Context(0)
    try:
        ctx.upload(ps)
        ctx.film_clear(); ctx.render()
        want = ctx.film_rgb()
    finally:
        ctx.close()
    exe = os.path.join(ROOT, "pbrt-r3_amd", "csrc", "pbrt_gpu")
    out = tmp_path / "cli.pfm"
    r = subprocess.run([exe, "-i", str(tmp_path / "s.pbrt"), "--outfile", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer(out.read_bytes().split(b"\n", 3)[3], "<f4").reshape(32, 32, 3)[::-1]
    assert np.array_equal(bits(got), bits(want)) and want.max() > 0
    # and the transmission did something: the same leaf with "transmit" 0 renders differently
    text = (tmp_path / "s.pbrt").read_text()
    assert '"rgb transmit" [0.6 0.6 0.6]' in text
    ps2 = pkg.capi.ParsedScene(text=text.replace('"rgb transmit" [0.6 0.6 0.6]', '"rgb transmit" [0 0 0]'), work_dir=str(tmp_path))
    ctx = pkg.Context(0)
    try:
        ctx.upload(ps2)
        ctx.film_clear(); ctx.render()
        assert not np.array_equal(ctx.film_rgb(), want)
    finally:
        ctx.close()
