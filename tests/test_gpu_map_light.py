"""Goniometric and projection lights on the GPU path, held to the float64 restatement in tests/map_light_ref.py: the light hooks, the
closed-form radiance of a lit matte quad per camera sample in every integrator, shadows, light selection under the three strategies
beside a spot and an area light, every shading route, two maps in one scene, the CLI, and that a scene without these lights runs what it
ran before.

Every comparison uses the bound the restatement derives for that evaluation (f32 roundings counted to first order, plus the bilinear
lookup's sensitivity times the error of st).  A sample within its bound of a discontinuity -- the projection's image edge, its near
plane, theta's clamp, the quad's edge, a shadow edge -- is left out and counted; each test caps that share at 2 %.  The poses are those
tests/test_map_light_host.py holds to that cap on the CPU.  No scene here goes to the oracle: it does not know these lights."""
import os
import subprocess

import numpy as np
import pytest

import delta_light_ref as dref
import map_light_cases as cases
import map_light_ref as ref
from helpers import pkg, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = ref.EPS
f32 = np.float32
KD, FLOOR, P_ERR, NEAR_CAP, EXTENT = cases.KD, cases.FLOOR, cases.P_ERR, cases.NEAR_CAP, cases.EXTENT
base, floor, quad, plane_hit, light_terms = cases.base, cases.floor, cases.quad, cases.plane_hit, cases.light_terms
KINDS = ["goniometric", "projection", "projection_grazing"]


class Run:
    """One upload of a SceneBuilder's scene: the per-sample radiance (n, 3), the camera rays in float64, and the restated delta and map
    lights of the uploaded records in light-list order."""

    def __init__(self, ctx, sb, sd=None):
        self.sd = sb.build() if sd is None else sd
        self.info = ctx.upload(self.sd)
        b = list(self.info.sample_bounds)
        w, h, spp = b[2] - b[0], b[3] - b[1], self.info.spp
        ctx.reset_counters()
        self.rad = ctx.radiance_samples(tuple(b)).reshape(-1, 3).astype(np.float64)
        self.shadow_rays = ctx.counters()["shadow_rays"]
        self.kernel_set = ctx.kernel_set()
        ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
        pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
        o, d, _ = ctx.generate_camera_rays(pix, np.tile(np.arange(spp, dtype=np.uint32), w * h))
        self.o, self.d = o.astype(np.float64), d.astype(np.float64)
        wb = np.array(list(self.info.world_bound), np.float64)
        self.wb_min, self.wb_max = wb[:3], wb[3:]
        self.radius = 0.5 * np.sqrt(((self.wb_max - self.wb_min) ** 2).sum())
        self.lights = cases.restate_lights(sb, self.radius)


def check_closed_form(run, want, rel, skip, near=None):
    """run.rad against want (n, 3) within rel (n,) wherever skip is False; exact zeros where want is zero.  near: the samples left out for
    lying within their bound of a discontinuity (default: all of skip), at most NEAR_CAP of the film."""
    share = (skip if near is None else near).mean()
    assert share <= NEAR_CAP, share
    got, ok = run.rad, ~skip
    zero = ok & (want.sum(1) == 0)
    assert (got[zero] == 0).all(), np.abs(got[zero]).max()
    lit = ok & (want.sum(1) > 0)
    err = np.abs(got[lit] - want[lit]) / want[lit]
    bound = rel[lit][:, None]
    print("closed form: %d lit, %d black, %d left out; worst error / bound %.3f (bound at most %.2e)" % (
        lit.sum(), zero.sum(), skip.sum(), float((err / bound).max()) if lit.any() else 0.0, float(bound.max()) if lit.any() else 0.0))
    assert (err <= bound).all(), (float((err / bound).max()), int(lit.sum()))
    return int(lit.sum()), int(zero.sum())


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- 1. hooks
@pytest.mark.parametrize("pose", ["identity", "translated_rotated_scaled"])
def test_hooks_sample_li_and_pdf_li(ctx, pose):
    """pt_light_sample_li of a goniometric and a projection light at 600 points in front of, behind and around the light, under the
    identity and under a translated, rotated, non-uniformly scaled transform; pdf 1, pdf_li 0, le refused.  Under the translated transform
    the goniometric light's `scale` adds the translation to the direction (transform_point): the restatement with transform_vector in its
    place lies outside the bound at most points, so an implementation that took it would fail here."""
    ctm = None if pose == "identity" else cases.HOOK_CTM
    sb = base()
    floor(sb)
    sb.light_goniometric(L=(5, 7, 9), scale=(2, 1, 0.5), image=cases.MAP_8x4, ctm=ctm)
    sb.light_projection(I=(4, 5, 6), scale=(1, 2, 0.5), fov=70.0, image=cases.MAP_8x4, ctm=ctm)
    sd = sb.build()
    info = ctx.upload(sd)
    assert info.n_lights == 2 and ctx.kernel_set() == 3
    lights = cases.restate_lights(sb)
    l2w = np.array(list(sb.map_lights[0].light_to_world), np.float64).reshape(4, 4)
    p64 = cases.hook_points(l2w)
    p = p64.astype(f32)
    u = np.random.default_rng(3).random((len(p), 2)).astype(f32)
    for j, lt in enumerate(lights):
        li, wi, pdf = ctx.light_sample_li(j, p, u)
        s = ref.sample_li(lt, p64, 0.0)
        assert (pdf == 1.0).all()
        assert (np.abs(wi - s["wi"]) <= s["wi_err"][:, None]).all()
        ok = ~s["near"]
        assert s["near"].mean() <= NEAR_CAP, s["near"].mean()
        black = ok & (s["li"].sum(1) == 0)
        assert (li[black] == 0).all()
        lit = ok & ~black
        err = np.abs(li[lit] - s["li"][lit])
        print("hooks %s light %d: %d lit, %d black, %d near; worst error / bound %.3f" % (pose, j, lit.sum(), black.sum(), s["near"].sum(), (err / s["li_err"][lit]).max()))
        assert (err <= s["li_err"][lit]).all(), (j, float((err / s["li_err"][lit]).max()))
        if lt.kind == ref.PROJECTION:
            assert (np.bincount(s["region"][ok], minlength=3) > 60).all()
        else:
            assert lit.sum() > 550
            if pose != "identity":
                vec = ref.MapLight(ref.GONIOMETRIC, lt.spectrum, lt.v, lt.w2l * np.array([1.0, 1, 1, 0])[None, :] + np.diag([0.0, 0, 0, 1]), lt.levels)
                other = ref.sample_li(vec, p64, 0.0)["li"]
                assert (np.abs(other[lit] - s["li"][lit]) > 4 * s["li_err"][lit]).any(1).mean() > 0.8
        assert (ctx.light_pdf_li(j, wi) == 0).all()
        with pytest.raises(pkg.capi.PtError):
            ctx.light_le(j, wi)


# ---------------------------------------------------------------- 2. closed-form radiance
INTEGRATORS = [("path", 1), ("path", 5), ("all", 5), ("one", 5), ("whitted", 5)]


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("light", KINDS)
def test_lit_quad_is_the_closed_form_in_every_integrator(ctx, sampler, light):
    """A matte quad cannot see itself: every integrator returns Kd / pi Li(p) |cos| at the camera ray's hit point, 0 where the ray misses.
    The projector's image edge lies across the quad: lit and black samples are both on the film (and black-behind ones for the grazing pose)."""
    first = None
    for integ, depth in INTEGRATORS:
        sb = base(integ, sampler, maxdepth=depth)
        floor(sb)
        cases.LIGHTS[light](sb)
        run = Run(ctx, sb)
        assert run.kernel_set == 3
        p, hit, edge = plane_hit(run.o, run.d, 0.0, FLOOR, P_ERR)
        (c, rel, near, lit), = light_terms(run.lights, p)
        want = np.where(hit[:, None], c, 0.0)
        n_lit, n_zero = check_closed_form(run, want, rel, edge | (hit & near))
        assert (~hit).sum() > 50 and (run.rad[~hit & ~edge] == 0).all()
        region = ref.sample_li(run.lights[0], p[hit])["region"]
        if light == "goniometric":
            assert (region == 0).all() and n_lit > 400 and len(np.unique(want[hit], axis=0)) > 400
        elif light == "projection":
            assert (region == 0).sum() > 100 and (region == 1).sum() > 50
        else:
            assert (np.bincount(region, minlength=3) > 20).all(), np.bincount(region, minlength=3)
        # the shadow-ray counter: one ray per sample with non-black f Li, none for a sample outside the image, behind the light or off the quad
        expect = int((hit & lit & ~edge & ~near).sum())
        slack = int((edge | (hit & near)).sum())
        assert expect <= run.shadow_rays <= expect + slack, (integ, run.shadow_rays, expect, slack)
        if first is None:
            first = run.rad
        else:
            assert np.abs(run.rad - first).max() <= 16 * EPS * max(first.max(), 1e-30)            # and the integrators agree among themselves


# ---------------------------------------------------------------- 3. shadows
@pytest.mark.parametrize("integ", ["path", "all", "whitted"])
@pytest.mark.parametrize("light", ["goniometric", "projection"])
def test_occluder_between_and_behind(ctx, integ, light):
    """An occluder quad between the light and the floor blacks out exactly the samples whose float64 shadow segment crosses its interior; a
    quad behind (above) the light changes nothing: the segment ends at the light.  Shadow rays: one per floor vertex whose f Li is not
    black before the visibility test."""
    occ = (0.1, 0.9, -0.9, 0.4, 0.7)
    behind = (-1.5, 1.5, -1.5, 1.5, 3.5)
    sb = base(integ, res=24)
    floor(sb)
    sb.material_none()
    quad(sb, *occ)
    quad(sb, *behind)
    cases.LIGHTS[light](sb)
    run = Run(ctx, sb)
    p, hit, edge = plane_hit(run.o, run.d, 0.0, FLOOR, P_ERR)
    # camera rays that meet an occluder first do not shade the floor ("none" material: path and directlighting pass through, whitted returns 0)
    blocked, blocked_edge = np.zeros(len(p), bool), np.zeros(len(p), bool)
    for r in (occ, behind):
        _, h2, e2 = plane_hit(run.o, run.d, r[4], r[:4], P_ERR)
        blocked |= h2 | e2
        blocked_edge |= e2
    (c, rel, tnear, lit), = light_terms(run.lights, p, occluders=[occ, behind])
    (c_free, _, fnear, _), = light_terms(run.lights, p)
    near = edge | (hit & tnear)
    skip = near | blocked                        # (a camera ray that meets an occluder first is not a sample of the floor: left out, not "near")
    want = np.where(hit[:, None], c, 0.0)
    check_closed_form(run, want, rel + 2 * EPS, skip, near=near)
    shadowed = hit & ~skip & (c.sum(1) == 0) & (c_free.sum(1) > 0)
    assert shadowed.sum() > 30, shadowed.sum()                   # the occluder's shadow is on the film
    (above, _, _, _), = light_terms(run.lights, p, occluders=[behind])
    assert np.array_equal(above, c_free)                         # the quad above the light takes nothing
    # a camera ray that meets an occluder first goes on to the floor in `path` and `directlighting` (a surface without BSDF is passed through) and
    # ends in `whitted`; the re-spawned ray reaches the floor within 256 EPS EXTENT of the straight line
    p_err2 = 256 * EPS * EXTENT
    (_, _, wnear, _), = light_terms(run.lights, p, occluders=[occ, behind], p_err=p_err2)
    _, _, edge2 = plane_hit(run.o, run.d, 0.0, FLOOR, p_err2)
    unsure = edge | blocked_edge | (hit & tnear) | (blocked & (edge2 | (hit & wnear)))
    shades = hit & ~blocked if integ == "whitted" else hit
    expect = int((shades & lit & ~unsure).sum())
    slack = int(unsure.sum())
    occluded_lit = int((shades & ~unsure & lit & (c.sum(1) == 0)).sum())
    print("occluder %s %s: shadow rays %d, expected %d (+ at most %d unsure), of them occluded %d" % (light, integ, run.shadow_rays, expect, slack, occluded_lit))
    assert occluded_lit > 30
    assert expect <= run.shadow_rays <= expect + slack, (integ, run.shadow_rays, expect, slack)


# ---------------------------------------------------------------- 4. light selection
EMITTER = dict(P=[1.2, 1.0, 3.8, 1.7, 1.0, 3.8, 1.7, 1.5, 3.8, 1.2, 1.5, 3.8], idx=[0, 2, 1, 0, 3, 2], L=(150.0, 150.0, 150.0))          # faces down


def emitter_triangles():
    v = np.array(EMITTER["P"], np.float64).reshape(4, 3)
    i = np.array(EMITTER["idx"]).reshape(2, 3)
    return [v[t] for t in i]


def triangle_contrib(tri, po, u):
    """sum over the probes of Li.y / pdf for a one-sided emissive triangle (Triangle::sample + Shape::sample_from, diffuse.rs:63-96):
    uniform_sample_triangle, pdf = d^2 / (|cos| area), L where the light's face looks at the point."""
    p0, p1, p2 = tri
    su0 = np.sqrt(u[:, 0])
    b0, b1 = 1 - su0, u[:, 1] * su0
    q = b0[:, None] * p0 + b1[:, None] * p1 + (1 - b0 - b1)[:, None] * p2
    n = np.cross(p1 - p0, p2 - p0)
    area = 0.5 * np.linalg.norm(n)
    n = n / np.linalg.norm(n)
    w = q - po
    d2 = (w * w).sum(1)
    wi = w / np.sqrt(d2)[:, None]
    cos = -(wi @ n)
    pdf = d2 / (np.abs(cos) * area)
    ok = (cos > 0) & (pdf > 0) & np.isfinite(pdf)
    return float((np.where(ok, dref.luminance(np.array(EMITTER["L"])) / np.where(ok, pdf, 1.0), 0.0)).sum()), bool((np.abs(cos) < 1e-4).any())


def selection_pdfs(run, p, strategy):
    """pdf of each of the four lights (the emitter's two triangles, the map light, the spot) at floor points p under the restated
    distribution: (pdf (n, 4), relative bound (n, 4), near (n,))."""
    tris = emitter_triangles()
    nl = 2 + len(run.lights)
    if strategy == "power":
        y = [dref.luminance(np.array(EMITTER["L"]) * (0.5 * np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0])) * np.pi)) for t in tris]
        y += [dref.luminance(ref.power(lt) if isinstance(lt, ref.MapLight) else dref.power(lt)) for lt in run.lights]
        return np.tile(dref.distribution_pdf(y), (len(p), 1)), np.full((len(p), nl), 32 * EPS), np.zeros(len(p), bool)
    # "spatial", and "uniform" with more than one light (create_light_sample_distribution.rs:23-26)
    vox = dref.spatial_voxels(run.wb_min, run.wb_max)
    pi = dref.voxel_of(p, run.wb_min, run.wb_max, vox)
    ext = np.where(run.wb_max > run.wb_min, run.wb_max - run.wb_min, 1.0)
    fr = (p - run.wb_min) / ext * np.array(vox)
    face = np.round(fr)                      # a point within its error of a voxel face may be looked up in the neighbour
    near = ((np.abs(fr - face) * ext / np.array(vox) <= 4 * P_ERR) & (face > 0) & (face < np.array(vox))).any(1)
    pdf, rel = np.zeros((len(p), nl)), np.zeros((len(p), nl))
    cache = {}
    v = np.array(vox, np.float64)
    p_err = 4 * EPS * np.abs(np.stack([run.wb_min, run.wb_max])).max()
    for i, key in enumerate(map(tuple, pi)):
        if key not in cache:
            lo = run.wb_min + (np.array(key) / v) * (run.wb_max - run.wb_min)
            hi = run.wb_min + ((np.array(key) + 1) / v) * (run.wb_max - run.wb_min)
            po = lo + dref.PROBES[:, :3] * (hi - lo)
            contrib, crel, cnear = np.zeros(nl), np.zeros(nl), False
            for j, t in enumerate(tris):
                contrib[j], grazing = triangle_contrib(t, po, dref.PROBES[:, 3:5])
                crel[j] = 64 * EPS + 8 * p_err              # the sampled point, the distance, the cosine and the area: gamma(24) and the probe's own error over a distance > 1
                cnear = cnear or grazing
            for j, lt in enumerate(run.lights):
                s = cases.light_sample(lt, po, p_err)
                y = dref.luminance(s["li"])
                contrib[2 + j] = y.sum()
                cnear = cnear or bool(s["near"].any())
                crel[2 + j] = ((s["li_rel"] + 3 * EPS) * y).sum() / contrib[2 + j] + 128 * EPS if contrib[2 + j] > 0 else 0.0
            avg = contrib.sum() / (128 * nl)
            func = np.maximum(0.001 * avg if avg > 0 else 1.0, contrib)
            cache[key] = (dref.distribution_pdf(func), crel + crel.max() + (2 * nl + 4) * EPS, cnear)
        pdf[i], rel[i] = cache[key][0], cache[key][1]
        near[i] |= cache[key][2]
    return pdf, rel, near


def selection_scene(strategy):
    sb = base("path", res=16, spp=4, strategy=strategy, maxdepth=1)
    floor(sb)
    sb.material_none()
    sb.area_light_source_diffuse(L=EMITTER["L"])
    sb.shape_trianglemesh(EMITTER["P"], EMITTER["idx"], twosided=False)
    sb.no_area_light()
    cases.add_gonio(sb, image=(cases.MAP_4x2 * f32(0.4)).astype(f32))          # (a map whose mean is not 1: power() must read it)
    sb.light_spot(I=(20.0, 25.0, 30.0), coneangle=75.0, conedelta=20.0, frm=(-0.5, 0.3, 3.0), to=(0.0, 0.0, 0.0))          # covers the floor
    return sb


@pytest.mark.parametrize("strategy", ["uniform", "power", "spatial"])
def test_light_selection_follows_the_restated_distribution(ctx, strategy):
    """An emissive quad (two lights), a goniometric light and a spot; `path` with maxdepth 1 estimates one light per camera vertex.  A sample
    whose light was the goniometric light or the spot carries exactly c_j(p) / pdf_j, pdf_j from the restated distribution (the hit point's
    voxel for "spatial", the restated power() for "power"; "uniform" with four lights IS "spatial"); every other sample chose the emitter.
    Over the film each is chosen within five binomial standard deviations of its expected count."""
    sb = selection_scene(strategy)
    run = Run(ctx, sb)
    assert run.info.n_lights == 4 and run.kernel_set == 3
    p, hit, edge = plane_hit(run.o, run.d, 0.0, FLOOR, P_ERR)
    terms = light_terms(run.lights, p)
    pdf, pdf_rel, vnear = selection_pdfs(run, p, strategy)
    use = hit & ~edge & ~vnear & ~(terms[0][2] | terms[1][2])
    assert (hit & ~use).mean() <= NEAR_CAP, (hit & ~use).mean()
    assert (pdf[use] > 0).all() and np.allclose(pdf[use].sum(1), 1.0)
    matches = np.zeros((len(p), 2), bool)
    for j, (c, rel, _, _) in enumerate(terms):
        assert (c[use].sum(1) > 0).all()                   # both cover the floor: a black sample is never one of theirs
        want = c / pdf[:, 2 + j:3 + j]
        bound = (rel + pdf_rel[:, 2 + j] + 2 * EPS)[:, None] * want
        matches[:, j] = (np.abs(run.rad - want) <= bound).all(1)
    assert (matches[use].sum(1) <= 1).all()
    n = int(use.sum())
    chosen = [int((~matches[use].any(1)).sum()), int(matches[use, 0].sum()), int(matches[use, 1].sum())]
    prob = [pdf[use, 0] + pdf[use, 1], pdf[use, 2], pdf[use, 3]]
    for name, got, pr in zip(("emitter", "goniometric", "spot"), chosen, prob):
        expect, var = pr.sum(), (pr * (1 - pr)).sum()
        print("selection %s: %s chosen %d times of %d, expected %.2f, standard deviation %.3f" % (strategy, name, got, n, expect, np.sqrt(var)))
        assert abs(got - expect) <= 5 * np.sqrt(var) + 1e-9, (strategy, name, got, expect, n)
    assert chosen[1] > 20
    if strategy == "power":                                # the restated power() decides: the table holds the map's lookup((.5, .5), .5)
        assert len(np.unique(np.round(pdf[use], 12), axis=0)) == 1
        flat = ref.MapLight(ref.GONIOMETRIC, run.lights[0].spectrum, run.lights[0].v, run.lights[0].w2l, ref.pyramid(np.ones((1, 1, 3))))
        assert abs(dref.luminance(ref.power(flat)) / dref.luminance(ref.power(run.lights[0])) - 1) > 0.1
    if strategy == "uniform":
        spatial = Run(ctx, selection_scene("spatial"))
        assert np.array_equal(spatial.rad, run.rad)


# ---------------------------------------------------------------- 5. every shading route
FAR = scenes.transform_translate(6.0, 3.5, 0.3)             # 40 degrees off the view axis: outside the film's 33-degree corners, clear of every shadow segment
KD2, AMOUNT = (0.2, 0.7, 0.3), 0.25


def route_plain(sb):
    floor(sb)


def route_texture(sb):
    img = np.tile(np.array(KD, np.float32), (4, 4, 1))
    sb.material_matte(sb.texture_imagemap(sb.image_pyramid(img)))
    quad(sb, FLOOR[0], FLOOR[1], FLOOR[2], FLOOR[3], 0.0, uv=True)


def route_instance(sb):
    floor(sb)
    sb.object_begin("o")
    quad(sb, -0.1, 0.1, -0.1, 0.1, 0.0)
    sb.object_end()
    sb.object_instance("o", to_world=FAR)


def route_sphere(sb):
    floor(sb)
    sb.shape_sphere(radius=0.25, object_to_world=FAR[0], world_to_object=FAR[1])


def route_quadric(sb):
    floor(sb)
    sb.shape_cylinder(radius=0.2, zmin=-0.1, zmax=0.1, object_to_world=FAR[0], world_to_object=FAR[1])
    sb.shape_disk(height=0.1, radius=0.2, object_to_world=FAR[0], world_to_object=FAR[1])


def route_mix(sb):
    sb.material_matte(KD)
    a = sb.cur_material
    sb.material_matte(KD2)
    b = sb.cur_material
    sb.material_mix(a, b, amount=AMOUNT)
    quad(sb, FLOOR[0], FLOOR[1], FLOOR[2], FLOOR[3], 0.0)


def route_disney(sb):
    floor(sb)
    sb.material_disney(color=(0.7, 0.3, 0.2), roughness=0.4, metallic=0.3)
    sb.shape_trianglemesh([5.9, 3.4, 0.3, 6.1, 3.4, 0.3, 6.1, 3.6, 0.3, 5.9, 3.6, 0.3], [0, 1, 2, 0, 2, 3])


ROUTES = [route_plain, route_texture, route_instance, route_sphere, route_quadric, route_mix, route_disney]


@pytest.mark.parametrize("route", ROUTES, ids=[r.__name__[6:] for r in ROUTES])
@pytest.mark.parametrize("integ", ["path", "all"])
def test_every_shading_route_gives_the_closed_form(ctx, route, integ):
    """The lit quad through the plain kernels, k_tex_resolve + the _res kernel (a Kd image map of one colour), the instanced kernel, the
    sphere family, the analytic shapes by kind, the scaled lobe list of a Material "mix" (two mattes: amount Kd1 / pi + (1 - amount) Kd2 / pi)
    and a scene that holds a Material "disney" -- with a projection light, whose image edge crosses the quad, and for `all` a goniometric
    light beside it.  The unlit extra shapes are out of view and out of every shadow segment's way."""
    sb = base(integ)
    route(sb)
    cases.add_proj(sb)
    if integ != "path":                          # `path` estimates one light per vertex (test 4 holds its selection); here it gets one light alone
        cases.add_gonio(sb)
    run = Run(ctx, sb)
    assert run.kernel_set == 3
    p, hit, edge = plane_hit(run.o, run.d, 0.0, FLOOR, P_ERR)
    brdf, extra = None, 0.0
    if route is route_texture:
        extra = 12 * EPS                   # the filtered lookup of a constant image: a weighted mean of equal texels, divided by the weights' sum
    if route is route_mix:
        kd = AMOUNT * np.array(KD) + (1 - AMOUNT) * np.array(KD2)
        extra = 8 * EPS                    # two scales, two lobes' f summed

        def brdf(wi, kd=kd):
            return np.tile(kd / np.pi, (len(wi), 1))
    terms = light_terms(run.lights, p, brdf=brdf)
    want = np.where(hit[:, None], sum(t[0] for t in terms), 0.0)
    rel = np.max([t[1] for t in terms], 0) + extra + 2 * EPS
    n_lit, n_zero = check_closed_form(run, want, rel, edge | (hit & np.any([t[2] for t in terms], 0)))
    assert n_lit > (300 if integ != "path" else 100)
    if integ == "path":
        assert ((want.sum(1) == 0) & hit).sum() > 50           # black outside the projector's image, on the quad


# ---------------------------------------------------------------- 6. two map lights, two images
@pytest.mark.parametrize("integ", ["all", "whitted"])
def test_two_map_lights_pick_their_own_images(ctx, integ):
    """A goniometric light on the 4 x 2 map and a projection light on the 8 x 4 map (and a third image in the table that neither uses):
    the sum of the two closed forms; with the images swapped in the restatement the film is out of bounds."""
    sb = base(integ)
    floor(sb)
    cases.add_gonio(sb, image=cases.MAP_4x2)
    sb.image_pyramid(np.full((2, 2, 3), 9.0, f32))
    cases.add_proj(sb, image=cases.MAP_8x4)
    run = Run(ctx, sb)
    assert sb.map_lights[0].image != sb.map_lights[1].image
    p, hit, edge = plane_hit(run.o, run.d, 0.0, FLOOR, P_ERR)
    terms = light_terms(run.lights, p)
    want = np.where(hit[:, None], terms[0][0] + terms[1][0], 0.0)
    rel = np.maximum(terms[0][1], terms[1][1]) + 2 * EPS
    skip = edge | (hit & (terms[0][2] | terms[1][2]))
    check_closed_form(run, want, rel, skip)
    g, pr = run.lights
    swapped = [ref.MapLight(g.kind, g.spectrum, g.v, g.w2l, pr.levels),
               ref.MapLight(pr.kind, pr.spectrum, pr.v, pr.w2l, g.levels, pr.proj, pr.screen, pr.cos_total, pr.proj_rel)]
    other = light_terms(swapped, p)
    wrong = np.where(hit[:, None], other[0][0] + other[1][0], 0.0)
    ok = hit & ~skip
    assert (np.abs(run.rad[ok] - wrong[ok]) > 8 * rel[ok][:, None] * want[ok]).any(1).mean() > 0.9


# ---------------------------------------------------------------- 7. CLI
def write_pfm(path, rgb_top_first):
    a = np.asarray(rgb_top_first, np.float32)
    h, w, _ = a.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(a[::-1]).astype("<f4").tobytes())


def test_cli_renders_the_scene_builder_film(ctx, tmp_path):
    """pbrt_gpu -i on .pbrt text with the three directives and a PFM map gives the film of the same scene built with SceneBuilder, bit for
    bit.  The CTMs are Translate * Scale (Scale 1 1 -1 turns the projector to look down)."""
    T = scenes
    sb = base("path", res=16, spp=4)
    floor(sb)
    sb.light_goniometric(L=(30, 20, 10), scale=(0.5, 1, 1.5), image=cases.MAP_4x2, ctm=T.transform_mul(T.transform_translate(0.3, -0.2, 1.5), T.transform_scale(3, 2, 4)))
    sb.light_projection(I=(40, 30, 20), scale=(1, 0.5, 2), fov=50, image=cases.MAP_4x2, ctm=T.transform_mul(T.transform_translate(0.2, -0.3, 2.5), T.transform_scale(1, 1, -1)))
    sb.light_point(I=(3, 2, 1), frm=(-1.0, 0.5, 1.0), ctm=T.transform_scale(2, 2, 2))
    ctx.upload(sb.build())
    ctx.film_clear()
    ctx.render()
    want = ctx.film_rgb()
    write_pfm(str(tmp_path / "map.pfm"), cases.MAP_4x2)
    text = '''LookAt 0 -4 3  0 0 0  0 0 1
Camera "perspective" "float fov" 50
Film "image" "integer xresolution" 16 "integer yresolution" 16 "string filename" "map.pfm"
PixelFilter "box"
Sampler "sobol" "integer pixelsamples" 4
Integrator "path" "integer maxdepth" 5
WorldBegin
Material "matte" "rgb Kd" [0.6 0.5 0.4]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -2 0 2 -2 0 2 2 0 -2 2 0]
AttributeBegin
Translate 0.3 -0.2 1.5
Scale 3 2 4
LightSource "goniometric" "rgb L" [30 20 10] "rgb scale" [0.5 1 1.5] "string mapname" "map.pfm"
AttributeEnd
AttributeBegin
Translate 0.2 -0.3 2.5
Scale 1 1 -1
LightSource "projection" "rgb I" [40 30 20] "rgb scale" [1 0.5 2] "float fov" 50 "string mapname" "map.pfm"
AttributeEnd
AttributeBegin
Scale 2 2 2
LightSource "point" "rgb I" [3 2 1] "point from" [-1 0.5 1]
AttributeEnd
WorldEnd
'''
    scene = tmp_path / "maplight.pbrt"
    scene.write_text(text)
    exe = os.path.join(ROOT, "pbrt-r3_amd", "csrc", "pbrt_gpu")
    out = tmp_path / "out.pfm"
    r = subprocess.run([exe, "-i", str(scene), "--outfile", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    head = raw.split(b"\n", 3)
    assert head[0] == b"PF" and head[1].split() == [b"16", b"16"]
    img = np.frombuffer(head[3], "<f4" if float(head[2]) < 0 else ">f4").reshape(16, 16, 3)[::-1]
    assert want.sum() > 0 and np.array_equal(img.astype(f32).view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------- 8. a scene without these lights runs what it ran
def test_a_spot_and_distant_scene_is_untouched_by_the_setter(ctx):
    """pt_scene_set_map_lights(ctx, 0, NULL) before the upload of a spot + distant scene: the same film bit for bit, the same shadow rays,
    and the scene runs the first build of the kernels (the unmangled k_* symbols it ran before this light existed), not the one that
    knows the image lookup; a bad record is refused by the upload with a message that names the light, and the records do not outlive it."""
    def scene():
        sb = base("path")
        floor(sb)
        sb.light_spot(I=(30.0, 20.0, 10.0), coneangle=25.0, conedelta=8.0, frm=(0.3, -0.2, 2.5), to=(0.1, 0.2, 0.0))
        sb.light_distant(L=(1.5, 2.0, 2.5), frm=(0.4, -1.0, 1.2), to=(0.0, 0.0, 0.0))
        return sb
    plain = Run(ctx, scene())
    lib = ctx.lib
    lib.pt_scene_set_map_lights.argtypes = [pkg.capi.C.c_void_p, pkg.capi.C.c_uint32, pkg.capi.C.POINTER(pkg.capi.pt_map_light)]
    assert lib.pt_scene_set_map_lights(ctx.h, 0, None) == 0
    again = Run(ctx, scene())
    assert plain.kernel_set == again.kernel_set == 0
    assert plain.rad.sum() > 0 and np.array_equal(plain.rad.astype(f32).view(np.uint32), again.rad.astype(f32).view(np.uint32))
    assert plain.shadow_rays == again.shadow_rays
    # refusals of the upload (PT_ERR_INVALID_ARGUMENT = 1), each consumed by the upload that refuses it
    sb = base("path")
    floor(sb)
    cases.add_proj(sb)
    good = sb.map_lights[0]
    for field, value, word in (("kind", 7, "kind"), ("image", 5, "image"), ("resolution", (0, 2), "resolution"), ("light_to_world", None, "projective")):
        bad = pkg.capi.pt_map_light.from_buffer_copy(good)
        if field == "resolution":
            bad.resolution[:] = list(value)
        elif field == "light_to_world":
            bad.light_to_world[12] = 0.5
        else:
            setattr(bad, field, value)
        sd = sb.build()
        sd.map_lights = [bad]
        with pytest.raises(pkg.capi.PtError) as e:
            ctx.upload(sd)
        assert e.value.status == 1 and word in str(e.value), str(e.value)
    mono = base("path")
    floor(mono)
    cases.add_proj(mono)
    sd = mono.build()
    one = pkg.capi.pt_map_light.from_buffer_copy(mono.map_lights[0])
    one.image = mono.image_pyramid(np.ones((2, 2), f32))                  # a one-channel image
    sd = mono.build()
    sd.map_lights = [one]
    with pytest.raises(pkg.capi.PtError) as e:
        ctx.upload(sd)
    assert e.value.status == 1 and "3 channels" in str(e.value)
    last = Run(ctx, scene())                                              # the refused records are gone
    assert last.kernel_set == 0 and np.array_equal(last.rad, plain.rad)
