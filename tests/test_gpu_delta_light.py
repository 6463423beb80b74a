"""Delta lights (spot, distant, point) on the GPU path, held to the float64 restatement in tests/delta_light_ref.py: the light hooks, the
closed-form radiance of a lit matte quad per camera sample in every integrator, shadows and the far end of the shadow ray, light selection
under the three strategies (dense and lazy grid), delta lights beside an area light, every shading route, and the CLI.

Every comparison uses the bound the restatement derives for that evaluation (f32 roundings counted, first order).  A sample within its
bound of a discontinuity -- cos(theta) against a cone cosine, the quad's edge, a shadow edge -- is left out and counted; each test caps
that share at 2 %.  No scene here goes to the oracle: it does not know these lights yet."""
import os
import subprocess

import numpy as np
import pytest

import delta_light_ref as ref
from helpers import pkg, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = ref.EPS
f32 = np.float32
KD = (0.6, 0.5, 0.4)
FLOOR = (-2.0, 2.0, -2.0, 2.0)                  # x0 x1 y0 y1 at z = 0
EXTENT = 4.0                                    # coordinates of everything a test looks at stay below this
P_ERR = 16 * EPS * EXTENT                       # a hit point rebuilt from barycentrics in f32: at most 7 roundings on terms below EXTENT, doubled
NEAR_CAP = 0.02
SPOT = dict(frm=(0.3, -0.2, 2.5), to=(0.1, 0.2, 0.0), I=(30.0, 20.0, 10.0), coneangle=25.0, conedelta=8.0)
DIST = dict(frm=(0.4, -1.0, 1.2), to=(0.0, 0.0, 0.0), L=(1.5, 2.0, 2.5))


def base(integrator="path", sampler="sobol", res=16, spp=4, **kw):
    sb = scenes.SceneBuilder()
    sb.look_at((0, -4, 3), (0, 0, 0), (0, 0, 1))
    sb.camera_perspective(fov=50.0)
    sb.film(xresolution=res, yresolution=res)
    sb.pixel_filter_box()
    (sb.sampler_halton if sampler == "halton" else sb.sampler_sobol)(pixelsamples=spp)
    if integrator == "path":
        sb.integrator_path(maxdepth=kw.get("maxdepth", 5), lightsamplestrategy=kw.get("strategy", "spatial"))
    elif integrator == "whitted":
        sb.integrator_whitted(maxdepth=kw.get("maxdepth", 5))
    else:
        sb.integrator_directlighting(maxdepth=kw.get("maxdepth", 5), strategy=integrator)          # "all" / "one"
    return sb


def quad(sb, x0, x1, y0, y1, z, uv=False):
    sb.shape_trianglemesh([x0, y0, z, x1, y0, z, x1, y1, z, x0, y1, z], [0, 1, 2, 0, 2, 3], uv=[0, 0, 1, 0, 1, 1, 0, 1] if uv else None)


def floor(sb, **kw):
    sb.material_matte(KD, **kw)
    quad(sb, FLOOR[0], FLOOR[1], FLOOR[2], FLOOR[3], 0.0)


def add_spot(sb, **over):
    s = dict(SPOT, **over)
    sb.light_spot(I=s["I"], coneangle=s["coneangle"], conedelta=s["conedelta"], frm=s["frm"], to=s["to"])


def add_distant(sb, **over):
    s = dict(DIST, **over)
    sb.light_distant(L=s["L"], frm=s["frm"], to=s["to"])


class Run:
    """One upload: the per-sample radiance (n, 3), the camera rays in float64, and the restated lights of the uploaded records."""

    def __init__(self, ctx, sd):
        self.info = ctx.upload(sd)
        b = list(self.info.sample_bounds)
        w, h, spp = b[2] - b[0], b[3] - b[1], self.info.spp
        ctx.reset_counters()
        self.rad = ctx.radiance_samples(tuple(b)).reshape(-1, 3).astype(np.float64)
        self.shadow_rays = ctx.counters()["shadow_rays"]
        ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
        pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
        o, d, _ = ctx.generate_camera_rays(pix, np.tile(np.arange(spp, dtype=np.uint32), w * h))
        self.o, self.d = o.astype(np.float64), d.astype(np.float64)
        wb = np.array(list(self.info.world_bound), np.float64)
        self.wb_min, self.wb_max = wb[:3], wb[3:]
        self.radius = 0.5 * np.sqrt(((self.wb_max - self.wb_min) ** 2).sum())
        self.lights = [ref.from_record(dl, self.radius) for dl in sd.delta_lights]


def plane_hit(o, d, z, rect, p_err):
    """Where rays o + t d meet the rectangle rect = (x0 x1 y0 y1) of the plane at height z: (p, hit, near the rectangle's edge)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (z - o[:, 2]) / d[:, 2]
    p = o + t[:, None] * d
    p[:, 2] = z
    ok = np.isfinite(t) & (t > 0)
    ex = np.minimum(np.minimum(p[:, 0] - rect[0], rect[1] - p[:, 0]), np.minimum(p[:, 1] - rect[2], rect[3] - p[:, 1]))
    return p, ok & (ex > 0), ok & (np.abs(ex) <= p_err)


def delta_terms(run, p, occluders=(), p_err=P_ERR, brdf=None):
    """Per light: (c (n, 3) = f Li |cos| at floor points p with the shadow applied, relative bound (n,), near (n,), lit (n,) bool =
    non-black f Li before the shadow test).  occluders: rectangles (x0 x1 y0 y1 z) in horizontal planes."""
    out = []
    for lt in run.lights:
        s = ref.sample_li(lt, p, p_err)
        cos = s["wi"][:, 2]
        f = np.tile(np.array(KD) / np.pi, (len(p), 1)) if brdf is None else brdf(s["wi"])
        c = f * s["li"] * np.abs(cos)[:, None]
        # Kd * INV_PI (2 roundings), |wi . n| (5, on a wi known to wi_err per component), f cos, f Li, then beta * (Ld / pdf) and L += (4)
        rel = s["li_rel"] + 3 * s["wi_err"] / np.maximum(np.abs(cos), 1e-30) + 14 * EPS
        near = s["near"].copy()
        lit = (s["li"].sum(1) > 0) & (np.abs(cos) > 0)
        for (x0, x1, y0, y1, z) in occluders:
            tgt = s["target"]
            with np.errstate(divide="ignore", invalid="ignore"):
                u = (z - p[:, 2]) / (tgt[:, 2] - p[:, 2])
            q = p + u[:, None] * (tgt - p)
            crosses = np.isfinite(u) & (u > 0) & (u < 1)
            ex = np.minimum(np.minimum(q[:, 0] - x0, x1 - q[:, 0]), np.minimum(q[:, 1] - y0, y1 - q[:, 1]))
            # the f32 shadow segment starts at the error-offset point and ends at the f32 light: its crossing moves by a few p_err
            margin = 8 * p_err + 64 * EPS * EXTENT
            near |= crosses & (np.abs(ex) <= margin)
            near |= np.isfinite(u) & (np.abs(u - 1) <= 1e-3) & (ex > -margin)          # an occluder at the segment's very end (PT_SHADOW_EPS)
            c = np.where((crosses & (ex > 0))[:, None], 0.0, c)
        out.append((c, rel, near, lit))
    return out


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
    assert (err <= bound).all(), (float((err / bound).max()), int(lit.sum()))
    return int(lit.sum()), int(zero.sum())


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- 1. hooks
def test_hooks_sample_li_and_pdf_li(ctx):
    """pt_light_sample_li of a spot, a distant and a point light under a rotated, non-uniformly scaled CTM at 600 points spread over the
    full-intensity cone, the falloff band, outside the cone and behind the light; pdf 1, pdf_li 0, le refused."""
    T = scenes
    ctm = T.transform_mul(T.transform_translate(0.5, -0.25, 0.75), T.transform_mul(T.transform_rotate_x(25.0), T.transform_scale(1.5, 0.75, 2.0)))
    sb = base()
    floor(sb)
    sb.light_spot(I=(5, 7, 9), scale=(2, 1, 0.5), coneangle=35, conedelta=12, frm=(0.2, 0.1, 1.0), to=(0.3, -0.2, -1.0), ctm=ctm)
    sb.light_distant(L=(1, 2, 3), frm=(0.3, 0.2, 1.0), to=(0, 0, 0), ctm=ctm)
    sb.light_point(I=(4, 5, 6), frm=(0.5, 0.5, 1.5), ctm=ctm)
    sd = sb.build()
    info = ctx.upload(sd)
    assert info.n_lights == 3
    wb = np.array(list(info.world_bound), np.float64)
    radius = 0.5 * np.sqrt(((wb[3:] - wb[:3]) ** 2).sum())
    lights = [ref.from_record(dl, radius) for dl in sd.delta_lights]
    rng = np.random.default_rng(11)
    axis = ref.normalize(np.linalg.inv(lights[0].w2l) @ np.array([0.0, 0.0, 1.0]))        # the cone's world axis is not w2l's row under scaling:
    p = np.concatenate([lights[0].v + rng.uniform(0.5, 3.0, (300, 1)) * ref.normalize(axis + rng.normal(0, 0.45, (300, 3))),   # around the cone
                        lights[0].v - rng.uniform(0.5, 3.0, (100, 1)) * ref.normalize(axis + rng.normal(0, 0.45, (100, 3))),   # behind the light
                        rng.uniform(-3, 3, (200, 3))]).astype(np.float32)
    u = rng.random((len(p), 2)).astype(np.float32)
    p64 = p.astype(np.float64)
    bands = None
    for j, lt in enumerate(lights):
        li, wi, pdf = ctx.light_sample_li(j, p, u)
        s = ref.sample_li(lt, p64, 0.0)
        assert (pdf == 1.0).all()
        assert (np.abs(wi - s["wi"]) <= s["wi_err"][:, None]).all()
        ok = ~s["near"]
        assert s["near"].mean() <= NEAR_CAP
        black = ok & (s["li"].sum(1) == 0)
        assert (li[black] == 0).all()
        lit = ok & ~black
        err = np.abs(li[lit] - s["li"][lit]) / s["li"][lit]
        assert (err <= s["li_rel"][lit][:, None]).all(), (j, float((err / s["li_rel"][lit][:, None]).max()))
        if lt.kind == ref.SPOT:
            f = s["falloff"]
            bands = ((f == 1).sum(), ((f > 0) & (f < 1)).sum(), (f == 0).sum())
        assert (ctx.light_pdf_li(j, wi) == 0).all()
        with pytest.raises(pkg.capi.PtError):
            ctx.light_le(j, wi)
    assert min(bands) >= 30, bands


# ---------------------------------------------------------------- 2. closed-form radiance
INTEGRATORS = [("path", 1), ("path", 5), ("all", 5), ("one", 5), ("whitted", 5)]


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("light", ["spot", "distant"])
def test_lit_quad_is_the_closed_form_in_every_integrator(ctx, sampler, light):
    """A matte quad cannot see itself: every integrator returns Kd / pi Li(p) |cos| at the camera ray's hit point, 0 where the ray misses."""
    first = None
    for integ, depth in INTEGRATORS:
        sb = base(integ, sampler, maxdepth=depth)
        floor(sb)
        (add_spot if light == "spot" else add_distant)(sb)
        run = Run(ctx, sb.build())
        p, hit, edge = plane_hit(run.o, run.d, 0.0, FLOOR, P_ERR)
        (c, rel, near, lit), = delta_terms(run, p)
        want = np.where(hit[:, None], c, 0.0)
        n_lit, n_zero = check_closed_form(run, want, rel, edge | (hit & near))
        assert (~hit).sum() > 50 and (run.rad[~hit & ~edge] == 0).all()
        if light == "spot":
            f = ref.sample_li(run.lights[0], p[hit])["falloff"]
            assert (f == 1).sum() > 20 and ((f > 0) & (f < 1)).sum() > 20 and (f == 0).sum() > 100          # all three bands on the floor
        else:
            assert len(np.unique(want[hit], axis=0)) == 1 and len(np.unique(run.rad[hit & ~edge], axis=0)) == 1      # one constant
        # the shadow-ray counter: one ray per sample with non-black f Li, none for a sample outside the cone or off the quad
        expect = int((hit & lit & ~edge & ~near).sum())
        slack = int((edge | (hit & near)).sum())
        assert expect <= run.shadow_rays <= expect + slack, (integ, run.shadow_rays, expect, slack)
        if first is None:
            first = run.rad
        else:
            assert np.abs(run.rad - first).max() <= 16 * EPS * max(first.max(), 1e-30)            # and the integrators agree among themselves


# ---------------------------------------------------------------- 3. shadows and the ray's far end
@pytest.mark.parametrize("integ", ["path", "all", "whitted"])
def test_occluder_between_and_behind(ctx, integ):
    """An occluder quad between the spot and the floor blacks out exactly the samples whose float64 shadow segment crosses its interior; a quad
    behind (above) the light changes nothing: the segment ends at the light.  The occluders are out of the camera's sight lines to the floor."""
    occ = (0.1, 0.9, -0.9, 0.4, 1.2)
    behind = (-1.5, 1.5, -1.5, 1.5, 3.5)
    sb = base(integ, res=24)
    floor(sb)
    sb.material_none()
    quad(sb, *occ)
    quad(sb, *behind)
    add_spot(sb, coneangle=40.0)
    if integ != "path":                          # `path` estimates ONE light per vertex: it gets the spot alone (selection pdf 1)
        add_distant(sb)
    run = Run(ctx, sb.build())
    p, hit, edge = plane_hit(run.o, run.d, 0.0, FLOOR, P_ERR)
    # camera rays that meet an occluder first do not shade the floor ("none" material: path and directlighting pass through, whitted returns 0)
    blocked, blocked_edge = np.zeros(len(p), bool), np.zeros(len(p), bool)
    for r in (occ, behind):
        _, h2, e2 = plane_hit(run.o, run.d, r[4], r[:4], P_ERR)
        blocked |= h2 | e2
        blocked_edge |= e2
    terms = delta_terms(run, p, occluders=[occ, behind])
    free = delta_terms(run, p)
    want = sum(t[0] for t in terms)
    rel = np.max([t[1] for t in terms], 0) + 2 * EPS
    near = edge | (hit & np.any([t[2] for t in terms], 0))
    skip = near | blocked                        # (a camera ray that meets an occluder first is not a sample of the floor: left out, not "near")
    want = np.where(hit[:, None], want, 0.0)
    n_lit, n_zero = check_closed_form(run, want, rel, skip, near=near)
    shadowed = hit & ~skip & (terms[0][0].sum(1) == 0) & (free[0][0].sum(1) > 0)
    assert shadowed.sum() > 30                                   # the occluder's shadow of the spot is on the film
    # the spot's segment ends at the light: the quad above it takes nothing from the spot's term, wherever the extended segment would cross it
    above = delta_terms(run, p, occluders=[behind])[0][0]
    assert np.array_equal(above, free[0][0])
    # the shadow-ray counter: one ray per light and floor vertex whose f Li is not black BEFORE the visibility test -- an occluded sample
    # counts, a sample outside the cone or off the floor does not.  A camera ray that meets an occluder first goes on to the floor in `path`
    # and `directlighting` (a surface without BSDF is passed through: path.rs:100-104, directlighting.rs:113-116) and ends in `whitted`; the
    # re-spawned ray reaches the floor within 256 EPS EXTENT of the straight line, so those samples' discontinuities get that margin.
    p_err2 = 256 * EPS * EXTENT
    wide = delta_terms(run, p, occluders=[occ, behind], p_err=p_err2)
    _, _, edge2 = plane_hit(run.o, run.d, 0.0, FLOOR, p_err2)
    unsure = edge | blocked_edge | (hit & np.any([t[2] for t in terms], 0)) | (blocked & (edge2 | (hit & np.any([t[2] for t in wide], 0))))
    shades = hit & ~blocked if integ == "whitted" else hit
    expect = sum(int((shades & t[3] & ~unsure).sum()) for t in free)
    slack = len(free) * int(unsure.sum())
    occluded_lit = sum(int((shades & ~unsure & t[3] & (o[0].sum(1) == 0)).sum()) for t, o in zip(free, terms))
    dark = sum(int((shades & ~unsure & ~t[3]).sum()) for t in free)
    print("occluder %s: shadow rays %d, expected %d (+ at most %d unsure), of them occluded %d; floor vertices with black f Li %d" % (
        integ, run.shadow_rays, expect, slack, occluded_lit, dark))
    assert occluded_lit > 30 and dark > 0
    assert expect <= run.shadow_rays <= expect + slack, (integ, run.shadow_rays, expect, slack)
    if integ == "path":
        return
    # the quad above the spot shadows the DISTANT light only: where the spot's segment would cross it had it not ended at the light, the spot's term is whole
    beyond = hit & ~skip & (free[0][0].sum(1) > 0) & (terms[0][0].sum(1) > 0) & (terms[1][0].sum(1) == 0) & (free[1][0].sum(1) > 0)
    assert beyond.sum() > 30


# ---------------------------------------------------------------- 4. light selection
def selection_pdfs(run, p, strategy):
    """pdf of each light at floor points p under the restated distribution: (pdf (n, n_lights), relative bound (n, n_lights), near (n,))."""
    nl = len(run.lights)
    if strategy == "power":
        y = np.array([ref.luminance(ref.power(lt)) for lt in run.lights])
        return np.tile(ref.distribution_pdf(y), (len(p), 1)), np.full((len(p), nl), 16 * EPS), np.zeros(len(p), bool)
    # "spatial", and "uniform" with more than one light (create_light_sample_distribution.rs:23-26)
    vox = ref.spatial_voxels(run.wb_min, run.wb_max)
    pi = ref.voxel_of(p, run.wb_min, run.wb_max, vox)
    # a point within its error of a voxel face may be looked up in the neighbour
    ext = np.where(run.wb_max > run.wb_min, run.wb_max - run.wb_min, 1.0)
    fr = (p - run.wb_min) / ext * np.array(vox)
    face = np.round(fr)                      # (faces 0 and `vox` are the grid's outside: the lookup clamps there, no neighbour to fall into)
    near = ((np.abs(fr - face) * ext / np.array(vox) <= 4 * P_ERR) & (face > 0) & (face < np.array(vox))).any(1)
    pdf, rel = np.zeros((len(p), nl)), np.zeros((len(p), nl))
    cache = {}
    for i, key in enumerate(map(tuple, pi)):
        if key not in cache:
            cache[key] = ref.compute_distribution(run.lights, key, run.wb_min, run.wb_max, vox)
        pdf[i], rel[i] = cache[key][0], cache[key][1]
        near[i] |= cache[key][2]
    return pdf, rel, near


def selection_scene(strategy):
    sb = base("path", res=16, spp=4, strategy=strategy)
    floor(sb)
    add_spot(sb, coneangle=75.0, conedelta=20.0, frm=(-0.5, 0.3, 3.0), to=(0.0, 0.0, 0.0), I=(20.0, 25.0, 30.0))          # covers the floor
    add_spot(sb)                                                                                                  # covers its middle
    add_distant(sb)
    return sb.build()


@pytest.mark.parametrize("strategy", ["uniform", "power", "spatial"])
def test_light_selection_follows_the_restated_distribution(ctx, strategy, monkeypatch):
    """Every sample's radiance is c_j(p) / pdf_j for exactly one light j, pdf_j from the restated distribution (the hit point's voxel for
    "spatial"; "uniform" with three lights IS "spatial"); over the film each light is chosen within five binomial standard deviations of its
    expected count; and the lazily filled grid gives the dense grid's film bit for bit."""
    sd = selection_scene(strategy)
    run = Run(ctx, sd)
    p, hit, edge = plane_hit(run.o, run.d, 0.0, FLOOR, P_ERR)
    terms = delta_terms(run, p)
    pdf, pdf_rel, vnear = selection_pdfs(run, p, strategy)
    use = hit & ~edge & ~vnear & ~(terms[0][2] | terms[1][2] | terms[2][2])
    print("selection %s: world bound %s %s, hits %d, edge %d, voxel-face / probe near %d, cone near %d" % (
        strategy, run.wb_min, run.wb_max, hit.sum(), (hit & edge).sum(), (hit & vnear).sum(), (hit & (terms[0][2] | terms[1][2] | terms[2][2])).sum()))
    assert (hit & ~use).mean() <= NEAR_CAP, (hit & ~use).mean()
    matches = np.zeros((len(p), 3), bool)
    for j, (c, rel, _, _) in enumerate(terms):
        want = c / pdf[:, j:j + 1]
        bound = (rel + pdf_rel[:, j] + 2 * EPS)[:, None] * want
        matches[:, j] = (np.abs(run.rad - want) <= bound).all(1)
    assert (matches[use].sum(1) == 1).all(), np.bincount(matches[use].sum(1))
    n = int(use.sum())
    for j in range(3):
        expect, var = pdf[use, j].sum(), (pdf[use, j] * (1 - pdf[use, j])).sum()
        print("selection %s: light %d chosen %d times of %d, expected %.2f, standard deviation %.3f" % (strategy, j, matches[use, j].sum(), n, expect, np.sqrt(var)))
        assert abs(matches[use, j].sum() - expect) <= 5 * np.sqrt(var), (strategy, j, int(matches[use, j].sum()), expect, n)
    assert (pdf[use] > 0).all() and np.allclose(pdf[use].sum(1), 1.0)
    if strategy == "spatial":
        assert pdf[use, 1].min() < 0.01 < pdf[use, 1].max()                           # the narrow spot sits on the min_contrib floor where its cone misses the voxel
        monkeypatch.setenv("PBRTGPU_LIGHT_GRID_DENSE_MAX", "0")
        lazy = Run(ctx, sd)
        assert np.array_equal(lazy.rad.astype(f32).view(np.uint32), run.rad.astype(f32).view(np.uint32))
        assert lazy.shadow_rays == run.shadow_rays
    if strategy == "uniform":
        spatial = Run(ctx, selection_scene("spatial"))
        assert np.array_equal(spatial.rad, run.rad)


# ---------------------------------------------------------------- 5. beside area lights
@pytest.mark.parametrize("integ", ["whitted", "all"])
def test_delta_lights_add_to_an_area_light(ctx, integ):
    """An emissive quad listed first, then a spot and a distant light: per sample, the radiance is the area-lit scene's plus the closed-form
    delta terms.  The area light's two triangles precede the new lights, so its sample points do not move (Q23: every array comes from
    dimensions 5, 6; whitted draws light by light in list order)."""
    def scene(with_delta):
        sb = base(integ, res=16, spp=4)
        floor(sb)
        sb.material_none()
        sb.area_light_source_diffuse(L=(8, 8, 8))
        sb.shape_trianglemesh([1.2, 1.0, 3.8, 1.7, 1.0, 3.8, 1.7, 1.5, 3.8, 1.2, 1.5, 3.8], [0, 2, 1, 0, 3, 2], twosided=False)      # faces down
        sb.no_area_light()
        if with_delta:
            add_spot(sb)
            add_distant(sb, frm=(0.0, -1.0, 1.0))                 # its shadow segments pass z = 3.8 at y <= -1.8: clear of the emitter
        return sb.build()
    area = Run(ctx, scene(False))
    both = Run(ctx, scene(True))
    assert both.info.n_lights == 4 and area.info.n_lights == 2
    p, hit, edge = plane_hit(both.o, both.d, 0.0, FLOOR, P_ERR)
    assert np.array_equal(area.o, both.o) and area.rad[hit].sum() > 0
    terms = delta_terms(both, p, occluders=[(1.2, 1.7, 1.0, 1.5, 3.8)])
    skip = edge | (hit & (terms[0][2] | terms[1][2]))
    assert skip.mean() <= NEAR_CAP
    ok = hit & ~skip
    s, d = terms[0][0][ok], terms[1][0][ok]
    want = area.rad[ok] + s + d
    # the area-lit sum is the same f32 value in both scenes; then two more f32 additions, each one rounding of the running sum
    bound = terms[0][1][ok][:, None] * s + terms[1][1][ok][:, None] * d + 2 * EPS * want
    assert (np.abs(both.rad[ok] - want) <= bound).all(), float((np.abs(both.rad[ok] - want) / bound).max())
    assert np.array_equal(both.rad[~hit & ~edge], area.rad[~hit & ~edge])
    assert (s.sum(1) > 0).sum() > 50 and (d.sum(1) > 0).all()


# ---------------------------------------------------------------- 6. every shading route
def route_oren(sb):
    floor(sb, sigma=20.0)


def route_texture(sb):
    img = np.tile(np.array(KD, np.float32), (4, 4, 1))
    sb.material_matte(sb.texture_imagemap(sb.image_pyramid(img)))
    quad(sb, FLOOR[0], FLOOR[1], FLOOR[2], FLOOR[3], 0.0, uv=True)


def route_sphere(sb):
    floor(sb)
    t = scenes.transform_translate(6.0, 3.5, 0.3)             # 40 degrees off the view axis: outside the film's 33-degree corners
    sb.shape_sphere(radius=0.25, object_to_world=t[0], world_to_object=t[1])


def route_instance(sb):
    floor(sb)
    sb.object_begin("o")
    quad(sb, -0.1, 0.1, -0.1, 0.1, 0.0)
    sb.object_end()
    sb.object_instance("o", to_world=scenes.transform_translate(6.0, 3.5, 0.3))


@pytest.mark.parametrize("route", [route_oren, route_texture, route_sphere, route_instance], ids=["oren_nayar", "kd_imagemap", "sphere", "instance"])
@pytest.mark.parametrize("integ", ["path", "all"])
def test_every_shading_route_gives_the_closed_form(ctx, route, integ):
    """The lit quad through the lobe-list kernel (Oren-Nayar), k_tex_resolve + the _res kernel (a Kd image map of one colour), the sphere
    family and the instanced kernel (an unlit sphere / instance out of view and out of every shadow segment's way)."""
    sb = base(integ)
    route(sb)
    add_spot(sb)
    if integ != "path":                          # `path` estimates one light per vertex (test 4 holds its selection); here it gets the spot alone
        add_distant(sb)
    run = Run(ctx, sb.build())
    p, hit, edge = plane_hit(run.o, run.d, 0.0, FLOOR, P_ERR)
    brdf, extra = None, 0.0
    if route is route_oren:
        wo = -ref.normalize(run.d)
        # OrenNayar::f: sin / cos of both directions, the azimuth difference, A + B max_cos sin_a tan_b: 30 more roundings
        extra = 30 * EPS

        def brdf(wi, wo=wo):
            return np.concatenate([ref.oren_nayar_f(KD, 20.0, wo[i], wi[i:i + 1]) for i in range(len(wi))])
    if route is route_texture:
        extra = 12 * EPS                   # the filtered lookup of a constant image: a weighted mean of equal texels, divided by the weights' sum
    terms = delta_terms(run, p, brdf=brdf)
    want = np.where(hit[:, None], sum(t[0] for t in terms), 0.0)
    rel = np.max([t[1] for t in terms], 0) + extra + 2 * EPS
    n_lit, _ = check_closed_form(run, want, rel, edge | (hit & np.any([t[2] for t in terms], 0)))
    assert n_lit > (300 if integ != "path" else 100)


@pytest.mark.parametrize("integ", ["path", "whitted"])
def test_mirror_then_next_event_estimation(ctx, integ):
    """The camera sees the floor in a mirror (a specular bounce, then NEE at the floor) and directly.  maxdepth 2: no second diffuse vertex,
    so the floor's own light never comes back through the mirror."""
    kr = 0.8
    sb = base(integ, maxdepth=2, res=24)
    floor(sb)
    sb.material_mirror(Kr=(kr, kr, kr))
    sb.shape_trianglemesh([-2, 2, 0, 2, 2, 0, 2, 2, 3, -2, 2, 3], [0, 1, 2, 0, 2, 3])              # the plane y = 2 behind the floor
    add_spot(sb, coneangle=40.0)
    if integ != "path":
        add_distant(sb)
    run = Run(ctx, sb.build())
    p, hit, edge = plane_hit(run.o, run.d, 0.0, FLOOR, P_ERR)
    t = (2.0 - run.o[:, 1]) / run.d[:, 1]
    pm = run.o + t[:, None] * run.d
    on_mirror = ~hit & (t > 0) & (np.abs(pm[:, 0]) < 2) & (pm[:, 2] > 0) & (pm[:, 2] < 3)
    m_edge = (t > 0) & ~hit & (np.abs(np.minimum(np.minimum(2 - np.abs(pm[:, 0]), pm[:, 2]), 3 - pm[:, 2])) <= P_ERR)
    rd = run.d * np.array([1.0, -1.0, 1.0])
    # the reflected ray starts at the f32 mirror point pushed off the surface by its error bound (gamma(7) |p|) and is renormalised: over the
    # ~6 units to the floor the hit point moves by at most 256 EPS EXTENT
    p_err2 = 256 * EPS * EXTENT
    p2, hit2, edge2 = plane_hit(pm, rd, 0.0, FLOOR, p_err2)
    hit2 &= on_mirror
    edge2 &= on_mirror
    direct = delta_terms(run, p)
    refl = delta_terms(run, p2, p_err=p_err2)
    want = np.where(hit[:, None], sum(t[0] for t in direct), np.where(hit2[:, None], kr * sum(t[0] for t in refl), 0.0))
    rel = np.where(hit, np.max([t[1] for t in direct], 0), np.max([t[1] for t in refl], 0) + 8 * EPS) + 2 * EPS
    skip = edge | m_edge | edge2 | (hit & np.any([t[2] for t in direct], 0)) | (hit2 & np.any([t[2] for t in refl], 0))
    n_lit, n_zero = check_closed_form(run, want, rel, skip)
    assert (hit2 & ~skip & (want.sum(1) > 0)).sum() > 100


# ---------------------------------------------------------------- 8. CLI
def test_cli_renders_the_scene_builder_film(ctx, tmp_path):
    """pbrt_gpu -i on a spot- and distant-lit .pbrt gives the film of the same scene built with SceneBuilder, bit for bit."""
    sb = base("path", res=16, spp=4)
    floor(sb)
    add_spot(sb)
    add_distant(sb)
    ctx.upload(sb.build())
    ctx.film_clear()
    ctx.render()
    want = ctx.film_rgb()
    text = '''LookAt 0 -4 3  0 0 0  0 0 1
Camera "perspective" "float fov" 50
Film "image" "integer xresolution" 16 "integer yresolution" 16 "string filename" "delta.pfm"
PixelFilter "box"
Sampler "sobol" "integer pixelsamples" 4
Integrator "path" "integer maxdepth" 5
WorldBegin
Material "matte" "rgb Kd" [0.6 0.5 0.4]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -2 0 2 -2 0 2 2 0 -2 2 0]
LightSource "spot" "point from" [0.3 -0.2 2.5] "point to" [0.1 0.2 0] "rgb I" [30 20 10] "float coneangle" 25 "float conedelta" 8
LightSource "distant" "point from" [0.4 -1 1.2] "point to" [0 0 0] "rgb L" [1.5 2 2.5]
WorldEnd
'''
    scene = tmp_path / "delta.pbrt"
    scene.write_text(text)
    exe = os.path.join(ROOT, "pbrt-r3_amd", "csrc", "pbrt_gpu")
    out = tmp_path / "delta.pfm"
    r = subprocess.run([exe, "-i", str(scene), "--outfile", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    head = raw.split(b"\n", 3)
    assert head[0] == b"PF" and head[1].split() == [b"16", b"16"]
    img = np.frombuffer(head[3], "<f4" if float(head[2]) < 0 else ">f4").reshape(16, 16, 3)[::-1]
    assert want.sum() > 0 and np.array_equal(img.astype(f32).view(np.uint32), want.view(np.uint32))
