"""The folded next-event estimate against the oracle bit for bit.

A vertex whose estimate has a shadow ray and no probe stores the finished term beta * ((0 + A) / pdf) (pendA.w = +0 marks it) and
k_nee_resolve adds it if the ray was unoccluded; a vertex with a probe ray keeps the three-array form.  The scene: a matte floor, a large
emissive triangle close above it, a blocker that covers part of the emitter, 16 x 16 pixels, 4 spp.

The scene is accepted only if the oracle ALONE shows at least one first vertex of each kind.  With one light (selection pdf 1) a depth-1
sample on the floor returns a + b, a in {A, 0}, b in {B, 0}.  A is restated in float64 from the oracle's own hooks (camera ray, closest
hit, the Sobol' dimensions 6, 7 of the light sample, light_sample_li): A = Kd / pi |cos| Li w / pdf, w the power heuristic against the
cosine pdf.  The oracle's render WITHOUT the blocker gives A + B, so B = L_open - A tells whether the BSDF sample met the emitter (a probe)
or not (shadow only); the render WITH the blocker then tells which of A and B survived.

The same film under an infinite light beside the emitter (the *_env kernels; its probe counts when it escapes) is held to the oracle as
well.  The oracle renders no delta lights: the spot-lit film (k_shade_delta, no probe at all: every estimate folds) is held to the float64
restatement of tests/delta_light_ref.py within the bound it derives, lit and shadowed samples both present."""
import numpy as np
import pytest

import delta_light_ref as dref
from helpers import bits, scenes

pytestmark = pytest.mark.gpu

KD = (0.6, 0.5, 0.4)
RES, SPP = 16, 4
FLOOR = (-2.0, 2.0, -2.0, 2.0)
BLOCKER = (-0.2, 1.4, -1.0, 0.6, 0.45)            # x0 x1 y0 y1 z
TOL = 1e-4                                        # float64 restatement of an f32 estimate: a few dozen roundings of 6e-8


def scene(depth, blocker=True, light="area", blocker_material="matte"):
    sb = scenes.SceneBuilder()
    sb.look_at((0, -4, 3), (0, 0, 0), (0, 0, 1))
    sb.camera_perspective(fov=50.0)
    sb.film(xresolution=RES, yresolution=RES)
    sb.pixel_filter_box()
    sb.sampler_sobol(pixelsamples=SPP)
    sb.integrator_path(maxdepth=depth)
    sb.material_matte(KD)
    sb.shape_trianglemesh([(FLOOR[0], FLOOR[2], 0), (FLOOR[1], FLOOR[2], 0), (FLOOR[1], FLOOR[3], 0), (FLOOR[0], FLOOR[3], 0)], [0, 1, 2, 0, 2, 3])
    if blocker:
        if blocker_material == "none":
            sb.material_none()
        x0, x1, y0, y1, z = BLOCKER
        sb.shape_trianglemesh([(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)], [0, 1, 2, 0, 2, 3])
    if light == "spot":
        sb.light_spot(I=(30.0, 20.0, 10.0), coneangle=40.0, conedelta=8.0, frm=(0.3, -0.2, 2.5), to=(0.1, 0.2, 0.0))
        return sb.build()
    sb.area_light_source_diffuse(L=(4, 4, 4), twosided=False)
    sb.shape_trianglemesh([(-1.5, -1.5, 1.0), (0.0, 1.8, 1.0), (1.5, -1.5, 1.0)], [0, 1, 2])           # faces down
    sb.no_area_light()
    if light == "env":
        sb.light_infinite(L=(0.5, 0.6, 0.7))
    return sb.build()


def camera_samples(osc):
    b = tuple(osc.info.sample_bounds)
    ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
    pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), SPP, axis=0).astype(np.int32)
    si = np.tile(np.arange(SPP, dtype=np.uint32), xs.size)
    return b, pix, si


def first_vertex_kinds(oracle):
    """From the oracle alone: how many depth-1 floor samples are (shadow only & unoccluded, shadow only & occluded, probe that hits, probe that misses)."""
    o_open, o_full = oracle.scene(scene(1, blocker=False)), oracle.scene(scene(1))
    b, pix, si = camera_samples(o_full)
    l_open = o_open.radiance_samples(b).reshape(-1, 3).astype(np.float64)
    l_full = o_full.radiance_samples(b).reshape(-1, 3).astype(np.float64)
    o, d, _ = o_full.generate_camera_rays(pix, si)
    hit, _ = o_full.trace_closest(o, d, np.full(len(o), np.inf, np.float32))
    p = o.astype(np.float64) + hit["t"].astype(np.float64)[:, None] * d
    floor = (hit["prim"] >= 0) & (np.abs(p[:, 2]) < 1e-4)
    # the camera sample takes dimensions 0-4, the light pick dimension 5 (one light: always it), the light sample 6, 7
    u = np.stack([o_full.sobol_samples(pix, si, np.full(len(si), k, np.uint32)) for k in (6, 7)], 1)
    li, wi, pdf = o_full.light_sample_li(0, p.astype(np.float32), u)
    o_open.close()
    o_full.close()
    cos = np.abs(wi[:, 2].astype(np.float64))
    pdf = pdf.astype(np.float64)
    with np.errstate(all="ignore"):
        w = pdf ** 2 / (pdf ** 2 + (cos / np.pi) ** 2)
        a = np.where((pdf > 0)[:, None], (np.array(KD) / np.pi)[None, :] * cos[:, None] * li * (w / pdf)[:, None], 0.0)
    bterm = l_open - a
    scale = np.maximum(l_open.max(1), 1e-30)

    def near(x, y):
        return np.abs(x - y).max(1) <= TOL * scale
    zero = np.zeros_like(a)
    has_a = floor & (a.min(1) > 10 * TOL * scale)
    shadow_only = has_a & near(bterm, zero)
    probe = has_a & (bterm.min(1) > 10 * TOL * scale) & (np.abs(bterm - a).max(1) > 10 * TOL * scale)       # (A and B told apart)
    kinds = (shadow_only & near(l_full, a), shadow_only & near(l_full, zero),
             probe & (near(l_full, bterm) | near(l_full, l_open)), probe & (near(l_full, a) | near(l_full, zero)))
    assert (bterm[floor].min(1) >= -TOL * scale[floor]).all()                                              # the restated A never exceeds the oracle's A + B
    return tuple(int(k.sum()) for k in kinds), int(floor.sum())


def check_against_oracle(gpu_ctx, oracle, sd):
    osc = oracle.scene(sd)
    gpu_ctx.upload(sd)
    b = tuple(gpu_ctx.info.sample_bounds)
    g, r = gpu_ctx.radiance_samples(b), osc.radiance_samples(b)
    assert r.sum() > 0 and np.isfinite(r).all()
    differ = int((bits(g) != bits(r)).any(-1).sum())
    print("per-sample radiance: %d of %d samples differ" % (differ, g.shape[0] * g.shape[1]))
    assert differ == 0
    gpu_ctx.film_clear()
    gpu_ctx.reset_counters()
    gpu_ctx.render()
    gc = gpu_ctx.counters()
    _, oc, _ = osc.render(threads=4, want_image=False)
    osc.close()
    for k in ("camera_rays", "regular_rays", "shadow_rays", "path_vertices"):
        assert gc[k] == oc[k], (k, gc[k], oc[k])
    return r


@pytest.fixture(scope="module")
def kinds(oracle):
    k, n_floor = first_vertex_kinds(oracle)
    print("oracle alone, %d depth-1 floor samples: shadow only unoccluded %d, shadow only occluded %d, probe hits %d, probe misses %d" % ((n_floor,) + k))
    return k


@pytest.mark.parametrize("depth", [1, 5])
def test_folded_and_three_array_vertices(gpu_ctx, oracle, kinds, depth):
    assert min(kinds) >= 1, kinds
    check_against_oracle(gpu_ctx, oracle, scene(depth))


@pytest.mark.parametrize("depth", [1, 5])
def test_under_an_infinite_light(gpu_ctx, oracle, depth):
    """Two lights: the emitter (its shadow-only vertices fold) and the environment (its probe counts when it escapes, k_nee_resolve_env)."""
    r_full = check_against_oracle(gpu_ctx, oracle, scene(depth, light="env"))
    o_open = oracle.scene(scene(depth, blocker=False, light="env"))
    r_open = o_open.radiance_samples(tuple(o_open.info.sample_bounds))
    o_open.close()
    changed = (bits(r_full) != bits(r_open)).any(-1)
    assert changed.sum() > 20 and (~changed & (r_full.sum(-1) > 0)).sum() > 20            # the blocker takes light from some samples and leaves others alone


@pytest.mark.parametrize("depth", [1, 5])
def test_under_a_spot_light(gpu_ctx, depth):
    """No probe ray: every estimate folds.  A "none" blocker casts a shadow and reflects nothing, the matte floor cannot see itself: each
    floor sample is Kd / pi Li |cos| or 0 at any depth."""
    eps = dref.EPS
    sd = scene(depth, light="spot", blocker_material="none")
    info = gpu_ctx.upload(sd)
    b = tuple(info.sample_bounds)
    rad = gpu_ctx.radiance_samples(b).reshape(-1, 3).astype(np.float64)
    ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
    pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), SPP, axis=0).astype(np.int32)
    o, d, _ = gpu_ctx.generate_camera_rays(pix, np.tile(np.arange(SPP, dtype=np.uint32), xs.size))
    o, d = o.astype(np.float64), d.astype(np.float64)
    p_err = 16 * eps * 4.0
    wb = np.array(list(info.world_bound), np.float64)
    lt = dref.from_record(sd.delta_lights[0], 0.5 * np.sqrt(((wb[3:] - wb[:3]) ** 2).sum()))

    def rect(z, r, margin):
        t = (z - o[:, 2]) / d[:, 2]
        q = o + t[:, None] * d
        ex = np.minimum(np.minimum(q[:, 0] - r[0], r[1] - q[:, 0]), np.minimum(q[:, 1] - r[2], r[3] - q[:, 1]))
        return q, (t > 0) & (ex > margin), (t > 0) & (np.abs(ex) <= margin)
    p, on_floor, floor_edge = rect(0.0, FLOOR, p_err)
    p[:, 2] = 0.0
    _, through, through_edge = rect(BLOCKER[4], BLOCKER[:4], p_err)                # the camera ray passes the blocker first: re-spawned, left out
    s = dref.sample_li(lt, p, p_err)
    cos = s["wi"][:, 2]
    want = (np.array(KD) / np.pi)[None, :] * s["li"] * np.abs(cos)[:, None]
    rel = s["li_rel"] + 3 * s["wi_err"] / np.maximum(np.abs(cos), 1e-30) + 14 * eps
    tgt = s["target"]
    uu = (BLOCKER[4] - p[:, 2]) / (tgt[:, 2] - p[:, 2])
    q = p + uu[:, None] * (tgt - p)
    ex = np.minimum(np.minimum(q[:, 0] - BLOCKER[0], BLOCKER[1] - q[:, 0]), np.minimum(q[:, 1] - BLOCKER[2], BLOCKER[3] - q[:, 1]))
    margin = 8 * p_err + 64 * eps * 4.0
    shadowed = (uu > 0) & (uu < 1) & (ex > 0)
    near = s["near"] | ((uu > 0) & (uu < 1) & (np.abs(ex) <= margin))
    use = on_floor & ~floor_edge & ~through & ~through_edge & ~near
    want = np.where(shadowed[:, None], 0.0, want)
    lit, dark = use & (want.sum(1) > 0), use & shadowed & (s["li"].sum(1) > 0)
    print("spot, depth %d: %d floor samples used, %d lit, %d in the blocker's shadow" % (depth, use.sum(), lit.sum(), dark.sum()))
    assert lit.sum() > 50 and dark.sum() > 20
    assert (rad[use & (want.sum(1) == 0)] == 0).all()
    err = np.abs(rad[lit] - want[lit]) / want[lit]
    assert (err <= rel[lit][:, None]).all(), float((err / rel[lit][:, None]).max())
