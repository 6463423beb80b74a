"""k_trace's loop around the node and leaf rounds -- the service part: the prefetch state machine (which a complete reservation now
branches past), the retire stores and the hand-out of prefetched rays.  Whatever is rearranged there, a ray must do what it did and
its result must be stored exactly once.  (Two such rearrangements were built with this file and not kept, tools/patches/r06_*.patch:
node rounds in runs without a service pass between them, and the retire stores issued after the hand-out's shuffles.)

The scene is a stack of sheets over a floor: 64 stacks of 2-4 parallel triangles 0.01 apart above a floor of 128 triangles, stored
top-down in half of the stacks and bottom-up in the other half.  The rays: a fifth passes between the stacks and the light
(they end in a node round, without one triangle test: that is where the retire is furthest from the hand-out that stores it), a quarter skims over the floor at the stacks' height (long runs of node
visits), the others go through a stack from above or below, perpendicular, oblique or grazing, with t_max infinite or cut between two sheets, dealt as continuation, shadow and
probe items.  What the set is for is checked with the oracle alone, ray by ray (test_oracle_alone_meets_the_conditions).  On the GPU
every hit, t, barycentric, occlusion flag and the four counters must equal the oracle's at batch sizes on either side of
PT_REFILL_MIN (8), of one reservation (64) and of one block (1 024)."""
import os

import numpy as np
import pytest

from helpers import bits, scenes
from test_gpu_wavefront import _check

GAP = 0.01
N_STACKS = 64
SPACING = 2.0
FLOOR_Y = -1.0
SIZES = [1, 7, 8, 9, 63, 64, 65, 127, 129, 1023, 1025, 4097]


def _stack_table():
    """(centre x, centre z, lowest sheet's y, sheets, stored top-down) per stack."""
    return [(SPACING * (s % 8 - 3.5), SPACING * (s // 8 - 3.5), 0.3 * (s % 4), 2 + s % 3, (s // 3) % 2 == 1) for s in range(N_STACKS)]


def sheets_over_floor(res=16, spp=1, maxdepth=2, filter_width=0.5):
    b = scenes.SceneBuilder()
    b.look_at((0, 9.0, -16.0), (0, 0, 0), (0, 1, 0))
    b.camera_perspective(fov=45.0)
    b.film(xresolution=res, yresolution=res)
    b.pixel_filter_box(filter_width, filter_width)
    b.sampler_sobol(spp)
    b.integrator_path(maxdepth=maxdepth)
    b.accelerator_bvh("sah", 4)
    b.material_matte((0.6, 0.5, 0.4))
    b.area_light_source_diffuse(L=(8, 8, 8))
    scenes._quad(b, (3, 12, -3), (3, 12, 3), (-3, 12, 3), (-3, 12, -3))
    b.no_area_light()
    g = np.linspace(-8.0, 8.0, 9)
    for i in range(8):                                   # the floor: 8 x 8 quads
        for j in range(8):
            scenes._quad(b, (g[i], FLOOR_Y, g[j]), (g[i], FLOOR_Y, g[j + 1]), (g[i + 1], FLOOR_Y, g[j + 1]), (g[i + 1], FLOOR_Y, g[j]))
    for cx, cz, y0, n, top_down in _stack_table():
        ys = y0 + GAP * np.arange(n)
        if top_down:
            ys = ys[::-1]
        P, idx = [], []
        for k, y in enumerate(ys):
            P += [(cx - 0.8, y, cz - 0.8), (cx + 0.8, y, cz - 0.8), (cx, y, cz + 1.0)]
            idx += [3 * k, 3 * k + 1, 3 * k + 2]
        b.shape_trianglemesh(np.asarray(P, np.float32), idx)
    return b.build()


def make_rays(n=4097, seed=11):
    """Origins, directions, t_max, kinds.  Every stack ray has |dy| = 1, so t is the distance along y."""
    rng = np.random.default_rng(seed)
    tab = _stack_table()
    o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32); tmax = np.full(n, np.inf, np.float32)
    for i in range(n):
        u = rng.uniform()
        if u < 0.2:                                      # between the stacks and the light, parallel to the floor: nodes, no triangle
            a = rng.uniform(0, 2 * np.pi)
            o[i] = (-12.0 * np.cos(a) + rng.uniform(-4, 4) * np.sin(a), rng.uniform(1.5, 10.0), -12.0 * np.sin(a) - rng.uniform(-4, 4) * np.cos(a))
            d[i] = (np.cos(a), 0.0, np.sin(a))
        elif u < 0.45:                                   # skimming over the floor at the stacks' height, sinking slowly: long runs of node visits
            a = rng.uniform(0, 2 * np.pi)
            o[i] = (-12.0 * np.cos(a) + rng.uniform(-4, 4) * np.sin(a), rng.uniform(0.0, 1.0), -12.0 * np.sin(a) - rng.uniform(-4, 4) * np.cos(a))
            d[i] = (np.cos(a), rng.uniform(-0.15, -0.05), np.sin(a))
        else:                                            # through a stack, from above or from below (from between floor and stack)
            cx, cz, y0, ns, top_down = tab[rng.integers(N_STACKS)]
            s = -1.0 if rng.uniform() < 0.6 else 1.0
            shape = rng.integers(4)                      # perpendicular, one zero component, oblique, grazing (low over the neighbouring stacks)
            dx, dz = (0.0, 0.0) if shape == 0 else ((rng.uniform(-0.2, 0.2), 0.0) if shape == 1 else rng.uniform(-0.2, 0.2, 2))
            if shape == 3:
                dx, dz = rng.uniform(-3.0, 3.0, 2)
            tx, tz = cx + rng.uniform(-0.2, 0.2), cz + rng.uniform(-0.2, 0.2)
            mid = y0 + 0.5 * GAP * (ns - 1)
            dist = rng.uniform(0.5, 0.9) if s > 0 else (rng.uniform(0.3, 1.2) if shape == 3 else rng.uniform(2.0, 5.0))
            o[i] = (tx - dx * dist, mid - s * dist, tz - dz * dist)
            d[i] = (dx, s, dz)
            if rng.uniform() < 0.25:                     # cut between two sheets (or just behind the only other one)
                tmax[i] = np.float32(dist + GAP * (rng.integers(0, ns) - 0.5 * (ns - 1) + 0.5))
    kind = np.asarray([1, 2, 3], np.uint8)[rng.integers(0, 3, n)]
    return o, d, tmax, kind


def ray_by_ray(osc, rays):
    """Per ray, from the oracle alone: node visits, triangle tests, accepted any-hit, closest hit that accepts more than one triangle.

    The last one without looking inside the traversal: the order of a ray's tests does not depend on t_max (a smaller t_max only
    drops tests), closest-hit and any-hit traversal run the same steps up to the first accept, and an any-hit traversal's
    tris_tested is the position of its first accept.  If a closest-hit ray that ends on P accepted P alone, P is its first accept at
    position k; with t_max = nextafter(t_P) nothing but P can be accepted, and P's position can only have shrunk.  So an any-hit
    count with the tight t_max ABOVE the count with the ray's own t_max proves an accept before P."""
    o, d, tmax, kind = rays
    n = len(kind)
    nodes = np.zeros(n, np.int64); tris = np.zeros(n, np.int64)
    occluded = np.zeros(n, bool); multi = np.zeros(n, bool)
    for i in range(n):
        oi, di, ti = o[i:i + 1], d[i:i + 1], tmax[i:i + 1]
        if kind[i] == 2:
            occ, c = osc.trace_any(oi, di, ti)
            occluded[i] = bool(occ[0])
        else:
            r, c = osc.trace_closest(oi, di, ti)
            if r["prim"][0] >= 0:
                _, c_own = osc.trace_any(oi, di, ti)
                tight = np.nextafter(r["t"].astype(np.float32), np.float32(np.inf))
                occ, c_tight = osc.trace_any(oi, di, tight)
                multi[i] = bool(occ[0]) and c_tight["tris_tested"] > c_own["tris_tested"]
        nodes[i] = c["nodes_visited"]; tris[i] = c["tris_tested"]
    return nodes, tris, occluded, multi


@pytest.fixture(scope="module")
def sheets(oracle):
    sd = sheets_over_floor()
    osc = oracle.scene(sd)
    yield sd, osc, make_rays()
    osc.close()


def test_oracle_alone_meets_the_conditions(sheets):
    """(no GPU) The ray set does what it is for, whatever the kernel does with it."""
    sd, osc, rays = sheets
    assert 200 <= sd.desc.n_triangles <= 400
    assert len(rays[3]) == max(SIZES)
    nodes, tris, occluded, multi = ray_by_ray(osc, rays)
    print("no triangle test %.3f, accepted any-hits %.3f, closest hits with several accepts %.3f, node visits per ray %.2f"
          % ((tris == 0).mean(), occluded.mean(), multi.mean(), nodes.mean()))
    assert ((tris == 0) & (nodes >= 1)).mean() >= 0.1       # ... and not for having missed the root's box
    assert occluded.mean() >= 0.1
    assert multi.mean() >= 0.1
    assert nodes.mean() >= 4.0
    # ... and already in the batch that fills one block, the smallest in which lanes are refilled many times
    assert (tris[:1023] == 0).mean() >= 0.1 and occluded[:1023].mean() >= 0.1 and multi[:1023].mean() >= 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_mixed_batches_exact(sheets, gpu_ctx, n):
    sd, osc, rays = sheets
    gpu_ctx.upload(sd)
    o, d, tmax, kind = (a[:n] for a in rays)
    _check(gpu_ctx, osc, o, d, tmax, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3])
def test_single_kind_batches_exact(sheets, gpu_ctx, k):
    """The same batches with every item a continuation ray, a shadow ray, a probe ray."""
    sd, osc, rays = sheets
    gpu_ctx.upload(sd)
    for n in SIZES:
        o, d, tmax = (a[:n] for a in rays[:3])
        _check(gpu_ctx, osc, o, d, tmax, np.full(n, k, np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 129, 1025])
def test_every_ray_stored_exactly_once(sheets, gpu_ctx, n):
    """Two calls of one size with different rays: a ray of the second call that was never stored would show the first call's value."""
    sd, osc, rays = sheets
    gpu_ctx.upload(sd)
    first = tuple(a[:n] for a in rays)
    second = tuple(a[n:2 * n][::-1] for a in rays)
    r1, _ = osc.trace_closest(first[0], first[1], first[2])
    r2, _ = osc.trace_closest(second[0], second[1], second[2])
    assert (r1["prim"] != r2["prim"]).mean() > 0.5          # the two sets do differ, item by item
    _check(gpu_ctx, osc, *first)
    _check(gpu_ctx, osc, *second)


@pytest.mark.gpu
def test_small_render_exact(gpu_ctx, oracle):
    """16 x 16, 4 spp, path depth 5, at the smallest path pool there is: every bounce's launch ends with a dry queue (the drain, which
    retires in every iteration), some ten times in the frame.  Film and counters equal to the oracle's, bit for bit.

    The box filter is 0.45 wide, not the default 0.5: at 0.5 a sample on a pixel's edge (the Sobol' points are dyadic: many are) also lands in
    the neighbouring pixel, and where samples of DIFFERENT pixels meet in one sum the film is defined only up to the order of the additions --
    the reference merges tiles in any order, the device adds with float atomics (tests/test_gpu_features.py,
    test_pass_structure_does_not_change_the_film).  At 0.5 the parent commit's kernel and this one both differ from the oracle in the
    same 12 of 256 pixels by 1-2 ulp with every sample's radiance bit-equal; below 0.5 a sample's footprint is its own pixel, the sum
    runs in sample order on both sides and every bit is defined."""
    sd = sheets_over_floor(res=16, spp=4, maxdepth=5, filter_width=0.45)
    osc = oracle.scene(sd)
    gpu_ctx.upload(sd)
    os.environ["PBRTGPU_POOL_PATHS"] = "65536"
    try:
        gpu_ctx.film_clear(); gpu_ctx.reset_counters(); gpu_ctx.render()
        gx, gc = gpu_ctx.film_xyzw().copy(), gpu_ctx.counters()
    finally:
        os.environ.pop("PBRTGPU_POOL_PATHS", None)
    ox, oc, _ = osc.render(threads=4)
    osc.close()
    assert gc["trace_launches"] >= 5
    for k in ("camera_rays", "regular_rays", "shadow_rays", "path_vertices", "nodes_visited", "tris_tested"):
        assert gc[k] == oc[k], (k, gc[k], oc[k])
    assert ox[..., :3].sum() > 0 and (ox[..., 3] >= 2.0).all()        # every pixel keeps at least two of its four samples
    same = np.all(bits(gx) == bits(ox), axis=-1)
    print("bit-equal pixels: %d of %d" % (int(same.sum()), same.size))
    assert same.all()
