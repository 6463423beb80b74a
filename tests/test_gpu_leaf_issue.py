"""The pooled leaf round's issue half on rounds of known shape.  In a leaf round of k_trace the parked lanes' leaves are pooled: owners
are served in lane order while their whole leaf fits into the wave's 64 items, and lane i learns which triangle of which owner it tests
from the owner map (tests/test_leaf_item_map.py is the scheme's model).  The other leaf tests vary what a leaf's
triangles do to t_max; none controls how a round's items fall on the lanes.

Stacked sheets again (tests/test_gpu_leaf_accept.py), but 64 well-separated clusters of exactly s sheets each, one scene per s, so that
every leaf holds s triangles; and one ray per cluster, so that the 64 lanes of a wave park on 64 different leaves of s triangles: 64 s
items.  s = 8 makes rounds of exactly eight owners (an exact fit of 64), s = 7 nine owners, 63 items and a tenth owner that must stay
parked, s = 3 and s = 5 put first items on odd lanes across every row of 16, and a mixed scene cycles 1..8 over the clusters.  That the
leaves are what they are meant to be is asserted from the oracle alone (see SCENES for what a leaf limit of 8 can and cannot give).
Hits, t, barycentrics, occlusion, probe records and the four counters must equal the oracle's, ray by ray, at 1 ray (the only round is
the "nothing else can run" round with one owner), around the leaf round's trigger of 18 parked lanes (17, 18, 19), around one wave
(63, 64, 65) and at one block and one lane (1 025: lanes refilled many times)."""
import numpy as np
import pytest

from helpers import scenes
from test_gpu_wavefront import _check

GAP = 0.01                     # distance between two sheets of a cluster
N_CLUSTERS = 64
SPACING = 4.0
N_POOL = 2 * 1025

# (sheets per cluster: s, or 0 for 1..8 cycling over the clusters; leaf limit).
# The builder (the reference's, restated by the oracle) makes a leaf of ANY group of at most `limit` triangles, before it looks at a cost.  At a
# limit of 8 a cluster of s >= 5 sheets is therefore a leaf of its own (two clusters never fit), but clusters of s <= 4 cannot all be: a group
# of more than 8 triangles would have to split into sides that are each one cluster or more than 8 triangles, and the last such split (of
# 9..16 triangles) always leaves a side of 2..8 that holds more than one cluster.  No geometry changes that.  So the scenes of s = 1, 2, 3 are
# built twice: at the limit of 8, where a leaf pools several neighbouring clusters (every ray still tests whole leaves), and at a
# limit of s, where every cluster is exactly one leaf of s triangles.  EXACT lists the scenes on which the oracle must show that.
SCENES = [(1, 8), (2, 8), (3, 8), (5, 8), (7, 8), (8, 8), (1, 1), (2, 2), (3, 3), (0, 8), (0, 4)]
EXACT = [(5, 8), (7, 8), (8, 8), (1, 1), (2, 2), (3, 3)]


def _cluster_table(s):
    """(centre x, centre y, centre z, sheets, stored far-to-near in +z, reversed winding) per cluster."""
    out = []
    for c in range(N_CLUSTERS):
        n = s if s else 1 + (c + c // 8) % 8                # mixed: 1..8, shifted from row to row of the grid
        out.append((SPACING * (c % 8 - 3.5), SPACING * (c // 8 - 3.5), 0.25 * (c % 5), n, (c // 2) % 2 == 1, c % 2 == 1))
    return out


def cluster_scene(s, leaf):
    b = scenes.SceneBuilder()
    b.look_at((0, 0, -60.0), (0, 0, 0), (0, 1, 0))
    b.camera_perspective(fov=40.0)
    b.film(xresolution=16, yresolution=16)
    b.pixel_filter_box()
    b.sampler_sobol(1)
    b.integrator_path(maxdepth=2)
    b.accelerator_bvh("sah", leaf)
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=(1, 1, 1))
    scenes._quad(b, (1, 40, -1), (1, 40, 1), (-1, 40, 1), (-1, 40, -1))
    b.no_area_light()
    for cx, cy, cz, n, far_first, reverse in _cluster_table(s):
        zs = cz + GAP * np.arange(n)
        if far_first:
            zs = zs[::-1]
        P, idx = [], []
        for j, z in enumerate(zs):
            P += [(cx - 1.0, cy - 1.0, z), (cx + 1.0, cy - 1.0, z), (cx, cy + 1.2, z)]
            idx += [3 * j, 3 * j + 2, 3 * j + 1] if reverse else [3 * j, 3 * j + 1, 3 * j + 2]
        b.shape_trianglemesh(np.asarray(P, np.float32), idx)
    return b.build()


def cluster_rays(s, seed=11):
    """The ray pool: ray i is aimed at cluster i % 64, so every 64 consecutive rays park on 64 different leaves.  Perpendicular (two infinite
    reciprocals) and oblique rays alternate, from both sides, t_max infinite, kinds dealt at random."""
    rng = np.random.default_rng(seed)
    tab = _cluster_table(s)
    o, d, cl = [], [], []
    for i in range(N_POOL):
        c = i % N_CLUSTERS
        cx, cy, cz, n, far_first, reverse = tab[c]
        mid = cz + 0.5 * GAP * (n - 1)
        side = 1.0 if rng.integers(2) else -1.0
        dx, dy = (0.0, 0.0) if (i + i // N_CLUSTERS) % 2 == 0 else rng.uniform(-0.2, 0.2, 2)
        tx, ty = cx + rng.uniform(-0.25, 0.25), cy + rng.uniform(-0.25, 0.25)
        dist = rng.uniform(3.0, 6.0)
        d.append((dx, dy, side)); o.append((tx - dx * dist, ty - dy * dist, mid - side * dist))
        cl.append(c)
    o = np.asarray(o, np.float32); d = np.asarray(d, np.float32)
    tmax = np.full(N_POOL, np.inf, np.float32)
    kind = np.asarray([1, 2, 3], np.uint8)[rng.integers(0, 3, N_POOL)]
    return o, d, tmax, kind, np.asarray(cl)


@pytest.fixture(scope="module", params=SCENES, ids=lambda p: "s%d_leaf%d" % p if p[0] else "mixed_leaf%d" % p[1])
def clusters(request, oracle):
    s, leaf = request.param
    sd = cluster_scene(s, leaf)
    osc = oracle.scene(sd)
    rays = cluster_rays(s)
    yield s, leaf, sd, osc, rays
    osc.close()


def test_every_ray_tests_exactly_its_clusters_leaf(clusters):
    """(no GPU, from the oracle alone) On the scenes of EXACT every ray aimed at a cluster tests exactly that cluster's triangles: each cluster
    is one whole leaf, no ray enters another, and a wave of 64 such rays parks 64 leaves of the intended size.  Nothing here assumes what the
    SAH build does with a cluster: the count is the oracle's, cluster by cluster."""
    s, leaf, sd, osc, rays = clusters
    o, d, tmax, kind, cl = rays
    tab = _cluster_table(s)
    r, _ = osc.trace_closest(o, d, tmax)
    assert (r["prim"] >= 0).all()                      # every ray passes through its cluster
    tested = np.asarray([int(osc.trace_closest(o[i:i + 1], d[i:i + 1], tmax[i:i + 1])[1]["tris_tested"]) for i in range(2 * N_CLUSTERS)])
    assert tested.min() >= 1 and tested.max() <= 8
    if (s, leaf) not in EXACT:
        if s == 0:
            assert len(set(tested.tolist())) >= 4       # the mixed scene: leaves of many sizes in one wave
        else:
            # s <= 3 at the limit of 8: a leaf pools whole neighbouring clusters, more than one of them, and every ray tests one whole leaf
            assert (tested % s == 0).all() and (tested > s).all() and (tested // s * s <= 8).all()
        return
    for c in range(N_CLUSTERS):
        m = cl == c
        _, cnt = osc.trace_closest(o[m], d[m], tmax[m])
        assert int(cnt["tris_tested"]) == int(m.sum()) * tab[c][3], (c, tab[c][3])
    for i in (0, 1, 63, 64, 65, N_POOL - 1):           # and ray by ray, perpendicular and oblique
        _, cnt = osc.trace_closest(o[i:i + 1], d[i:i + 1], tmax[i:i + 1])
        assert int(cnt["tris_tested"]) == tab[cl[i]][3]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 17, 18, 19, 63, 64, 65, 1025])
def test_cluster_rounds_exact(clusters, gpu_ctx, n):
    s, leaf, sd, osc, rays = clusters
    gpu_ctx.upload(sd)
    o, d, tmax, kind = (a[:n] for a in rays[:4])
    _check(gpu_ctx, osc, o, d, tmax, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3])
def test_cluster_rounds_single_kind_exact(clusters, gpu_ctx, k):
    """One block and one lane of rays as one kind: continuation, shadow and probe items."""
    s, leaf, sd, osc, rays = clusters
    gpu_ctx.upload(sd)
    o, d, tmax = (a[:1025] for a in rays[:3])
    n_hit, n_occ = _check(gpu_ctx, osc, o, d, tmax, np.full(1025, k, np.uint8))
    assert (n_hit if k == 1 else n_occ if k == 2 else 1) > 0


@pytest.mark.gpu
def test_second_call_of_the_same_size(clusters, gpu_ctx):
    """Two calls of one size with different rays: a ray of the second call that was left parked and never stored would show the first call's value."""
    s, leaf, sd, osc, rays = clusters
    gpu_ctx.upload(sd)
    n = 1025
    first = tuple(a[:n] for a in rays[:4])
    second = tuple(a[n:2 * n][::-1] for a in rays[:4])
    r1, _ = osc.trace_closest(first[0], first[1], first[2])
    r2, _ = osc.trace_closest(second[0], second[1], second[2])
    assert (r1["prim"] != r2["prim"]).mean() > 0.5          # the two sets do differ, item by item
    _check(gpu_ctx, osc, *first)
    _check(gpu_ctx, osc, *second)
