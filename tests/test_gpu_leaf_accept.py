"""The pooled leaf round's accept test on leaves where it matters.  In a leaf round of k_trace every helper lane compares its
(ray, triangle) result with the owner's t_max as the round starts, one ballot is the round's candidate mask, and the owner only
walks the candidates of its leaf: the first is accepted as it is, every later one is compared again with the t_max the hits
before it have left (exact because tri_accept is monotone in t_max: tests/test_accept_monotone.py).  Random scenes hardly ever
put two triangles that one ray passes through into one leaf, so this scene is made of nothing else.

Stacked sheets: 48 well-separated clusters of 2-8 parallel triangles 0.01 apart, stored near-to-far in half of the clusters and
far-to-near in the other half, half of them with reversed winding (both signs of the determinant), built with leaves of up to 4
and up to 8 triangles.  Rays come from both sides, perpendicular (two infinite reciprocals: the NaN-exact slab form), with one
zero component and oblique, as continuation, shadow and probe items, with t_max infinite, between two sheets, in front of the first
sheet and exactly at the first sheet's t (taken from the oracle).  Every hit, t, barycentric, occlusion flag and the four counters
must equal the oracle's, at batch sizes where the only retire is the final drain (1), around one wave (63, 64, 65) and where lanes
are refilled many times (4 097)."""
import numpy as np
import pytest

from helpers import scenes
from test_gpu_wavefront import _check

GAP = 0.01                     # distance between two sheets of a cluster
N_CLUSTERS = 48
SPACING = 4.0


def _cluster_table():
    """(centre x, centre y, centre z, sheets, stored far-to-near in +z, reversed winding) per cluster."""
    out = []
    for c in range(N_CLUSTERS):
        n = 2 + c % 7                                   # 2..8 sheets
        out.append((SPACING * (c % 8 - 3.5), SPACING * (c // 8 - 2.5), 0.25 * (c % 5), n, (c // 2) % 2 == 1, c % 2 == 1))
    return out


def sheets_scene(leaf):
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
    scenes._quad(b, (1, 30, -1), (1, 30, 1), (-1, 30, 1), (-1, 30, -1))
    b.no_area_light()
    first = []                                          # index of each cluster's first triangle, in submission order
    n_before = 2
    for cx, cy, cz, n, far_first, reverse in _cluster_table():
        zs = cz + GAP * np.arange(n)
        if far_first:
            zs = zs[::-1]
        P, idx = [], []
        for j, z in enumerate(zs):
            P += [(cx - 1.0, cy - 1.0, z), (cx + 1.0, cy - 1.0, z), (cx, cy + 1.2, z)]
            idx += [3 * j, 3 * j + 2, 3 * j + 1] if reverse else [3 * j, 3 * j + 1, 3 * j + 2]
        b.shape_trianglemesh(np.asarray(P, np.float32), idx)
        first.append(n_before)
        n_before += n
    return b.build(), np.asarray(first)


def sheet_rays(osc, seed=5):
    """The ray pool (origins, directions, t_max, kinds) and per ray: its cluster, the side it comes from (+1: travelling towards +z) and
    which of the four t_max classes it has.  Every direction has |dz| = 1, so t is the distance along z."""
    rng = np.random.default_rng(seed)
    tab = _cluster_table()
    o, d, cl, side = [], [], [], []
    for c, (cx, cy, cz, n, far_first, reverse) in enumerate(tab):
        mid = cz + 0.5 * GAP * (n - 1)
        for s in (1.0, -1.0):
            for shape in range(3):
                for _ in range(16):
                    if shape == 0:
                        dx, dy = 0.0, 0.0                                   # perpendicular: two infinite reciprocals
                    elif shape == 1:
                        dx, dy = (rng.uniform(-0.2, 0.2), 0.0) if rng.integers(2) else (0.0, rng.uniform(-0.2, 0.2))
                    else:
                        dx, dy = rng.uniform(-0.2, 0.2, 2)
                    tx, ty = cx + rng.uniform(-0.25, 0.25), cy + rng.uniform(-0.25, 0.25)
                    dist = rng.uniform(3.0, 6.0)
                    d.append((dx, dy, s)); o.append((tx - dx * dist, ty - dy * dist, mid - s * dist))
                    cl.append(c); side.append(s)
    o = np.asarray(o, np.float32); d = np.asarray(d, np.float32)
    cl = np.asarray(cl); side = np.asarray(side)
    n = len(cl)
    r0, _ = osc.trace_closest(o, d, np.full(n, np.inf, np.float32))
    assert (r0["prim"] >= 0).all()                     # every ray passes through its cluster
    t_first = r0["t"].astype(np.float32)               # the first sheet's t: exactly what a hit there reports
    tclass = rng.integers(0, 4, n)
    nsheets = np.asarray([tab[c][3] for c in cl])
    between = t_first + np.float32(GAP) * (rng.integers(1, 8, n) % np.maximum(nsheets - 1, 1) + 0.5).astype(np.float32)
    tmax = np.where(tclass == 0, np.float32(np.inf),
                    np.where(tclass == 1, between, np.where(tclass == 2, t_first - np.float32(0.5 * GAP), t_first))).astype(np.float32)
    kind = np.asarray([1, 2, 3], np.uint8)[rng.integers(0, 3, n)]
    perm = rng.permutation(n)
    return o[perm], d[perm], tmax[perm], kind[perm], cl[perm], side[perm], tclass[perm]


def check_not_empty(osc, first, rays):
    """What makes this scene a test of the candidate walk, from the oracle alone: closest-hit rays that meet a cluster far sheet first
    in storage order end on its LAST stored sheet (several successive accepts if the sheets share a leaf), and any-hit rays stop early."""
    o, d, tmax, kind, cl, side, tclass = rays
    tab = _cluster_table()
    far_first_z = np.asarray([t[4] for t in tab])[cl]
    nsheets = np.asarray([t[3] for t in tab])[cl]
    # stored far-to-near AS THE RAY SEES IT: far-to-near in +z and travelling towards +z, or near-to-far in +z and travelling towards -z
    far_to_near = far_first_z == (side > 0)
    m = far_to_near & (kind != 2)
    r, _ = osc.trace_closest(o[m], d[m], tmax[m])
    last = (first[cl] + nsheets - 1)[m]
    share = float((r["prim"] == last).mean())
    a = (kind == 2) & (tclass == 0)
    occ, cnt = osc.trace_any(o[a], d[a], tmax[a])
    return share, int(cnt["tris_tested"]), int(nsheets[a].sum()), int(occ.sum()), int(a.sum())


@pytest.fixture(scope="module", params=[4, 8])
def sheets(request, oracle):
    sd, first = sheets_scene(request.param)
    osc = oracle.scene(sd)
    rays = sheet_rays(osc)
    yield sd, first, osc, rays
    osc.close()


def test_oracle_alone_meets_the_conditions(sheets):
    """(no GPU) The scene does what it is for: see check_not_empty."""
    sd, first, osc, rays = sheets
    assert len(rays[3]) >= 4097
    share, tested, whole, n_occ, n_any = check_not_empty(osc, first, rays)
    print("last stored sheet reported by %.3f of the far-to-near closest-hit rays; any-hit: %d tests against %d for whole clusters" % (share, tested, whole))
    assert share >= 0.1
    assert n_occ == n_any and tested < whole


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_stacked_sheets_exact(sheets, gpu_ctx, n):
    sd, first, osc, rays = sheets
    gpu_ctx.upload(sd)
    o, d, tmax, kind = (a[:n] for a in rays[:4])
    _check(gpu_ctx, osc, o, d, tmax, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3])
def test_stacked_sheets_single_kind_exact(sheets, gpu_ctx, k):
    """All rays of the pool as one kind: every t_max class and direction shape as a closest-hit, an any-hit and a probe item."""
    sd, first, osc, rays = sheets
    gpu_ctx.upload(sd)
    o, d, tmax = rays[:3]
    n_hit, n_occ = _check(gpu_ctx, osc, o, d, tmax, np.full(len(tmax), k, np.uint8))
    if k == 1:
        assert n_hit > 0
    if k == 2:
        assert n_occ > 0
