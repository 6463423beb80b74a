"""The oracle's geometric results (trace_closest, trace_any, light_sample_li) held to the float64 truths of geometry_ref.py, on exactly
the cases test_gpu_geometry_truth.py puts to the device -- so the bounds and the left-out shares are proven here, without a GPU, before
a GPU sees them.  Plus the truth's own self-tests: hand values, an analytic solid angle, invariance under a permutation of the
primitive list.

Per case the printed line gives the left-out share, the worst and the median err / bound (recorded in profiles/geometry_truth.txt)."""
import numpy as np
import pytest

import geometry_cases as GC
import geometry_ref as G
from helpers import scenes


# ------------------------------------------------------------------------------------------------------------- self-tests
def _tiny_scene(fill):
    b = scenes.SceneBuilder()
    b.look_at((0, 0, -5), (0, 0, 0), (0, 1, 0)); b.camera_perspective(fov=40.0)
    b.film(xresolution=16, yresolution=16); b.pixel_filter_box(); b.sampler_sobol(1); b.integrator_path(maxdepth=1)
    b.material_matte((0.5, 0.5, 0.5))
    fill(b)
    return b.build()


def test_truth_hand_values():
    """One axis-aligned ray on one triangle, one on a unit sphere."""
    sd = _tiny_scene(lambda b: b.shape_trianglemesh([(0, 0, 1), (1, 0, 1), (0, 1, 1)], [0, 1, 2]))
    tr = G.closest_hits(sd, [(0.25, 0.25, 0.0), (0.25, 0.25, 0.0), (0.75, 0.75, 0.0), (0.25, 0.25, 2.0)], [(0, 0, 1), (0, 0, 2), (0, 0, 1), (0, 0, 1)],
                        [np.inf, np.inf, np.inf, np.inf])
    assert list(tr["kind"]) == [G.TRIANGLE, G.TRIANGLE, G.MISS, G.MISS] and list(tr["prim"][:2]) == [0, 0]
    assert np.array_equal(tr["t"][:2], [1.0, 0.5]) and np.array_equal(tr["b0"][:2], [0.5, 0.5]) and np.array_equal(tr["b1"][:2], [0.25, 0.25])
    assert list(tr["occluded"]) == [True, True, False, False] and not tr["rule"].any()
    assert 0 < tr["bound"][0] < 1e-5 and 0 < tr["bound_b"][0] < 1e-5
    # t_max before, behind and on the hit; a ray through an edge
    tr = G.closest_hits(sd, [(0.25, 0.25, 0.0)] * 3 + [(0.5, 0.5, 0.0)], [(0, 0, 1)] * 4, [0.5, 2.0, 1.0, np.inf])
    assert list(tr["kind"][:2]) == [G.MISS, G.TRIANGLE] and [G.RULES[r] for r in tr["rule"]] == ["", "", "c", "a"]
    sd = _tiny_scene(lambda b: b.shape_sphere(radius=1.0))
    tr = G.closest_hits(sd, [(0.0, 0.0, -3.0), (0.0, 0.0, 0.0), (0.0, 0.0, -3.0), (2.0, 0.0, -3.0)], [(0, 0, 1)] * 4, [np.inf, np.inf, 1.5, np.inf])
    assert list(tr["kind"]) == [G.SPHERE, G.SPHERE, G.MISS, G.MISS] and not tr["rule"].any()
    assert np.allclose(tr["t"][:2], [2.0, 1.0], rtol=0, atol=1e-15) and list(tr["occluded"]) == [True, True, False, False]
    assert 0 < tr["bound"][0] < 1e-5
    # the silhouette and the surface itself are not decided
    tr = G.closest_hits(sd, [(1.0, 0.0, -3.0), (0.0, 0.0, -1.0)], [(0, 0, 1)] * 2, [np.inf] * 2)
    assert [G.RULES[r] for r in tr["rule"]] == ["a", "c"]


def test_truth_clipped_sphere_and_second_root():
    """z and phi clips; the far side seen through the cut, where intersect wraps phi by PI and intersect_p by 2 PI (Q58)."""
    sd = _tiny_scene(lambda b: b.shape_sphere(radius=1.0, zmin=-0.5, zmax=0.5, phimax=270.0))
    o = [(-3.0, 0.3, 0.0), (-3.0, 0.3, 0.8), (0.5, -3.0, 0.0), (3.0, -0.5, 0.0)]
    d = [(1, 0, 0), (1, 0, 0), (0, 1, 0), (-1, 0, 0)]
    tr = G.closest_hits(sd, o, d, [np.inf] * 4)
    x = np.sqrt(1 - float(np.float32(0.3)) ** 2)
    # 0: near side at phi ~ 163 deg.  1: above zmax both ways.  2: enters through the cut (phi ~ 300 deg), leaves at phi ~ 60 deg.
    # 3: near side in the cut (phi = 330 deg), far side at phi = 210 deg: raw phi < 0 -> +PI = 30 deg in intersect, 210 in intersect_p
    assert list(tr["kind"]) == [G.SPHERE, G.MISS, G.SPHERE, G.SPHERE]
    assert np.allclose(tr["t"][[0, 2, 3]], [3 - x, 3 + np.sqrt(0.75), 3 + np.sqrt(0.75)], rtol=0, atol=1e-14)
    assert list(tr["occluded"]) == [True, False, True, True] and not tr["rule"].any()
    # a chord inside the cut, from phi = 340 deg to phi = 290 deg: intersect accepts the far side (-70 + 180 = 110 <= 270), intersect_p does not
    p1, p2 = np.array([np.cos(np.radians(-20.0)), np.sin(np.radians(-20.0)), 0.0]), np.array([np.cos(np.radians(-70.0)), np.sin(np.radians(-70.0)), 0.0])
    tr = G.closest_hits(sd, [p1 - 2 * (p2 - p1)], [p2 - p1], [np.inf])
    assert tr["kind"][0] == G.SPHERE and abs(tr["t"][0] - 3.0) < 1e-6 and not tr["occluded"][0] and tr["rule"][0] == 0


def test_truth_octant_subtends_half_pi():
    e = np.eye(3)
    assert abs(G.triangle_solid_angle(np.zeros(3), e[0], e[1], e[2]) - np.pi / 2) < 1e-15
    assert abs(G.triangle_solid_angle(np.zeros(3), 5 * e[0], 0.1 * e[1], 3 * e[2]) - np.pi / 2) < 1e-15


def test_truth_is_invariant_under_a_permutation_of_the_primitives():
    sd = scenes.cornell_box(res=16, spp=1)
    from helpers import random_rays

    class Info:
        world_bound = [0.0, 0.0, 0.0, 556.0, 548.8, 559.2]
    o, d, t = random_rays(Info, 2000, 9)
    a = G.Scene(sd)
    ta = G.closest_hits(a, o, d, t)
    b = G.Scene(sd)
    perm = np.random.default_rng(3).permutation(len(b.idx))
    b.idx, b.tri_flags, b.tri_object, b.tri_light, b.tri_prim = b.idx[perm], b.tri_flags[perm], b.tri_object[perm], b.tri_light[perm], b.tri_prim[perm]
    b.groups = [([], np.arange(len(b.idx)), [], None)]
    tb = G.closest_hits(b, o, d, t)
    assert (ta["kind"] > 0).sum() > 500
    for k in ("kind", "t", "occluded", "rule", "tied_t"):
        assert np.array_equal(ta[k], tb[k]), k
    dec = ta["rule"] == 0
    for k in ("prim", "b0", "b1", "bound", "bound_b"):            # (which of two exactly tied faces comes first is the list's order)
        assert np.array_equal(ta[k][dec], tb[k][dec]), k


# ------------------------------------------------------------------------------------------------------ the oracle: rays
@pytest.mark.parametrize("name", list(GC.RAY_CASES))
def test_oracle_rays_against_truth(oracle, name):
    make, key, _ = GC.RAY_CASES[name]
    sd = make()
    osc = oracle.scene(sd)
    rays = GC.make_rays(name, sd, osc.info, osc.generate_camera_rays)
    o, d, t, kind = rays
    tr = GC.truth_of(key, sd, rays)
    every = np.ones(len(t), bool)
    inst = name == "instances"
    hits, _ = osc.trace_closest(o, d, t)
    occ, _ = osc.trace_any(o, d, t)
    osc.close()
    ratio = GC.hold_hits(name, tr, every, hits, inst=inst)
    GC.hold_occlusion(name, tr, every, occ)
    GC.report("oracle " + name, tr, ratio)
    assert (tr["occluded"] & (tr["rule"] == 0)).sum() >= 1000
    if name == "spheres":          # the rim rays do what they are for: rule (d) fires, and decisive rays end on the clipped sphere's far side
        assert (tr["rule"] == 4).sum() >= 20 and ((tr["kind"] == G.SPHERE) & (tr["rule"] == 0)).sum() >= 500


# ---------------------------------------------------------------------------------------------------- the oracle: lights
@pytest.fixture(scope="module")
def light_scenes(oracle):
    out = {}
    for k, make in GC.LIGHT_SCENES.items():
        sd = make()
        out[k] = (sd, G.Scene(sd), oracle.scene(sd))
    yield out
    for sd, sc, osc in out.values():
        osc.close()


@pytest.mark.parametrize("case", GC.light_cases(), ids=GC.light_id)
def test_oracle_light_samples_against_truth(light_scenes, case):
    scene, light, p = case
    sd, sc, osc = light_scenes[scene]
    u = G.stratum_grid(64)
    tr = G.light_truth(sc, light, p, u)
    li, wi, pdf = osc.light_sample_li(light, np.float32(p), u)
    GC.hold_light("oracle " + GC.light_id(case), tr, li, wi, pdf, p)


def test_light_cases_reach_every_branch(light_scenes):
    seen = set()
    for scene, light, p in GC.light_cases():
        tr = G.light_truth(light_scenes[scene][1], light, p, G.stratum_grid(4))
        seen |= set(tr["branch"])
        sc = light_scenes[scene][1]
        kind, idx = sc.lights()[light][:2]
        if kind == G.TRIANGLE:                    # the truth's points lie on the light's shape: inside the triangle's plane and edges ...
            p0, p1, p2 = (sc.P[sc.idx[idx, k]] for k in range(3))
            bary = np.linalg.lstsq(np.stack([p0 - p2, p1 - p2], 1), (tr["p"] - p2).T, rcond=None)
            assert (bary[0] >= -1e-12).all() and (bary[0].sum(0) <= 1 + 1e-12).all() and np.abs(np.stack([p0 - p2, p1 - p2], 1) @ bary[0] - (tr["p"] - p2).T).max() < 1e-9
        else:                                     # ... on the sphere in object space (inside), on the world sphere around the centre (outside, Q59)
            sp = sc.spheres[idx]
            po = tr["p"] @ sp.w2o[:3, :3].T + sp.w2o[:3, 3]
            on = np.where(tr["branch"] == "inside", np.linalg.norm(po, axis=1), np.linalg.norm(tr["p"] - sp.o2w[:3, 3], axis=1))
            assert np.abs(on / sp.r - 1.0).max() < 1e-6          # (the stored inverse is a float32 matrix: not the exact inverse)
        if tr["branch"][0] != "triangle":         # away from the inside test's and the small-angle branch's thresholds
            sp = light_scenes[scene][1].spheres[light_scenes[scene][1].lights()[light][1]]
            dc2 = ((np.float32(p).astype(np.float64) - sp.o2w[:3, 3]) ** 2).sum()
            assert abs(dc2 / sp.r ** 2 - 1.0) > 1e-2 and abs(sp.r ** 2 / dc2 - 0.00068523) > 1e-5
    assert seen == {"triangle", "inside", "cone", "cone_small"}


@pytest.mark.parametrize("case", GC.SOLID_ANGLE_CASES, ids=GC.light_id)
def test_oracle_mean_inverse_pdf_is_the_solid_angle(light_scenes, case):
    """Tolerance: twice the float64 restatement's own 64 x 64 discrepancy.  Cornell triangle 34 from (278, 273, 100): analytic 0.04766595,
    the float64 grid off by 2.03e-6 at 64^2 and 7.27e-7 at 128^2, the oracle's mean(1 / pdf) 0.04766392 (off 2.03e-6, tolerance 4.06e-6).
    A cone's constant density has no discrepancy: there the pdf's derived float32 bound is added (geometry_cases.hold_solid_angle)."""
    scene, light, p = case
    sd, sc, osc = light_scenes[scene]
    GC.hold_solid_angle("oracle " + GC.light_id(case), sc, light, p, lambda u: osc.light_sample_li(light, np.float32(p), u)[2])
