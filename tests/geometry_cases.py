"""The cases of the geometry truth (tests/geometry_ref.py) and what is asserted on them -- shared by test_geometry_truth_oracle.py, which
holds the oracle to the truth without a GPU, and test_gpu_geometry_truth.py, which holds the device to it without the oracle.

Ray cases: 8 191 rays (not a multiple of 64) per scene -- a third camera rays, a third helpers.random_rays, a third shadow_like
segments, shuffled; 192 of them start on a triangle (unshifted spawns), and the sphere scene swaps another 512 for rays aimed at
the clipped sphere's rims.  Every case reaches another
traversal kernel (the table in test_gpu_geometry_truth.py).  Light cases: (scene, light, reference point) with a 64 x 64 grid of
stratum midpoints plus the corners of [0, 1 - 2^-24]^2."""
import numpy as np

import feature_scenes as fs
import geometry_ref as G
from helpers import random_rays, scenes
from test_texture_oracle import MAX_LEFT_OUT

N_RAYS = 8191
N_RIM = 512
N_SURFACE = 192
# The reference's delta_t is 10-200 times wider than the real error, so a bias of a few percent of it would pass |err| <= bound
# on every ray; the median of err / bound must stay below 4 x the largest median the oracle shows on these cases, 0.0062
# (spheres; 0.0041-0.0048 on the others: profiles/geometry_truth.txt).
MEDIAN_LIMIT = 4 * 0.0062

# name -> (scene, key of the geometry (cases of one key share a truth), environment of the device context)
RAY_CASES = {
    "cornell": (lambda: scenes.cornell_box(res=64, spp=16), "cornell", {}),
    "rt4k_sah_leaf4": (lambda: fs.scene_accel("sah", 4), "rt4k", {}),
    "rt4k_hlbvh_leaf2": (lambda: fs.scene_accel("hlbvh", 2), "rt4k", {}),
    "rt4k_sah_leaf12": (lambda: fs.scene_accel("sah", 12), "rt4k", {}),
    "spheres": (lambda: fs.scene_spheres(), "spheres", {}),
    "instances": (lambda: fs.scene_instances(), "instances", {}),
    "rt4k_sah_leaf4_far": (lambda: fs.scene_accel("sah", 4), "rt4k", {"PBRTGPU_TRACE_FAR": "1"}),
}


def _rim_rays(sd, info, n, rng):
    """Rays aimed at the clipped sphere's rims: the circles z = zmin and z = zmax, the meridians phi = phimax and phi = 0 and the
    pole axis, each target moved off its rim by 1e-7 ... 1e-2 (log-uniform) of the radius."""
    sph = [sd.buffers["spheres"][i] for i in range(sd.desc.n_spheres)]
    sp = next(s for s in sph if s.zmin > -s.radius or s.zmax < s.radius)
    m = np.array(list(sp.object_to_world), np.float64).reshape(4, 4)
    r, phimax = sp.radius, np.radians(sp.phimax)
    which = rng.integers(0, 5, n)
    z = np.where(which == 0, sp.zmin, np.where(which == 1, sp.zmax, rng.uniform(sp.zmin, sp.zmax, n)))
    phi = np.where(which == 2, phimax, np.where(which == 3, 0.0, rng.uniform(0.0, 2 * np.pi, n)))
    rho = np.sqrt(np.maximum(0.0, r * r - z * z))
    p = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1)
    p[which == 4] = np.stack([np.zeros((which == 4).sum()), np.zeros((which == 4).sum()), rng.uniform(-r, r, (which == 4).sum())], 1)
    p += rng.standard_normal((n, 3)) * (r * np.exp(rng.uniform(np.log(1e-7), np.log(1e-2), (n, 1))))
    target = p @ m[:3, :3].T + m[:3, 3]
    wb = np.array(list(info.world_bound), np.float64)
    o = wb[:3] + rng.random((n, 3)) * (wb[3:] - wb[:3])
    d = (target - o) * np.exp(rng.uniform(-1, 1, (n, 1)))
    tmax = np.where(rng.random(n) < 0.5, np.inf, np.exp(rng.uniform(-0.5, 0.5, n)) / np.exp(rng.uniform(-1, 1, n)))
    return o.astype(np.float32), d.astype(np.float32), tmax.astype(np.float32)


def _surface_rays(sd, n, rng):
    """Rays that start ON a world triangle, as a renderer's unshifted spawn would: the float32 point b0 p0 + b1 p1 + b2 p2, any
    direction.  Their own triangle lies at |t64| ~ 1e-8, far inside delta_t: the reference's `t <= delta_t` is what rejects it."""
    P = np.asarray(sd.buffers["P"], np.float32).reshape(-1, 3)
    idx = np.asarray(sd.buffers["indices"]).reshape(-1, 3)
    tm = np.asarray(sd.buffers["tri_mesh"]).reshape(-1)
    world = np.nonzero(np.array([sd.buffers["meshes"][int(m)].object == 0 for m in tm]))[0]
    tri = world[rng.integers(0, len(world), n)]
    b = rng.uniform(0.15, 0.35, (n, 2)).astype(np.float32)
    b2 = np.float32(1.0) - b[:, 0] - b[:, 1]
    o = b[:, :1] * P[idx[tri, 0]] + b[:, 1:] * P[idx[tri, 1]] + b2[:, None] * P[idx[tri, 2]]
    d = rng.standard_normal((n, 3)).astype(np.float32)
    return o.astype(np.float32), d, np.full(n, np.inf, np.float32)


def make_rays(name, sd, info, camera_rays, seed=5):
    """(o, d, t_max, kind) of a case.  camera_rays(pixel_xy, sample_index) -> (o, d, ...): the device's or the oracle's generator
    (the truth takes whatever rays it is given)."""
    rng = np.random.default_rng(seed)
    n = N_RAYS - N_SURFACE - (N_RIM if name == "spheres" else 0)
    sb = list(info.sample_bounds)
    n_cam = n // 3
    px = np.stack([rng.integers(sb[0], sb[2], n_cam), rng.integers(sb[1], sb[3], n_cam)], 1).astype(np.int32)
    si = rng.integers(0, max(1, info.spp), n_cam).astype(np.uint32)
    cam = camera_rays(px, si)
    n_rand = (n - n_cam) // 2
    ro, rd, rt = random_rays(info, n_rand, seed)
    so, sd_, st = random_rays(info, n - n_cam - n_rand, seed + 1, shadow_like=True)
    parts_o, parts_d, parts_t = [cam[0], ro, so], [cam[1], rd, sd_], [np.full(n_cam, np.inf, np.float32), rt, st]
    xo, xd, xt = _surface_rays(sd, N_SURFACE, rng)
    parts_o.append(xo); parts_d.append(xd); parts_t.append(xt)
    if name == "spheres":
        xo, xd, xt = _rim_rays(sd, info, N_RIM, rng)
        parts_o.append(xo); parts_d.append(xd); parts_t.append(xt)
    o, d, t = np.concatenate(parts_o), np.concatenate(parts_d), np.concatenate(parts_t)
    perm = rng.permutation(N_RAYS)
    kind = np.asarray([1, 2, 3], np.uint8)[rng.integers(0, 3, N_RAYS)]
    return np.ascontiguousarray(o[perm], np.float32), np.ascontiguousarray(d[perm], np.float32), np.ascontiguousarray(t[perm], np.float32), kind


_truths = {}


def truth_of(key, sd, rays):
    """The float64 truth of a geometry and a ray set, computed once per process."""
    k = (key, rays[0].tobytes(), rays[1].tobytes(), rays[2].tobytes())
    if k not in _truths:
        _truths[k] = G.closest_hits(G.Scene(sd), rays[0], rays[1], rays[2])
        for a in _truths[k].values():
            a.setflags(write=False)
    return _truths[k]


def hold_hits(label, tr, sel, hits, inst=False, probe=False):
    """Closest hits `hits` (pt_hit records) of the rays tr[..][sel] against the truth.  inst: t and hit / miss only (the hooks report
    no barycentrics and an inner primitive inside an instance).  probe: hit / miss and the primitive only.  Returns the err / bound
    ratios of t."""
    rule, kind = tr["rule"][sel], tr["kind"][sel]
    dec = rule == 0
    dev_hit = hits["prim"] >= 0
    wrong = dec & (dev_hit != (kind > 0))
    assert not wrong.any(), "%s: hit / miss differs on %d decisive rays, first %s" % (label, wrong.sum(), np.nonzero(sel)[0][wrong][:5] if sel.dtype == bool else wrong.nonzero()[0][:5])
    both = dec & dev_hit
    if not inst:
        wrong = both & (hits["prim"] != tr["prim"][sel])
        assert not wrong.any(), "%s: primitive differs on %d decisive rays" % (label, wrong.sum())
    t = hits["t"].astype(np.float64)
    # rule (b) must not swallow a wrong primitive: the ray does hit, and t is within bound of one of the tied hits
    tied = rule == 2
    if tied.any():
        assert dev_hit[tied].all(), "%s: a ray with two tied hits missed" % label
        if not probe:
            e1 = np.abs(t - tr["t"][sel]) <= tr["bound"][sel]
            e2 = np.abs(t - tr["tied_t"][sel]) <= tr["tied_bound"][sel]
            assert (e1 | e2)[tied].all(), "%s: t of a tied ray is within bound of neither hit" % label
    if probe:
        return np.zeros(0)
    with np.errstate(all="ignore"):
        ratio = (np.abs(t - tr["t"][sel]) / tr["bound"][sel])[both]
    assert (ratio <= 1.0).all(), "%s: |t - t64| exceeds its bound, worst ratio %.3f" % (label, ratio.max())
    if not inst:
        tri = both & (kind == G.TRIANGLE)
        for f in ("b0", "b1"):
            with np.errstate(all="ignore"):
                rb = (np.abs(hits[f].astype(np.float64) - tr[f][sel]) / tr["bound_b"][sel])[tri]
            assert (rb <= 1.0).all(), "%s: %s exceeds its bound, worst ratio %.3f" % (label, f, rb.max())
    return ratio


def hold_occlusion(label, tr, sel, occ):
    dec = tr["rule"][sel] == 0
    wrong = dec & (occ.astype(bool) != tr["occluded"][sel])
    assert not wrong.any(), "%s: occlusion flag differs on %d decisive rays" % (label, wrong.sum())


def report(label, tr, ratio):
    """The case's line: left-out share (by rule), worst and median err / bound; asserts the share and the median."""
    left = float((tr["rule"] != 0).mean())
    by = np.bincount(tr["rule"], minlength=5)
    worst, med = (float(ratio.max()), float(np.median(ratio))) if len(ratio) else (0.0, 0.0)
    line = "%-28s left out %.2f %% (a %d, b %d, c %d, d %d of %d)  err/bound worst %.3f median %.4f  (%d hits)" % (
        label, 100 * left, by[1], by[2], by[3], by[4], len(tr["rule"]), worst, med, len(ratio))
    print(line)
    assert left <= MAX_LEFT_OUT, "%s: %.2f %% left out" % (label, 100 * left)
    assert len(ratio) >= 1000, "%s: only %d hits compared" % (label, len(ratio))
    assert med <= MEDIAN_LIMIT, "%s: median err / bound %.4f above %.4f" % (label, med, MEDIAN_LIMIT)
    return line


# --------------------------------------------------------------------------------------------------------------------- lights
LIGHT_SCENES = {"cornell": lambda: scenes.cornell_box(res=64, spp=16), "spheres_lights": lambda: fs.scene_spheres(lights_only=True)}
# (scene, reference point, what it is for).  Every light of the scene is sampled from every point of its scene.
LIGHT_POINTS = [
    ("cornell", (278.0, 273.0, 100.0), "inside the room"),
    ("cornell", (100.0, 30.0, 400.0), "inside the room, oblique"),
    ("spheres_lights", (0.3, -0.5, -0.2), "inside the room"),
    ("spheres_lights", (1.3, 0.95, 0.85), "inside the two-sided light sphere"),
    ("spheres_lights", (-1.2, 1.0, 0.5), "inside the scaled light sphere's world sphere"),
    ("spheres_lights", (9.0, -6.0, -30.0), "far: the small sphere's cone takes the small-angle branch"),
    ("spheres_lights", (0.5, -40.0, 3.0), "far: both spheres' cones take the small-angle branch"),
]
COS_MARGIN = 1e-3            # |cos| at the light below this: facing, and with it None / Li, is not decided (and pdf ~ 1 / cos)


def light_cases():
    out = []
    for scene, p, what in LIGHT_POINTS:
        n = 2 if scene == "cornell" else 4
        out += [(scene, light, p) for light in range(n)]
    return out


def light_id(c):
    return "%s-light%d-%s" % (c[0], c[1], "_".join("%g" % v for v in c[2]))


def hold_light(label, tr, li, wi, pdf, ref_p):
    """One light from one point over the grid: unit wi, the ray along wi through the truth's point, pdf and Li within their bounds,
    pdf == 0 exactly where the truth returns None.  Returns the printed line."""
    w = wi.astype(np.float64)
    dec = np.abs(tr["cos"]) > COS_MARGIN
    left = float((~dec).mean())
    v = tr["valid"]
    assert ((pdf == 0) == ~v)[dec].all(), "%s: None differs on %d decisive samples" % (label, ((pdf == 0) != ~v)[dec].sum())
    ok = dec & v
    norm = np.sqrt((w * w).sum(1))[ok]
    assert (np.abs(norm - 1.0) <= 4 * 2.0 ** -23).all(), "%s: |wi| off by %.3g" % (label, np.abs(norm - 1.0).max())
    # the truth's point lies on the line ref + s wi, s > 0: within the float32 point's bound, the rounding of p - ref (half an ulp
    # of each component) and of the normalisation (gamma(4) per component), together below gamma(10) of the distance
    pp = tr["p"] - np.asarray(ref_p, np.float32).astype(np.float64)
    s = (pp * w).sum(1)
    off = np.linalg.norm(pp - s[:, None] * w, axis=1)
    line_bound = tr["p_bound"] + G.gamma(10) * tr["dist"]
    r_line = (off / line_bound)[ok]
    assert (s[ok] > 0).all() and (r_line <= 1.0).all(), "%s: the ray along wi passes the truth's point at %.3f of its bound" % (label, r_line.max())
    r_pdf = (np.abs(pdf.astype(np.float64) / np.where(v, tr["pdf"], 1.0) - 1.0) / tr["pdf_rel"])[ok]
    assert (r_pdf <= 1.0).all(), "%s: pdf off by %.3f of its bound" % (label, r_pdf.max())
    assert np.array_equal(li.astype(np.float64)[ok], tr["li"][ok]), "%s: Li differs" % label
    line = "%-58s %-10s left out %.2f %%  None %.2f %%  pdf err/bound worst %.3f  point err/bound worst %.3f" % (
        label, "/".join(sorted(set(tr["branch"]))), 100 * left, 100 * float((~v).mean()), r_pdf.max() if len(r_pdf) else 0.0, r_line.max() if len(r_line) else 0.0)
    print(line)
    assert left <= MAX_LEFT_OUT, "%s: %.2f %% left out" % (label, 100 * left)
    return line


# mean(1 / pdf) over the grid is the solid angle the light subtends.  The tolerance is the discretisation error of the grid itself,
# taken from the float64 restatement: twice its discrepancy at 64 x 64.  For the Cornell triangle 34 from (278, 273, 100) the
# analytic value is 0.04766595, the grid mean is off by 2.03e-6 at 64^2 and by 7.27e-7 at 128^2 (the square root in
# uniform_sample_triangle keeps the midpoint rule from quartering), and the oracle's float32 mean by 2.03e-6.  A cone's density is constant, its discrepancy zero, and what is
# left is the float32 density's own error, so there the tolerance is the largest relative bound of pdf times the solid angle.
SOLID_ANGLE_CASES = [("cornell", 0, (278.0, 273.0, 100.0)), ("cornell", 1, (100.0, 30.0, 400.0)), ("spheres_lights", 1, (0.3, -0.5, -0.2)),
                     ("spheres_lights", 3, (0.3, -0.5, -0.2)), ("spheres_lights", 0, (1.3, 0.95, 0.85))]


def hold_solid_angle(label, sc, light, ref_p, sample):
    """sample(u) -> pdf of the code under test."""
    u = G.stratum_grid(64)[:4096]
    tr = G.light_truth(sc, light, ref_p, u)
    omega = float(tr["solid_angle"][0])
    assert tr["valid"].all() and np.isfinite(omega)
    d64 = abs(float(np.mean(1.0 / tr["pdf"])) - omega)
    g128 = (np.arange(128) + 0.5) / 128
    u128 = np.stack(np.meshgrid(g128, g128, indexing="ij"), -1).reshape(-1, 2)
    tr128 = G.light_truth(sc, light, ref_p, u128)
    d128 = abs(float(np.mean(1.0 / tr128["pdf"])) - omega)
    tol = 2.0 * d64 if tr["branch"][0] == "triangle" else 2.0 * d64 + omega * float(tr["pdf_rel"].max())
    pdf = sample(u)
    got = float(np.mean(1.0 / pdf.astype(np.float64)))
    line = "%-58s solid angle %.8f  mean(1/pdf) %.8f  off %.3g  tolerance %.3g  (float64 grid: 64^2 off %.3g, 128^2 off %.3g)" % (
        label, omega, got, abs(got - omega), tol, d64, d128)
    print(line)
    assert (pdf > 0).all()
    assert abs(got - omega) <= tol, line
    return line
