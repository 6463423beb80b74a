"""The cases of the cylinder / disk truth (tests/quadric_ref.py): scenes, rays and lights, shared by test_quadric_host.py (the float32
restatement against the truth, no GPU) and test_gpu_quadric_truth.py (the device against the truth).  What is asserted on a case is
geometry_cases.hold_hits / hold_occlusion / hold_light: the same rules as for triangles and spheres.

Ray cases: 8 191 rays per scene -- camera rays, helpers.random_rays and shadow-like segments in equal parts, shuffled, of which 512 are
aimed at the rims (each target moved off its rim by 1e-7 ... 1e-2 of the radius, log-uniform), 128 start on a shape's surface or inside a
cylinder, and in the axis-aligned scene 128 run exactly parallel to a cylinder's axis or exactly in a disk's plane."""
import numpy as np

import feature_scenes as fs
import geometry_ref as G
import quadric_ref as Q
from helpers import random_rays, scenes

N_RAYS = 8191
N_RIM = 512
N_SURFACE = 128
N_PARALLEL = 128
# The reference's interval, and the first-order bound the truth derives, are many times wider than the real error, so a bias of a few
# per cent of the bound would pass |err| <= bound on every ray.  The median of err / bound over a case's cylinder hits must stay below
# 4 x the median the float32 restatement of cylinder.rs shows on that case's geometry (profiles/quadric_truth.txt;
# test_quadric_host.py holds the restatement to the figure) -- the factor and the reason of geometry_cases.MEDIAN_LIMIT.
RESTATEMENT_MEDIAN = {"world": 0.0846, "axis": 0.1306}          # (rounded up to four digits)
MEDIAN_LIMIT = {k: 4 * v for k, v in RESTATEMENT_MEDIAN.items()}
T = scenes


def _shapes(b, instanced=False):
    """Cylinders and disks rotated, non-uniformly scaled, mirrored and clipped, with different materials."""
    b.material_matte((0.3, 0.4, 0.8), sigma=20.0)
    t = T.transform_mul(T.transform_translate(-0.9, -1.2, 0.6), T.transform_rotate_x(-90.0))
    b.shape_cylinder(radius=0.45, zmin=-0.8, zmax=0.7, object_to_world=t[0], world_to_object=t[1])                  # an upright pillar
    b.material_plastic()
    t = T.transform_mul(T.transform_translate(0.9, -0.3, -0.2), T.transform_mul(T.transform_rotate_x(35.0), T.transform_scale(0.5, 0.3, 0.9)))
    b.shape_cylinder(radius=1.0, zmin=0.6, zmax=-0.9, phimax=250.0, object_to_world=t[0], world_to_object=t[1])     # clipped in phi, zmin > zmax
    b.material_mirror()
    t = T.transform_mul(T.transform_translate(-0.2, 0.7, 0.9), T.transform_mul(T.transform_rotate_x(-60.0), T.transform_scale(0.6, -0.6, 0.6)))
    b.shape_cylinder(radius=0.7, zmin=-0.5, zmax=0.5, phimax=300.0, object_to_world=t[0], world_to_object=t[1])     # mirrored
    b.material_matte((0.8, 0.7, 0.2))
    t = T.transform_mul(T.transform_translate(0.2, -1.6, -0.6), T.transform_rotate_x(-90.0))
    b.shape_disk(height=0.1, radius=0.8, object_to_world=t[0], world_to_object=t[1])                                # a plate above the floor
    b.material_matte((0.7, 0.3, 0.6))
    t = T.transform_mul(T.transform_translate(-1.0, 0.9, -0.3), T.transform_mul(T.transform_rotate_x(40.0), T.transform_scale(0.8, 0.5, 1.0)))
    b.shape_disk(height=-0.2, radius=0.9, innerradius=0.35, phimax=290.0, object_to_world=t[0], world_to_object=t[1])  # an annulus sector
    if not instanced:
        b.reverse_orientation = True
        t = T.transform_mul(T.transform_translate(1.2, 1.1, 0.8), T.transform_scale(-0.5, 0.5, 0.5))
        b.shape_disk(height=0.0, radius=1.0, innerradius=0.2, object_to_world=t[0], world_to_object=t[1])           # mirrored and reversed
        b.reverse_orientation = False


def scene_world(split="sah", leaf=4, res=40, spp=8):
    """The shapes in the world list among the room's triangles, an emissive disk ahead of every triangle and an emissive cylinder after."""
    b = fs.base(res=res, spp=spp)
    b.accelerator_bvh(splitmethod=split, maxnodeprims=leaf)
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=(12, 11, 9))
    t = T.transform_mul(T.transform_translate(0.4, 1.7, 0.3), T.transform_rotate_x(90.0))
    b.shape_disk(height=0.0, radius=0.35, object_to_world=t[0], world_to_object=t[1])
    b.no_area_light()
    fs.room(b, light_L=(4, 4, 4))
    _shapes(b)
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=(6, 8, 12), twosided=True)
    t = T.transform_mul(T.transform_translate(-1.4, -0.2, -0.9), T.transform_rotate_x(-90.0))
    b.shape_cylinder(radius=0.12, zmin=-0.5, zmax=0.5, object_to_world=t[0], world_to_object=t[1])
    b.no_area_light()
    return b.build()


def scene_instanced(res=40, spp=8):
    """The shapes inside an object, instanced three times (translated; rotated and non-uniformly scaled; mirrored)."""
    b = fs.base(res=res, spp=spp)
    b.object_begin("kit")
    _shapes(b, instanced=True)
    b.material_matte((0.6, 0.6, 0.6))
    scenes._quad(b, (-0.6, -1.9, -0.6), (0.6, -1.9, -0.6), (0.6, -1.9, 0.6), (-0.6, -1.9, 0.6))
    b.object_end()
    b.object_instance("kit", T.transform_translate(0.1, 0.2, 0.3))
    fs.room(b, size=3.0)
    b.object_instance("kit", T.transform_mul(T.transform_translate(1.2, -0.4, 1.0), T.transform_mul(T.transform_rotate_x(25.0), T.transform_scale(0.5, 0.8, 0.6))))
    b.object_instance("kit", T.transform_mul(T.transform_translate(-1.4, 0.3, 1.2), T.transform_scale(-0.5, 0.5, 0.5)))
    return b.build()


def scene_axis(res=40, spp=8):
    """Translated and scaled shapes only: a ray along an axis keeps exact zeros in object space."""
    b = fs.base(res=res, spp=spp)
    fs.room(b)
    b.material_matte((0.3, 0.4, 0.8))
    t = T.transform_mul(T.transform_translate(-0.75, -0.5, 0.25), T.transform_scale(0.5, 0.5, 1.5))
    b.shape_cylinder(radius=1.0, zmin=-1.0, zmax=0.5, object_to_world=t[0], world_to_object=t[1])
    t = T.transform_translate(0.75, 0.25, 0.5)
    b.shape_cylinder(radius=0.5, zmin=-0.75, zmax=0.75, phimax=270.0, object_to_world=t[0], world_to_object=t[1])
    b.material_matte((0.8, 0.7, 0.2))
    t = T.transform_translate(0.5, -1.0, -0.5)
    b.shape_disk(height=0.25, radius=0.75, innerradius=0.25, object_to_world=t[0], world_to_object=t[1])
    t = T.transform_mul(T.transform_translate(-0.5, 1.0, -0.75), T.transform_scale(1.0, 0.5, 1.0))
    b.shape_disk(height=-0.125, radius=0.5, phimax=200.0, object_to_world=t[0], world_to_object=t[1])
    return b.build()


# name -> (scene, key of the geometry, instanced)
RAY_CASES = {
    "quadrics_sah_leaf4": (lambda: scene_world("sah", 4), "world", False),
    "quadrics_hlbvh_leaf2": (lambda: scene_world("hlbvh", 2), "world", False),
    "quadrics_axis": (scene_axis, "axis", False),
    "quadrics_instanced": (scene_instanced, "instanced", True),
}


def _analytic(sd):
    return [Q._Quadric(sd.buffers["spheres"][i]) for i in range(sd.desc.n_spheres) if sd.buffers["spheres"][i].kind != 0 and sd.buffers["spheres"][i].object == 0]


def _to_world(sp, p):
    return p @ sp.o2w[:3, :3].T + sp.o2w[:3, 3]


def _surface_points(sp, n, rng):
    """Object-space points on the shape proper (inside the clips)."""
    phi = rng.uniform(0.05, 0.95, n) * sp.phimax
    if sp.kind == Q.SHAPE_CYLINDER:
        z = sp.zmin + rng.uniform(0.05, 0.95, n) * (sp.zmax - sp.zmin)
        return np.stack([sp.r * np.cos(phi), sp.r * np.sin(phi), z], 1)
    rho = sp.ri + rng.uniform(0.05, 0.95, n) * (sp.r - sp.ri)
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), np.full(n, sp.h)], 1)


def _rim_rays(shapes, info, n, rng):
    """Rays aimed at the rims: a cylinder's circles z = zmin / zmax and lines phi = 0 / phimax, a disk's circles r = radius /
    innerradius and its phi seam, each target moved off its rim by 1e-7 ... 1e-2 of the radius."""
    wb = np.array(list(info.world_bound), np.float64)
    os_, ds, ts = [], [], []
    per = -(-n // len(shapes))
    for sp in shapes:
        which = rng.integers(0, 4, per)
        phi = np.where(which == 2, 0.0, np.where(which == 3, sp.phimax, rng.uniform(0.0, 1.0, per) * sp.phimax))
        if sp.kind == Q.SHAPE_CYLINDER:
            z = np.where(which == 0, sp.zmin, np.where(which == 1, sp.zmax, sp.zmin + rng.uniform(0, 1, per) * (sp.zmax - sp.zmin)))
            p = np.stack([sp.r * np.cos(phi), sp.r * np.sin(phi), z], 1)
        else:
            rho = np.where(which == 0, sp.r, np.where(which == 1, sp.ri, sp.ri + rng.uniform(0, 1, per) * (sp.r - sp.ri)))
            p = np.stack([rho * np.cos(phi), rho * np.sin(phi), np.full(per, sp.h)], 1)
        p += rng.standard_normal((per, 3)) * (sp.r * np.exp(rng.uniform(np.log(1e-7), np.log(1e-2), (per, 1))))
        target = _to_world(sp, p)
        o = wb[:3] + rng.random((per, 3)) * (wb[3:] - wb[:3])
        d = (target - o) * np.exp(rng.uniform(-1, 1, (per, 1)))
        os_.append(o); ds.append(d)
        ts.append(np.where(rng.random(per) < 0.5, np.inf, np.exp(rng.uniform(-0.5, 0.5, per)) / np.exp(rng.uniform(-1, 1, per))))
    o, d, t = np.concatenate(os_)[:n], np.concatenate(ds)[:n], np.concatenate(ts)[:n]
    return o.astype(np.float32), d.astype(np.float32), t.astype(np.float32)


def _surface_rays(shapes, n, rng):
    """Rays that start on a shape's surface (the float32 image of an object-space surface point, any direction) and, half of a
    cylinder's, between its axis and its wall: inside it.  (A start on the surface is undecided by rule c more often than not: their number
    is what keeps the case's left-out share under the cap.)"""
    os_ = []
    per = -(-n // len(shapes))
    for sp in shapes:
        p = _surface_points(sp, per, rng)
        if sp.kind == Q.SHAPE_CYLINDER:
            inside = rng.random(per) < 0.5
            p[inside, :2] *= rng.uniform(0.0, 0.9, (int(inside.sum()), 1))
        os_.append(_to_world(sp, p))
    o = np.concatenate(os_)[:n]
    d = rng.standard_normal((n, 3))
    return o.astype(np.float32), d.astype(np.float32), np.full(n, np.inf, np.float32)


def _parallel_rays(shapes, info, n, rng):
    """Under an axis-aligned transform: rays along z through a cylinder's footprint (exactly parallel to its axis, inside and outside
    the wall) and rays with d.z = 0 that start in a disk's plane or beside it."""
    os_, ds = [], []
    per = -(-n // len(shapes))
    for sp in shapes:
        p = np.stack([rng.uniform(-1.5, 1.5, per) * sp.r, rng.uniform(-1.5, 1.5, per) * sp.r, rng.uniform(-2.0, 2.0, per)], 1)
        if sp.kind == Q.SHAPE_CYLINDER:
            d = np.stack([np.zeros(per), np.zeros(per), rng.choice([-1.0, 1.0, 0.5, -2.0], per)], 1)
        else:
            on = rng.random(per) < 0.5
            p[:, 2] = np.where(on, sp.h, sp.h + rng.choice([-0.25, 0.25, 0.5], per))
            ang = rng.uniform(0, 2 * np.pi, per)
            d = np.stack([np.cos(ang), np.sin(ang), np.zeros(per)], 1)
        os_.append(_to_world(sp, p)); ds.append(d @ sp.o2w[:3, :3].T)
    o, d = np.concatenate(os_)[:n], np.concatenate(ds)[:n]
    return o.astype(np.float32), d.astype(np.float32), np.full(n, np.inf, np.float32)


def make_rays(name, sd, info, camera_rays, seed=11):
    """(o, d, t_max, kind) of a case; camera_rays(pixel_xy, sample_index) -> (o, d, ...) is the device's generator or any other."""
    rng = np.random.default_rng(seed)
    shapes = _analytic(sd)
    world = bool(shapes)
    n_par = N_PARALLEL if name == "quadrics_axis" else 0
    n = N_RAYS - ((N_SURFACE + N_RIM + n_par) if world else 0)
    sb = list(info.sample_bounds)
    n_cam = n // 3
    px = np.stack([rng.integers(sb[0], sb[2], n_cam), rng.integers(sb[1], sb[3], n_cam)], 1).astype(np.int32)
    si = rng.integers(0, max(1, info.spp), n_cam).astype(np.uint32)
    cam = camera_rays(px, si)
    n_rand = (n - n_cam) // 2
    ro, rd, rt = random_rays(info, n_rand, seed)
    so, sd_, st = random_rays(info, n - n_cam - n_rand, seed + 1, shadow_like=True)
    parts = [(cam[0], cam[1], np.full(n_cam, np.inf, np.float32)), (ro, rd, rt), (so, sd_, st)]
    if world:
        parts += [_surface_rays(shapes, N_SURFACE, rng), _rim_rays(shapes, info, N_RIM, rng)]
        if n_par:
            parts.append(_parallel_rays(shapes, info, n_par, rng))
    o, d, t = (np.concatenate([p[k] for p in parts]) for k in range(3))
    assert len(o) == N_RAYS
    perm = rng.permutation(N_RAYS)
    kind = np.asarray([1, 2, 3], np.uint8)[rng.integers(0, 3, N_RAYS)]
    return np.ascontiguousarray(o[perm], np.float32), np.ascontiguousarray(d[perm], np.float32), np.ascontiguousarray(t[perm], np.float32), kind


def host_camera_rays(info):
    """A stand-in for the device's camera-ray generator where there is no device: rays from the camera's position through the room.
    (The truth takes whatever rays it is given; the CPU test only needs rays of the same kind.)"""
    def gen(px, si):
        rng = np.random.default_rng(3)
        n = len(px)
        o = np.repeat(np.array([[0.0, 0.0, -6.5]], np.float32), n, 0)
        d = np.stack([rng.uniform(-0.36, 0.36, n), rng.uniform(-0.36, 0.36, n), np.ones(n)], 1).astype(np.float32)
        return o, d
    return gen


_truths = {}


def truth_of(key, sd, rays):
    k = (key, rays[0].tobytes(), rays[1].tobytes(), rays[2].tobytes())
    if k not in _truths:
        _truths[k] = Q.closest_hits(Q.Scene(sd), rays[0], rays[1], rays[2])
        for a in _truths[k].values():
            a.setflags(write=False)
    return _truths[k]


# --------------------------------------------------------------------------------------------------------------------- lights
def scene_lights():
    """A full disk light (one-sided, facing down), a full cylinder light (two-sided) and a partial annulus light, where Disk::sample's
    whole-disk sampling shows: points outside the annulus sector are sampled, with the sector's density."""
    b = fs.base(res=16, spp=1)
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=(10, 9, 8))
    t = T.transform_mul(T.transform_translate(0.2, 1.5, 0.1), T.transform_rotate_x(90.0))
    b.shape_disk(height=0.0, radius=0.6, object_to_world=t[0], world_to_object=t[1])
    b.area_light_source_diffuse(L=(3, 5, 7), twosided=True)
    t = T.transform_mul(T.transform_translate(-1.0, -0.2, 0.5), T.transform_rotate_x(-70.0))
    b.shape_cylinder(radius=0.25, zmin=-0.6, zmax=0.5, object_to_world=t[0], world_to_object=t[1])
    b.area_light_source_diffuse(L=(2, 2, 2))
    t = T.transform_mul(T.transform_translate(1.1, 0.4, -0.2), T.transform_mul(T.transform_rotate_x(60.0), T.transform_scale(0.7, 0.5, 0.6)))
    b.shape_disk(height=0.1, radius=0.8, innerradius=0.3, phimax=200.0, object_to_world=t[0], world_to_object=t[1])
    b.no_area_light()
    fs.room(b, light_L=(1, 1, 1))
    return b.build()


LIGHT_POINTS = [(0.1, -0.8, 0.2), (-1.6, 1.2, -1.0), (0.9, -1.5, 1.4)]
LIGHT_CASES = [(light, p) for p in LIGHT_POINTS for light in range(3)]
SOLID_ANGLE_CASES = [(0, (0.1, -0.8, 0.2)), (0, (0.9, -1.5, 1.4)), (1, (0.1, -0.8, 0.2)), (1, (-1.6, 1.2, -1.0))]      # the full disk, the full cylinder


def light_id(c):
    return "light%d-%s" % (c[0], "_".join("%g" % v for v in c[1]))


def hold_solid_angle(label, sc, light, ref_p, sample):
    """geometry_cases.hold_solid_angle's rule with this module's truth: mean(1 / pdf) over the 64 x 64 grid against the quadrature of the
    solid angle, within twice the float64 restatement's own 64 x 64 discrepancy plus the float32 density's relative bound."""
    u = G.stratum_grid(64)[:4096]
    tr = Q.light_truth(sc, light, ref_p, u)
    omega = float(tr["solid_angle"][0])
    assert tr["valid"].all() and np.isfinite(omega)
    d64 = abs(float(np.mean(1.0 / tr["pdf"])) - omega)
    tol = 2.0 * d64 + omega * float(tr["pdf_rel"].max())
    pdf = sample(u)
    got = float(np.mean(1.0 / pdf.astype(np.float64)))
    line = "%-40s solid angle %.8f  mean(1/pdf) %.8f  off %.3g  tolerance %.3g  (float64 grid: 64^2 off %.3g)" % (label, omega, got, abs(got - omega), tol, d64)
    print(line)
    assert (pdf > 0).all()
    assert abs(got - omega) <= tol, line
    return line
