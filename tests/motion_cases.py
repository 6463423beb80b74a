"""The scenes and ray sets of the motion-blur tests -- shared by test_motion_host.py, which shows on the CPU that motion_ref decides the
cases, and test_gpu_motion.py, which holds the device to it.

motion_instances: a 12-triangle box object instanced six times (pure translation; translation plus 90 degrees about a skew axis; 120
degrees plus a non-uniform scale; a static instance; a record whose two ends are equal; a mirror that translates), a one-triangle object
(wrapped without an accelerator) that moves, an object holding a clipped sphere that moves, and a static floor quad.  TransformTimes 0 1.
Rays: geometry_cases.make_rays' 8 191 (camera rays, random rays, shadow-like segments, rays that start on the floor), each with a time:
uniform in [-0.1, 1.1], every 16th exactly 0 and every 16th exactly 1, so that the three branches of AnimatedTransform::interpolate run."""
import numpy as np

import geometry_cases as GC
import motion_ref as MR
from helpers import scenes

f32 = np.float32
RES, SPP = 64, 16


class Info:
    """What geometry_cases.make_rays reads of a scene's info, fixed here so that the CPU and the GPU tests draw the same rays."""
    sample_bounds = [0, 0, RES, RES]
    spp = SPP
    world_bound = [-2.6, -2.2, -2.2, 2.6, 2.2, 2.6]


def rotate(theta_deg, axis):
    """Matrix4x4::rotate (matrix4x4.rs:97-120) as (m, m_inv = its transpose), float32."""
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    s, c = np.sin(np.radians(theta_deg)), np.cos(np.radians(theta_deg))
    m = np.eye(4)
    m[0, :3] = [a[0] * a[0] + (1 - a[0] * a[0]) * c, a[0] * a[1] * (1 - c) - a[2] * s, a[0] * a[2] * (1 - c) + a[1] * s]
    m[1, :3] = [a[0] * a[1] * (1 - c) + a[2] * s, a[1] * a[1] + (1 - a[1] * a[1]) * c, a[1] * a[2] * (1 - c) - a[0] * s]
    m[2, :3] = [a[0] * a[2] * (1 - c) - a[1] * s, a[1] * a[2] * (1 - c) + a[0] * s, a[2] * a[2] + (1 - a[2] * a[2]) * c]
    return m.astype(f32).reshape(-1), m.T.astype(f32).reshape(-1)


def mul(*ts):
    out = ts[0]
    for t in ts[1:]:
        out = scenes.transform_mul(out, t)
    return out


T = scenes.transform_translate
S = scenes.transform_scale

# (object, start, end): end None = a static instance
MOVES = [
    ("box", T(-1.6, -1.2, 0.4), T(-1.0, -0.7, 0.9)),                                                                   # pure translation
    ("box", T(0.0, -1.3, 0.2), mul(T(0.5, -1.0, 0.5), rotate(90.0, (1.0, 2.0, 0.5)))),                                  # translation + 90 degrees about a skew axis
    ("box", mul(T(1.5, -1.0, 1.0), S(1.0, 0.6, 1.4)), mul(T(1.5, -1.0, 1.0), rotate(120.0, (0.3, 1.0, -0.2)), S(1.3, 0.6, 1.0))),   # 120 degrees + non-uniform scale
    ("box", T(-1.4, 0.9, 1.3), None),                                                                                  # static
    ("box", mul(T(0.1, 1.0, 1.5), rotate(30.0, (0.0, 0.0, 1.0))), mul(T(0.1, 1.0, 1.5), rotate(30.0, (0.0, 0.0, 1.0)))),   # equal ends
    ("box", mul(T(1.5, 1.0, 0.8), S(-0.8, 0.8, 0.8)), mul(T(1.2, 1.3, 1.2), S(-0.8, 0.8, 0.8))),                        # a mirror
    ("shard", T(-0.4, -0.2, -0.6), mul(T(0.2, 0.1, -0.4), rotate(60.0, (0.0, 1.0, 0.0)))),                              # one triangle: the direct path
    ("ball", T(0.9, 0.1, -0.3), mul(T(0.6, 0.4, 0.0), rotate(45.0, (1.0, 0.0, 0.0)))),                                  # a clipped sphere
]


def _box(b, h=0.35):
    P = [(-h, -h, -h), (h, -h, -h), (h, h, -h), (-h, h, -h), (-h, -h, h), (h, -h, h), (h, h, h), (-h, h, h)]
    idx = [0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 0, 1, 5, 0, 5, 4, 3, 6, 2, 3, 7, 6, 0, 4, 7, 0, 7, 3, 1, 2, 6, 1, 6, 5]
    b.shape_trianglemesh(P, idx)


def motion_instances(split="sah", maxnodeprims=4, at=None, light=False, integrator="path", shutter=(0.0, 1.0), spp=SPP, res=RES, moves=None,
                     camera_end=None):
    """at = None: the moving scene.  at = 0 / 1: the static scene built from the start / end transforms (the static limits)."""
    b = scenes.SceneBuilder()
    b.look_at((0, 0, -6.5), (0, 0, 0), (0, 1, 0))
    if camera_end is not None and at is None:
        b.look_at_end(*camera_end)
    if camera_end is not None and at == 1:
        b.look_at(*camera_end)
    b.camera_perspective(fov=40.0, shutteropen=shutter[0], shutterclose=shutter[1])
    b.film(xresolution=res, yresolution=res)
    b.pixel_filter_box()
    b.sampler_sobol(spp)
    if integrator == "path":
        b.integrator_path(maxdepth=3)
    elif integrator == "directlighting":
        b.integrator_directlighting(maxdepth=3)
    elif integrator == "ao":
        b.integrator_ao(nsamples=4)
    b.accelerator_bvh(splitmethod=split, maxnodeprims=maxnodeprims)
    b.transform_times(0.0, 1.0)
    b.object_begin("box")
    b.material_matte((0.3, 0.5, 0.8))
    _box(b)
    b.object_end()
    b.object_begin("shard")
    b.material_matte((0.8, 0.4, 0.3))
    b.shape_trianglemesh([(-0.5, 0.0, 0.0), (0.5, 0.0, 0.1), (0.0, 0.9, 0.05)], [0, 1, 2])
    b.object_end()
    b.object_begin("ball")
    b.material_matte((0.4, 0.8, 0.4))
    b.shape_sphere(radius=0.4, zmin=-0.25, zmax=0.3, phimax=300.0)
    b.object_end()
    b.material_matte((0.7, 0.7, 0.7))
    for k, (name, start, end) in enumerate(MOVES if moves is None else moves):
        if k == 3:                                       # the floor in the middle of the world list
            scenes._quad(b, (2.5, -2.0, -2.0), (-2.5, -2.0, -2.0), (-2.5, -2.0, 2.5), (2.5, -2.0, 2.5))
        if at is None:
            b.object_instance(name, start, end)
        else:
            b.object_instance(name, end if (at == 1 and end is not None) else start)
    if light:
        b.light_point(I=(40.0, 38.0, 36.0), frm=(0.3, 1.9, -1.7))
    return b.build()


def times_for(n, seed=11):
    rng = np.random.default_rng(seed)
    t = rng.uniform(-0.1, 1.1, n).astype(f32)
    t[::16] = 0.0
    t[8::16] = 1.0
    return t


def make_rays(camera_rays, sd):
    """(o, d, t_max, kind, time) of the motion_instances case."""
    o, d, t, kind = GC.make_rays("motion_instances", sd, Info, camera_rays)
    return o, d, t, kind, times_for(len(t))


_truth = {}


def truth_of(sd, rays):
    k = tuple(a.tobytes() for a in rays)
    if k not in _truth:
        _truth[k] = MR.closest_hits(sd, rays[0], rays[1], rays[2], rays[4])
        for a in _truth[k].values():
            a.setflags(write=False)
    return _truth[k]
