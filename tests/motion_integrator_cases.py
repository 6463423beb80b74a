"""The rendered cases of the motion-blur tests -- `aov` distance, a moving occluder's shadow under `path`, and `ao` under the same occluder
-- with what the float64 truth of motion_ref.py says about every camera sample at that sample's time.  Shared by
test_gpu_motion_integrators.py, which holds the device's per-sample values to it, and test_motion_host.py, which shows on the CPU that
the truth alone decides the cases (at most 3 % left out), so the GPU tests cannot hide behind exclusions.

A `source` gives the camera samples: generate_camera_rays(pixel_xy, sample_index) and sobol_samples(pixel_xy, sample_index, dim) -- the
device context, or the oracle's scene built from the start transforms (the camera does not move in these scenes, so both make the same
rays).  A sample's time is lerp(u, shutteropen, shutterclose) in float32 with u the sampler's fifth dimension."""
import numpy as np

import motion_cases as MC
import motion_ref as MR
from aov_cases import pixel_samples
from helpers import scenes

RES = 16
MAX_LEFT_OUT = 0.03
AO_SAMPLES = 4
LIGHT = np.array([0.0, 7.0, 0.3])
LIFTS = (1e-5, 2e-3)


def sample_times(source, px, si, shutter=(0.0, 1.0)):
    u = source.sobol_samples(px, si, np.full(len(si), 4, np.uint32))
    return (np.float32(1) - u) * np.float32(shutter[0]) + u * np.float32(shutter[1])


def near_scene(integrator="aov", moving=True):
    """Everything within unit distance of the camera (AOV "distance" reports clamp(t / |d|, 0, 1)): two moving boxes, a moving clipped
    sphere, a one-triangle object that moves, a static floor.  moving=False: every instance at its start transform."""
    T, S, R, mul = MC.T, MC.S, MC.rotate, MC.mul
    b = scenes.SceneBuilder()
    b.look_at((0, 0, 0), (0, 0, 1), (0, 1, 0))
    b.camera_perspective(fov=60.0, shutteropen=0.0, shutterclose=1.0)
    b.film(xresolution=RES, yresolution=RES)
    b.pixel_filter_box()
    b.sampler_sobol(64)
    if integrator == "aov":
        b.integrator_aov(target="distance", scale=1.0)
    else:
        b.integrator_path(maxdepth=1)
    b.transform_times(0.0, 1.0)
    b.object_begin("box")
    MC._box(b)
    b.object_end()
    b.object_begin("shard")
    b.shape_trianglemesh([(-0.5, 0.0, 0.0), (0.5, 0.0, 0.1), (0.0, 0.9, 0.05)], [0, 1, 2])
    b.object_end()
    b.object_begin("ball")
    b.shape_sphere(radius=0.4, zmin=-0.25, zmax=0.3, phimax=300.0)
    b.object_end()
    s = S(0.2, 0.2, 0.2)
    inst = lambda name, a, e: b.object_instance(name, a, e if moving else None)
    inst("box", mul(T(-0.2, 0.0, 0.6), s), mul(T(0.1, 0.05, 0.5), R(90.0, (1.0, 2.0, 0.5)), s))
    scenes._quad(b, (0.6, -0.2, 0.15), (-0.6, -0.2, 0.15), (-0.6, -0.2, 0.9), (0.6, -0.2, 0.9))
    inst("box", mul(T(0.2, 0.15, 0.7), S(0.2, 0.12, 0.28)), mul(T(0.2, 0.15, 0.7), R(120.0, (0.3, 1.0, -0.2)), S(0.26, 0.12, 0.2)))
    inst("shard", mul(T(-0.1, -0.1, 0.4), s), mul(T(0.05, 0.0, 0.45), R(60.0, (0.0, 1.0, 0.0)), s))
    inst("ball", mul(T(0.0, 0.2, 0.55), s), mul(T(-0.15, 0.1, 0.6), R(45.0, (1.0, 0.0, 0.0)), s))
    return b.build()


NEAR_MOVING_PRIMS = [0, 3, 4, 5]          # (the floor is 1, 2)


def shadow_scene(occluder=True, integrator="path", moving=True):
    """A matte floor (uv given: dpdu = p1 - p0 on both triangles), a point light, and a box that moves and turns above the view -- the
    frustum reaches |y| < 2.4 at its depth -- between the floor and the light."""
    T, S, R, mul = MC.T, MC.S, MC.rotate, MC.mul
    b = scenes.SceneBuilder()
    b.look_at((0, 0, -6.5), (0, 0, 0), (0, 1, 0))
    b.camera_perspective(fov=40.0, shutteropen=0.0, shutterclose=1.0)
    b.film(xresolution=RES, yresolution=RES)
    b.pixel_filter_box()
    b.sampler_sobol(16)
    if integrator == "ao":
        b.integrator_ao(nsamples=AO_SAMPLES, cossample=True)
    else:
        b.integrator_path(maxdepth=1)
    b.transform_times(0.0, 1.0)
    b.object_begin("box")
    b.material_matte((0.3, 0.5, 0.8))
    MC._box(b)
    b.object_end()
    b.material_matte((0.7, 0.7, 0.7))
    scenes._quad(b, (2.5, -2.0, -2.0), (-2.5, -2.0, -2.0), (-2.5, -2.0, 2.5), (2.5, -2.0, 2.5), uv=[(0, 0), (1, 0), (1, 1), (0, 1)])
    if occluder and integrator == "ao":          # a slab (7 x 0.7 x 4.2) that moves and turns about y: a hemisphere's rays need more sky covered than a light's
        start = mul(T(-1.6, 3.6, 0.0), S(10.0, 1.0, 6.0))
        b.object_instance("box", start, mul(T(1.6, 3.6, 0.4), R(90.0, (0.0, 1.0, 0.0)), S(10.0, 1.0, 6.0)) if moving else None)
    elif occluder:
        start = mul(T(-1.6, 3.6, 0.0), S(2.0, 1.0, 2.0))
        b.object_instance("box", start, mul(T(1.6, 3.6, 0.4), R(90.0, (0.2, 1.0, 0.1)), S(2.0, 1.0, 2.0)) if moving else None)
    b.light_point(I=(60.0, 58.0, 55.0), frm=tuple(LIGHT))
    return b.build()


def aov_case(source):
    """The camera samples of the near scene and their truth: dict(sd, o, d, time, truth, left) -- left: the share the truth leaves out."""
    sd = near_scene()
    px, si = pixel_samples(sd, 64, (0, 0, RES, RES))
    o, d = source.generate_camera_rays(px, si)[:2]
    tm = sample_times(source, px, si)
    tr = MR.closest_hits(sd, o, d, np.full(len(tm), np.inf, np.float32), tm)
    return dict(sd=sd, px=px, si=si, o=o, d=d, time=tm, truth=tr, left=float((tr["rule"] != 0).mean()))


def _floor_points(source, sd, spp):
    px, si = pixel_samples(sd, spp, (0, 0, RES, RES))
    o, d = source.generate_camera_rays(px, si)[:2]
    tm = sample_times(source, px, si)
    cam = MR.closest_hits(sd, o, d, np.full(len(tm), np.inf, np.float32), tm)
    on_floor = (cam["rule"] == 0) & np.isin(cam["prim"], [0, 1])
    p = o.astype(np.float64) + cam["t"][:, None] * d.astype(np.float64)
    return px, si, o, d, tm, cam, on_floor, p


def _segments(sd, origin, direction, tmax, tm):
    """Occlusion of the rays from `origin` lifted off the floor by each of LIFTS, which bracket the device's own lift (its error bound,
    about 1e-6, rounded into float32 at |p| ~ 3): (occluded, decisive) -- decisive where the truth decides both and they agree."""
    occ, dec = [], np.ones(len(tm), bool)
    for lift in LIFTS:
        q = origin + np.array([0.0, lift, 0.0])
        dd = direction(q)
        s = MR.closest_hits(sd, q.astype(np.float32), dd.astype(np.float32), np.full(len(tm), tmax, np.float32), tm)
        occ.append(s["occluded"])
        dec &= s["rule"] == 0
    return occ[0], dec & (occ[0] == occ[1])


def shadow_case(source):
    """Per camera sample of the shadow scene: on_floor (the camera ray decisively ends on the floor), occluded / decisive for the segment
    from the floor point to the light at the sample's time, left (the undecided share of the floor samples, and of the camera rays)."""
    sd = shadow_scene()
    px, si, o, d, tm, cam, on_floor, p = _floor_points(source, sd, 16)
    occ, dec = _segments(sd, p, lambda q: LIGHT - q, 0.999, tm)
    dec &= on_floor
    left = max(1.0 - dec.sum() / max(1, on_floor.sum()), float((cam["rule"] != 0).mean()))
    return dict(sd=sd, px=px, si=si, o=o, d=d, time=tm, cam=cam, p=p, on_floor=on_floor, occluded=occ, decisive=dec, left=float(left))


def _cosine_hemisphere(u):
    """cosine_sample_hemisphere over concentric_sample_disk (core/sampling/sampling.rs:109-159), float64 on the float32 samples."""
    u = u.astype(np.float64)
    ox, oy = 2.0 * u[:, 0] - 1.0, 2.0 * u[:, 1] - 1.0
    wide = np.abs(ox) > np.abs(oy)
    with np.errstate(all="ignore"):
        r = np.where(wide, ox, oy)
        th = np.where(wide, (np.pi / 4) * (oy / ox), np.pi / 2 - (np.pi / 4) * (ox / oy))
    zero = (ox == 0) & (oy == 0)
    x, y = np.where(zero, 0.0, r * np.cos(th)), np.where(zero, 0.0, r * np.sin(th))
    return np.stack([x, y, np.sqrt(np.maximum(0.0, 1.0 - x * x - y * y))], 1)


def ao_case(source):
    """AOIntegrator::li (integrators/ao.rs:49-110) on the shadow scene with 4 cosine-weighted samples: per camera sample on the floor the
    number of occlusion rays the truth finds occluded at the sample's time.  Ray k of camera sample s takes dimensions 5, 6 of sampler
    index s * 4 + k; its direction is x ss + y tt + z n in the floor's frame -- n = (0, 1, 0) towards the camera, ss = normalize(dpdu) =
    (-1, 0, 0), tt = n x ss = (0, 0, 1): axis-aligned, so the frame is exact.  Every term of the estimate is dot(wi, n) / (pdf 4) = pi / 4,
    so the reported value is (4 - occluded) pi / 4.  A sample is decisive where all four rays are (under both lifts) and none grazes the
    horizon (z > 1e-3)."""
    sd = shadow_scene(integrator="ao")
    px, si, o, d, tm, cam, on_floor, p = _floor_points(source, sd, 16)
    n_occ, dec = np.zeros(len(tm), np.int64), on_floor.copy()
    for k in range(AO_SAMPLES):
        idx = (si.astype(np.uint32) * np.uint32(AO_SAMPLES) + np.uint32(k)).astype(np.uint32)
        u = np.stack([source.sobol_samples(px, idx, np.full(len(idx), dim, np.uint32)) for dim in (5, 6)], 1)
        w = _cosine_hemisphere(u)
        wi = np.stack([-w[:, 0], w[:, 2], w[:, 1]], 1)
        occ, dk = _segments(sd, p, lambda q: wi, np.inf, tm)
        n_occ += occ
        dec &= dk & (w[:, 2] > 1e-3)
    left = max(1.0 - dec.sum() / max(1, on_floor.sum()), float((cam["rule"] != 0).mean()))
    return dict(sd=sd, px=px, si=si, time=tm, on_floor=on_floor, n_occluded=n_occ, decisive=dec, left=float(left))
