"""The device's ray hits, occlusion flags and area-light samples held to the float64 truths of geometry_ref.py.  The oracle is never
loaded here: a misreading of the reference that orc_accel.hpp / orc_sphere.hpp share with pt_kernels.hip / pt_sphere.h passes every
bit-parity test and fails this one.  (test_geometry_truth_oracle.py holds the oracle to the same truths on the same cases.)

Every ray case sends its 8 191 rays (geometry_cases.make_rays; camera rays from the device's own generator) through both entrances:
pt_trace_closest / pt_trace_any (k_trace_batch*) and pt_trace_wavefront with kinds 1 / 2 / 3 dealt at random (the renderer's kernel):

    cornell               k_trace, one-sided light            rt4k_sah_leaf12      k_trace_seq
    rt4k_sah_leaf4        pooled leaf rounds                  spheres              k_trace_sph_dist: clipped, rotated, scaled, mirrored
    rt4k_hlbvh_leaf2      pooled leaf rounds                  instances            k_trace_inst (t, hit / miss, occlusion only)
    rt4k_sah_leaf4_far    k_trace_far, forced with PBRTGPU_TRACE_FAR=1 in a context of its own

On every ray the truth does not leave out: same hit or miss, same primitive (world primitives, in the merged list's numbering),
|t - t64| <= bound, |b - b64| <= bound_b, occlusion flag = "some hit in (bound, t_max)"; at most 3 % left out per case; the median of
err / bound below geometry_cases.MEDIAN_LIMIT; a ray with two tied hits still within bound of one of them."""
import numpy as np
import pytest

import geometry_cases as GC
import geometry_ref as G
from helpers import pkg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(GC.RAY_CASES))
def test_device_rays_against_truth(gpu_ctx, monkeypatch, name):
    make, key, env = GC.RAY_CASES[name]
    sd = make()
    ctx = gpu_ctx
    if env:                       # read when a context is created
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = pkg.Context(0)
    try:
        info = ctx.upload(sd)
        rays = GC.make_rays(name, sd, info, ctx.generate_camera_rays)
        o, d, t, kind = rays
        tr = GC.truth_of(key, sd, rays)
        inst = name == "instances"
        every = np.ones(len(t), bool)
        # the batch entrance
        hits = ctx.trace_closest(o, d, t)
        occ = ctx.trace_any(o, d, t)
        ratio = GC.hold_hits(name + " batch", tr, every, hits, inst=inst)
        GC.hold_occlusion(name + " batch", tr, every, occ)
        GC.report("device " + name + " batch", tr, ratio)
        # the wavefront entrance: continuation, shadow and probe items in one launch
        whits, wocc = ctx.trace_wavefront(o, d, t, kind)
        m1, m2, m3 = kind == 1, kind == 2, kind == 3
        wratio = GC.hold_hits(name + " wavefront", tr, m1, whits[m1], inst=inst)
        GC.hold_occlusion(name + " wavefront", tr, m2, wocc[m2])
        if not inst:
            GC.hold_hits(name + " wavefront probes", tr, m3, whits[m3], probe=True)
        assert len(wratio) >= 1000 and float(np.median(wratio)) <= GC.MEDIAN_LIMIT
        print("device %-21s wavefront: err/bound worst %.3f median %.4f (%d continuation hits, %d shadow, %d probe items)" % (
            name, wratio.max(), np.median(wratio), len(wratio), m2.sum(), m3.sum()))
        # the two entrances run the same arithmetic
        assert np.array_equal(whits["t"][m1], hits["t"][m1]) and np.array_equal(wocc[m2], occ[m2])
    finally:
        if ctx is not gpu_ctx:
            ctx.close()


@pytest.fixture(scope="module")
def light_scenes():
    return {k: (sd, G.Scene(sd)) for k, sd in ((k, make()) for k, make in GC.LIGHT_SCENES.items())}


@pytest.mark.parametrize("case", GC.light_cases(), ids=GC.light_id)
def test_device_light_samples_against_truth(gpu_ctx, light_scenes, case):
    scene, light, p = case
    sd, sc = light_scenes[scene]
    gpu_ctx.upload(sd)
    u = G.stratum_grid(64)
    tr = G.light_truth(sc, light, p, u)
    li, wi, pdf = gpu_ctx.light_sample_li(light, np.float32(p), u)
    GC.hold_light("device " + GC.light_id(case), tr, li, wi, pdf, p)


@pytest.mark.parametrize("case", GC.SOLID_ANGLE_CASES, ids=GC.light_id)
def test_device_mean_inverse_pdf_is_the_solid_angle(gpu_ctx, light_scenes, case):
    """mean(1 / pdf) over the 64 x 64 grid against the analytic solid angle (Van Oosterom-Strackee; a cone's 2 pi (1 - cos theta_max)),
    within twice the float64 restatement's own 64 x 64 discrepancy (geometry_cases.hold_solid_angle has the figures)."""
    scene, light, p = case
    sd, sc = light_scenes[scene]
    gpu_ctx.upload(sd)
    GC.hold_solid_angle("device " + GC.light_id(case), sc, light, p, lambda u: gpu_ctx.light_sample_li(light, np.float32(p), u)[2])
