"""The time reaches every ray of a camera sample, and no hit is lost between the traversal and the surface reconstruction: rendered
values, sample by sample, against the float64 truth of motion_ref.py at that sample's time.  The cases, their truths and the proof that
the truth alone decides them (at most 3 % left out, checked on the CPU in test_motion_host.py) are in motion_integrator_cases.py."""
import numpy as np
import pytest

import geometry_ref as G
import motion_integrator_cases as IC
from helpers import bits

pytestmark = pytest.mark.gpu
RES = IC.RES
TILE = (0, 0, RES, RES)


def _device_times_are_the_cases(ctx, case):
    """pt_generate_camera_rays_time gives the ray and the time the case was built from."""
    o, d, pf, tm = ctx.generate_camera_rays(case["px"], case["si"], with_time=True)
    assert np.array_equal(bits(tm), bits(case["time"]))
    if "o" in case:
        assert np.array_equal(bits(o), bits(case["o"])) and np.array_equal(bits(d), bits(case["d"]))


def test_aov_distance_follows_each_samples_time(gpu_ctx):
    """Integrator "aov", target distance, 16 x 16 at 64 spp.  For every sample the truth does not leave out: a truth hit is reported as a
    hit (a value > 0: make_surf_inst found what the traversal found), a truth miss as 0, and the value is t / |d| within the truth's bound
    plus the division's and the length's roundings, gamma(6) t."""
    ctx = gpu_ctx
    sd = IC.near_scene()
    ctx.upload(sd)
    assert ctx.kernel_set() == 4
    case = IC.aov_case(ctx)
    _device_times_are_the_cases(ctx, case)
    o, d, tm, tr = case["o"], case["d"], case["time"], case["truth"]
    val = ctx.radiance_samples(TILE).reshape(-1, 3)
    assert np.array_equal(val[:, 0], val[:, 1]) and np.array_equal(val[:, 0], val[:, 2])
    dec = tr["rule"] == 0
    hit = tr["kind"] > 0
    assert case["left"] <= IC.MAX_LEFT_OUT, case["left"]
    v = val[:, 0].astype(np.float64)
    assert ((v > 0) == hit)[dec].all(), "%d decisive samples differ in hit / miss" % ((v > 0) != hit)[dec].sum()
    dl = np.sqrt((d.astype(np.float64) ** 2).sum(1))
    want = tr["t"] / dl
    m = dec & hit & (want < 0.999)
    ratio = np.abs(v - want)[m] / (tr["bound"][m] / dl[m] + G.gamma(6) * want[m])
    moving = np.isin(tr["prim"], IC.NEAR_MOVING_PRIMS)
    inside = (tm > 0) & (tm < 1)
    print("aov distance: left out %.2f %%, %d hits held, %d on moving instances between the times, err/bound worst %.3f median %.4f" % (
        100 * case["left"], m.sum(), (m & moving & inside).sum(), ratio.max(), np.median(ratio)))
    assert (m & moving & inside).sum() > 2000 and ratio.max() <= 1.0
    # the picture does depend on the time: the same samples at the start transforms report other distances
    ctx.upload(IC.near_scene(moving=False))
    v0 = ctx.radiance_samples(TILE).reshape(-1, 3)[:, 0]
    assert (v0 != val[:, 0]).mean() > 0.1


def test_shadow_rays_carry_the_samples_time(gpu_ctx):
    """A matte floor, a point light, a moving occluder out of the camera's view, `path` with maxdepth 1.  The same scene without the
    occluder gives every sample's unshadowed radiance L0; with it a sample's radiance is exactly L0 or exactly 0, and which one is what
    the truth says about the segment from the floor point to the light at the sample's time, on every decisive sample."""
    ctx = gpu_ctx
    ctx.upload(IC.shadow_scene())
    assert ctx.kernel_set() == 4
    case = IC.shadow_case(ctx)
    _device_times_are_the_cases(ctx, case)
    L = ctx.radiance_samples(TILE).reshape(-1, 3)
    ctx.upload(IC.shadow_scene(occluder=False))
    assert ctx.kernel_set() == 0
    L0 = ctx.radiance_samples(TILE).reshape(-1, 3)
    same, dark = (bits(L) == bits(L0)).all(1), (L == 0).all(1)
    assert (same | dark).all(), "%d samples are neither L0 nor 0" % (~(same | dark)).sum()
    assert not (case["cam"]["prim"] == 2).any()                           # the occluder is out of view
    assert case["left"] <= IC.MAX_LEFT_OUT, case["left"]
    dec, occ = case["decisive"] & (L0 > 0).any(1), case["occluded"]
    print("shadows: %d samples on the floor, %d decisive and lit, %d of them in shadow at their time (left out %.2f %%)" % (
        case["on_floor"].sum(), dec.sum(), (dec & occ).sum(), 100 * case["left"]))
    assert (dec & occ).sum() > 200 and (dec & ~occ).sum() > 200
    assert np.array_equal(dark[dec], occ[dec]), "%d decisive samples disagree with the truth" % (dark[dec] != occ[dec]).sum()
    # and the shadow does move: with the occluder held at its start the picture is another one
    ctx.upload(IC.shadow_scene(moving=False))
    assert ((ctx.radiance_samples(TILE).reshape(-1, 3) == 0).all(1)[dec] != dark[dec]).mean() > 0.05


def test_ao_rays_carry_the_samples_time(gpu_ctx):
    """`ao` with 4 samples on the same scene: every term of the estimate is pi / 4 (cosine sampling), so a sample's value counts its
    unoccluded rays, and the occluded count equals the truth's at the sample's time on every decisive sample.  The terms are float32:
    dot(wi, n) / (pdf 4) with pdf = |z| / pi is pi / 4 within gamma(8), far from the 1 / 4 between two counts."""
    ctx = gpu_ctx
    ctx.upload(IC.shadow_scene(integrator="ao"))
    assert ctx.kernel_set() == 4
    case = IC.ao_case(ctx)
    _device_times_are_the_cases(ctx, case)
    v = ctx.radiance_samples(TILE).reshape(-1, 3)[:, 0].astype(np.float64)
    assert case["left"] <= IC.MAX_LEFT_OUT, case["left"]
    dec, want = case["decisive"], case["n_occluded"]
    unocc = v / (np.pi / 4)
    assert (np.abs(unocc - np.rint(unocc))[dec] <= 4 * G.gamma(8)).all()
    got = IC.AO_SAMPLES - np.rint(unocc).astype(np.int64)
    hist = np.bincount(want[dec], minlength=IC.AO_SAMPLES + 1)
    print("ao: %d samples on the floor, %d decisive (left out %.2f %%), occluded counts 0..4: %s" % (case["on_floor"].sum(), dec.sum(), 100 * case["left"], [int(h) for h in hist]))
    assert hist[1:].sum() > 200 and hist[0] > 200
    assert np.array_equal(got[dec], want[dec]), "%d decisive samples disagree with the truth" % (got[dec] != want[dec]).sum()
    # the occlusion rays are not traced at the start transform
    ctx.upload(IC.shadow_scene(integrator="ao", moving=False))
    v0 = ctx.radiance_samples(TILE).reshape(-1, 3)[:, 0]
    assert (np.rint(v0 / (np.pi / 4)).astype(np.int64)[dec] != (IC.AO_SAMPLES - want)[dec]).mean() > 0.03
