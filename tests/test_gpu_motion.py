"""Motion blur on the device: rays that carry a time against the float64 truth of motion_ref.py, the camera's time and ray, and the
static limits of a moving scene held bit for bit to the static scenes built from its start and end transforms (which the oracle checks).

Measured on the first run (profiles/motion_truth.txt has the lines): 0.76 % of the rays left out, err / bound worst 0.515 and median
0.0061 under both accelerators; the moving camera's ray at most 0.26 of its bound."""
import numpy as np
import pytest

import feature_scenes as fs
import geometry_cases as GC
import geometry_ref as G
import motion_cases as MC
import motion_ref as MR
from helpers import bits, pkg, scenes

pytestmark = pytest.mark.gpu
capi = pkg.capi


def _hold_prims(label, tr, sel, hits):
    """Same world primitive on every decisive hit (an instance reports its own position in the world list)."""
    dec = (tr["rule"][sel] == 0) & (tr["kind"][sel] > 0)
    wrong = dec & (hits["prim"] != tr["prim"][sel])
    assert not wrong.any(), "%s: world primitive differs on %d decisive rays" % (label, wrong.sum())


# ------------------------------------------------------------------------------------------------ 6: rays against the truth
@pytest.mark.parametrize("split, mnp", [("sah", 4), ("hlbvh", 1)])
def test_rays_with_a_time_against_truth(gpu_ctx, split, mnp):
    sd = MC.motion_instances(split=split, maxnodeprims=mnp)
    ctx = gpu_ctx
    ctx.upload(sd)
    assert ctx.kernel_set() == capi.PT_KERNELS_MOTION == 4
    rays = MC.make_rays(ctx.generate_camera_rays, sd)
    o, d, t, kind, time = rays
    tr = MC.truth_of(sd, rays)
    name = "motion_instances %s/%d" % (split, mnp)
    every = np.ones(len(t), bool)
    hits = ctx.trace_closest(o, d, t, time=time)
    occ = ctx.trace_any(o, d, t, time=time)
    ratio = GC.hold_hits(name + " batch", tr, every, hits, inst=True)
    _hold_prims(name + " batch", tr, every, hits)
    GC.hold_occlusion(name + " batch", tr, every, occ)
    GC.report("device " + name + " batch", tr, ratio)
    whits, wocc = ctx.trace_wavefront(o, d, t, kind, time=time)
    m1, m2, m3 = kind == 1, kind == 2, kind == 3
    wratio = GC.hold_hits(name + " wavefront", tr, m1, whits[m1], inst=True)
    _hold_prims(name + " wavefront", tr, m1, whits[m1])
    GC.hold_occlusion(name + " wavefront", tr, m2, wocc[m2])
    # (a probe keeps the record it met, which inside an instance is the object's own: hit or miss is what the hook can be held to)
    dec3 = tr["rule"][m3] == 0
    assert np.array_equal((whits["prim"][m3] >= 0)[dec3], (tr["kind"][m3] > 0)[dec3]), name + " wavefront probes: hit / miss differs"
    assert len(wratio) >= 500 and float(np.median(wratio)) <= GC.MEDIAN_LIMIT          # (a third of the rays are continuation items)
    print("device %-28s wavefront: err/bound worst %.3f median %.4f (%d continuation hits, %d shadow, %d probe items)" % (
        name, wratio.max(), np.median(wratio), len(wratio), m2.sum(), m3.sum()))
    # the two entrances run the same arithmetic
    assert np.array_equal(whits["t"][m1], hits["t"][m1]) and np.array_equal(whits["prim"][m1], hits["prim"][m1]) and np.array_equal(wocc[m2], occ[m2])
    # every branch of interpolate ran, and rays met what moves while it was between its ends
    inside = (time > 0) & (time < 1)
    moving = np.isin(tr["prim"], [0, 1, 2, 7, 8, 9])          # (the floor is 3, 4; the static instance 5, the one with equal ends 6)
    assert (time <= 0).sum() > 500 and (time >= 1).sum() > 500 and (inside & moving & (tr["rule"] == 0)).sum() > 300
    # the hooks without a time trace at time 0
    h0 = ctx.trace_closest(o, d, t)
    assert np.array_equal(h0, ctx.trace_closest(o, d, t, time=np.zeros(len(t), np.float32)))
    assert not np.array_equal(h0["t"], hits["t"])


# ------------------------------------------------------------------------------------------------------------ 7: the camera
CAM_END = ((1.2, 0.4, -6.0), (1.2 + 6.5 * np.sin(np.radians(30.0)), 0.4, -6.0 + 6.5 * np.cos(np.radians(30.0))), (0, 1, 0))


CAM_END_LOOK = ((1.2, 0.4, -6.0), (0.3, -0.5, 0.0), (0, 1, 0))          # for the rendered limits: moved and turned, still on the scene


def _camera_scene(lens, end=True, identity=False):
    b = scenes.SceneBuilder()
    if identity:
        b.camera_to_world = np.eye(4, dtype=np.float32).reshape(-1)
    else:
        b.look_at((0, 0, -6.5), (0, 0, 0), (0, 1, 0))
        if end:
            b.look_at_end(*CAM_END)
    b.camera_perspective(fov=40.0, shutteropen=0.25, shutterclose=0.75, lensradius=0.05 if lens else 0.0, focaldistance=6.0)
    b.film(xresolution=16, yresolution=16)
    b.pixel_filter_box()
    b.sampler_sobol(16)
    b.transform_times(0.0, 1.0)
    scenes._quad(b, (2.5, -2.0, -2.0), (-2.5, -2.0, -2.0), (-2.5, -2.0, 2.5), (2.5, -2.0, 2.5))
    return b.build()


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
def test_camera_time_and_ray(gpu_ctx, lens):
    """The time is the float32 lerp of the sampler's fifth dimension, exactly.  The ray is the camera-space ray (what the same scene
    generates under the identity: no rounding without a lens; with one the origin's nudge along d, gamma(3) |o| / |d|, is part of the
    bound) under the float64 M64(t): each component within gamma(3) of the transform's own sums plus |dM| on the camera-space ray, and
    the origin also within the nudge transform_ray applies, |d_w| dot(|d_w|, o_err) / |d_w|^2 <= sqrt(3) max(o_err) (transform.rs:184-203)."""
    ctx = gpu_ctx
    sd = _camera_scene(lens)
    ctx.upload(sd)
    assert ctx.kernel_set() == 4
    px = np.stack(np.meshgrid(np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 2).repeat(16, 0).astype(np.int32)
    si = np.tile(np.arange(16, dtype=np.uint32), 256)
    o, d, pf, tm = ctx.generate_camera_rays(px, si, with_time=True)
    u = ctx.sobol_samples(px, si, np.full(len(si), 4, np.uint32))
    want = (np.float32(1) - u) * np.float32(0.25) + u * np.float32(0.75)
    assert np.array_equal(bits(tm), bits(want))
    assert tm.min() >= 0.25 and tm.max() <= 0.75 and len(np.unique(tm)) > 1000
    o2, d2, pf2 = ctx.generate_camera_rays(px, si)                      # the hook without a time: the camera at time 0
    ctx.upload(_camera_scene(lens, end=False))
    assert ctx.kernel_set() == 0
    o0, d0, pf0, tm0 = ctx.generate_camera_rays(px, si, with_time=True)
    assert np.array_equal(bits(tm0), bits(want)) and np.array_equal(bits(o2), bits(o0)) and np.array_equal(bits(d2), bits(d0))
    ctx.upload(_camera_scene(lens, identity=True))
    oc, dc, _ = ctx.generate_camera_rays(px, si)
    oc, dc = oc.astype(np.float64), dc.astype(np.float64)
    d_ = sd.desc
    rec = MR.Record(d_.camera_to_world, d_.camera_to_world, sd.motion.camera_to_world_end, d_.camera_to_world, [0.0, 1.0])
    M, dM = rec.m64(tm.astype(np.float64))
    A, T = M[:, :3, :3], M[:, :3, 3]
    mul = lambda X, v: np.einsum("nij,nj->ni", X, v)
    g = G.gamma
    ow, dw = mul(A, oc) + T, mul(A, dc)
    cam_nudge = g(3) * np.abs(oc).sum(1)[:, None] * np.sqrt(3.0) * 2.0 if lens else 0.0          # the identity transform's own shift of a lens origin
    o_err = g(3) * (mul(np.abs(A), np.abs(oc)) + np.abs(T)) + mul(dM[:, :3, :3], np.abs(oc)) + dM[:, :3, 3] + mul(np.abs(A), np.ones_like(oc) * cam_nudge)
    d_err = g(3) * mul(np.abs(A), np.abs(dc)) + mul(dM[:, :3, :3], np.abs(dc))
    nudge = np.sqrt(3.0) * (g(3) * (mul(np.abs(A), np.abs(oc)) + np.abs(T))).max(1)[:, None] * 1.01
    ro = np.abs(o.astype(np.float64) - ow) / (o_err + nudge + g(2) * np.abs(ow))
    rd = np.abs(d.astype(np.float64) - dw) / np.maximum(d_err, 1e-300)          # (a component that is exactly zero has a zero bound, and must be exact)
    print("camera %-8s origin err/bound worst %.3f median %.4f   direction worst %.3f median %.4f" % ("lens" if lens else "pinhole", ro.max(), np.median(ro), rd.max(), np.median(rd)))
    assert ro.max() <= 1.0 and rd.max() <= 1.0
    assert np.abs(o.astype(np.float64) - o2).max() > 0.1          # and the camera did move


# -------------------------------------------------------------------------------------------- 8: static limits, bit for bit
@pytest.mark.parametrize("integrator", ["path", "directlighting", "ao"])
@pytest.mark.parametrize("at", [0, 1])
def test_static_limits_bit_for_bit(gpu_ctx, integrator, at):
    """Shutter 0..0: every sample's time is 0 and the clamped start branch hands back the stored pair; shutter 1..1: (1 - u) + u is 1 in
    float32 for every u in [0, 1), the end branch.  The radiance of a tile equals that of the static scene, bit for bit."""
    ctx = gpu_ctx
    kw = dict(light=True, integrator=integrator, spp=4, res=32)
    ctx.upload(MC.motion_instances(shutter=(float(at), float(at)), **kw))
    assert ctx.kernel_set() == 4
    tile = (8, 8, 24, 24)
    moving = ctx.radiance_samples(tile)
    ctx.upload(MC.motion_instances(at=at, **kw))
    assert ctx.kernel_set() == 0
    static = ctx.radiance_samples(tile)
    assert (static > 0).mean() > 0.2
    assert np.array_equal(bits(moving), bits(static))
    other = MC.motion_instances(at=1 - at, **kw)
    ctx.upload(other)
    assert not np.array_equal(bits(ctx.radiance_samples(tile)), bits(static))


@pytest.mark.parametrize("at", [0, 1])
def test_static_limits_of_the_camera(gpu_ctx, at):
    ctx = gpu_ctx
    kw = dict(light=True, spp=4, res=32, moves=[(n, s, None) for n, s, _ in MC.MOVES], camera_end=CAM_END_LOOK)
    ctx.upload(MC.motion_instances(shutter=(float(at), float(at)), **kw))
    assert ctx.kernel_set() == 4
    tile = (8, 8, 24, 24)
    moving = ctx.radiance_samples(tile)
    ctx.upload(MC.motion_instances(at=at, **kw))
    assert ctx.kernel_set() == 0
    static = ctx.radiance_samples(tile)
    assert (static > 0).mean() > 0.2
    assert np.array_equal(bits(moving), bits(static))


def test_a_moving_scene_blurs(gpu_ctx):
    """Between the limits the picture is neither: with the shutter open over the whole motion the radiance differs from both static
    scenes, and samples of one pixel see the moving boxes at different places."""
    ctx = gpu_ctx
    kw = dict(light=True, spp=16, res=32)
    tile = (0, 0, 32, 32)
    ctx.upload(MC.motion_instances(**kw))
    blur = ctx.radiance_samples(tile)
    ctx.upload(MC.motion_instances(at=0, **kw))
    s0 = ctx.radiance_samples(tile)
    ctx.upload(MC.motion_instances(at=1, **kw))
    s1 = ctx.radiance_samples(tile)
    d0, d1 = (blur != s0).any(-1).mean(), (blur != s1).any(-1).mean()
    print("samples that differ from the start scene %.3f, from the end scene %.3f" % (d0, d1))
    assert d0 > 0.02 and d1 > 0.02


# ---------------------------------------------------------------------------------------------------- 11: nothing else moved
def test_scenes_that_do_not_move_keep_their_kernels(gpu_ctx):
    ctx = gpu_ctx
    ctx.upload(fs.scene_instances())
    assert ctx.kernel_set() == 0
    ctx.upload(scenes.cornell_box(res=32, spp=4))
    assert ctx.kernel_set() == 0
    # records whose two ends are equal are static: the scene runs what it ran before, and renders what it rendered
    equal = [(n, s, s) for n, s, _ in MC.MOVES]
    sd = MC.motion_instances(moves=equal, light=True, spp=4, res=32)
    assert sd.motion.n_instances == len(MC.MOVES)
    ctx.upload(sd)
    assert ctx.kernel_set() == 0
    a = ctx.radiance_samples((8, 8, 24, 24))
    ctx.upload(MC.motion_instances(at=0, light=True, spp=4, res=32))
    assert np.array_equal(bits(a), bits(ctx.radiance_samples((8, 8, 24, 24))))


def test_bad_motion_records_fail_the_upload(gpu_ctx):
    ctx = gpu_ctx
    for what in ("index", "twice", "projective", "sign"):
        sd = MC.motion_instances()
        recs = sd.buffers["motion_instances"]
        if what == "index":
            recs[0].instance = 99
        elif what == "twice":
            recs[1].instance = recs[0].instance
        elif what == "projective":
            recs[0].instance_to_world_end[12] = 0.5
        else:                                            # mirrored at the end only: the lerped scale passes through zero
            m, mi = MC.S(-1.0, 1.0, 1.0)
            recs[0].instance_to_world_end[:] = [float(v) for v in m]
            recs[0].world_to_instance_end[:] = [float(v) for v in mi]
        with pytest.raises(capi.PtError) as e:
            ctx.upload(sd)
        assert "PT_ERR_INVALID_ARGUMENT" in str(e.value) and "motion" in str(e.value)
    ctx.upload(MC.motion_instances())          # and the context is still good
