"""Integrator "aov" on the device, held straight to the float64 restatement (tests/aov_ref.py), no oracle in between.

Per case (tests/aov_cases.py) every target is rendered by an upload of its own; per-sample values come from pt_radiance_samples, the
rays from pt_generate_camera_rays, the lens samples from pt_sobol_samples (dimensions 2, 3).  Asserted: err <= bound outside the
left-out set, left-out share <= 3 %, median err / bound <= 4 x the float32 restatement's (profiles/aov_truth.txt), `rdyc` exactly 0,
scale 0.25 multiplying every value exactly.  Then the checks that need no truth: `distance` against pt_trace_closest bit for bit, the
film against the fold of the per-sample values, tiles against the whole frame, and `path` after `aov` on one context."""
import ctypes as C

import numpy as np
import pytest

import aov_cases as AC
import aov_ref as R
import geometry_ref as G
from helpers import bits, scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _clean_counters(gpu_ctx):
    """Leave the session's context as the other modules expect it: counters at zero."""
    yield
    gpu_ctx.reset_counters()


def _samples(ctx):
    """Every camera sample of the uploaded scene: (pixel_xy, sample_index, o, d, p_film, u_lens, tile)."""
    sb = tuple(ctx.info.sample_bounds)
    px, si = AC.pixel_samples(None, ctx.info.spp, sb)
    o, d, pf = ctx.generate_camera_rays(px, si)
    ul = np.stack([ctx.sobol_samples(px, si, np.full(len(si), k, np.uint32)) for k in (2, 3)], 1)
    return px, si, o, d, pf, ul, sb


def _render_targets(ctx, build, targets, scale=1.0, **kw):
    out = {}
    for t in targets:
        ctx.upload(build(R.SCENE_NAME.get(t, t), scale, **kw))
        out[t] = ctx.radiance_samples(tuple(ctx.info.sample_bounds)).reshape(-1, 3)
    return out


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_targets_against_truth(gpu_ctx, name):
    build = AC.CASES[name]
    sd = build()
    gpu_ctx.upload(sd)
    px, si, o, d, pf, ul, sb = _samples(gpu_ctx)
    assert gpu_ctx.info.spp == R.Camera(sd).spp
    hits, und = AC.truth_hits(name, sd, o, d)
    truth = R.evaluate(sd, o, d, pf, ul, hits, np.float64)
    got = _render_targets(gpu_ctx, build, R.TARGETS)
    lines = []
    try:
        AC.check(name, got, truth, und | truth["und"], medians=AC.read_medians(), report=lines)
    finally:
        print("\n" + "\n".join(lines))
    assert not got["rdyc"].any()
    quarter = _render_targets(gpu_ctx, build, R.TARGETS, scale=0.25)
    for t in R.TARGETS:
        assert np.array_equal(bits(quarter[t]), bits(got[t] * np.float32(0.25))), (name, t, "scale 0.25")
    if name == "reports":          # Material "none" and the emitter report, the rays that miss give exactly 0
        prim = hits["prim"]
        for p in (0, 1):
            sel = (prim == p) & ~und
            assert sel.sum() > 100 and (got["n"][sel] != 0).any(1).all()
        assert (~truth["hit"]).sum() > 100 and not got["n"][~truth["hit"] & ~und].any()


def test_fbm_bump_moves_the_normal(gpu_ctx):
    """An fbm displacement: the shading normal differs from the unbumped one and stays a unit vector.  2 v - 1 undoes v2c exactly; normalize
    leaves |n| within gamma(7) of 1 (three products, two sums, the root, the divide) and v2c's `+ 0.5` adds one rounding of a number below 1
    per component: | |n| - 1 | <= gamma(7) + 4 * 2^-24."""
    bumped = _render_targets(gpu_ctx, AC.case_bump, ("ns", "dpdus"), bump="fbm")
    flat = _render_targets(gpu_ctx, AC.case_bump, ("ns", "dpdus"), bump=None)
    hit = flat["ns"].any(1)
    assert hit.sum() > 1000 and np.array_equal(hit, bumped["ns"].any(1))
    moved = (bumped["ns"][hit] != flat["ns"][hit]).any(1)
    assert moved.mean() > 0.9, moved.mean()
    assert ((bumped["dpdus"][hit] != flat["dpdus"][hit]).any(1)).mean() > 0.9
    n = 2.0 * bumped["ns"][hit].astype(np.float64) - 1.0
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= G.gamma(7) + 4 * R.U


def test_set_aov_range_and_no_leak(gpu_ctx):
    """Targets 17 and -1 are refused, 16 is taken; the pair belongs to the next upload alone: an upload without the call renders uv at scale 1."""
    lib, h = gpu_ctx.lib, gpu_ctx.h
    assert lib.pt_scene_set_aov(h, C.c_int32(17), C.c_float(1.0)) == 1
    assert lib.pt_scene_set_aov(h, C.c_int32(-1), C.c_float(1.0)) == 1
    assert lib.pt_scene_set_aov(h, C.c_int32(16), C.c_float(1.0)) == 0
    uv = _render_targets(gpu_ctx, AC.case_frame, ("uv",))["uv"]
    sd = AC.case_frame("n", 0.5)
    gpu_ctx.upload(sd)
    n_half = gpu_ctx.radiance_samples(tuple(gpu_ctx.info.sample_bounds)).reshape(-1, 3)
    assert not np.array_equal(n_half, uv)
    assert lib.pt_scene_upload(h, C.byref(sd.desc)) == 0               # no pt_scene_set_aov before this one
    again = gpu_ctx.radiance_samples(tuple(gpu_ctx.info.sample_bounds)).reshape(-1, 3)
    assert np.array_equal(bits(again), bits(uv))


@pytest.mark.parametrize("name", ["frame", "sphere", "instances", "alpha"])
def test_distance_is_the_traced_t(gpu_ctx, name):
    """`distance` is float32 t / |d| with the t of pt_trace_closest on the same rays, bit for bit (clamped to 1)."""
    gpu_ctx.upload(AC.CASES[name]("distance", 1.0))
    px, si, o, d, pf, ul, sb = _samples(gpu_ctx)
    got = gpu_ctx.radiance_samples(sb).reshape(-1, 3)
    h = gpu_ctx.trace_closest(o, d, np.full(len(o), np.inf, np.float32))
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=np.float32)
    want = np.where(h["prim"] >= 0, np.minimum(h["t"] / length, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    assert (h["prim"] >= 0).sum() > 500
    for c in range(3):
        assert np.array_equal(bits(got[:, c]), bits(want)), (name, c)


def test_distance_saturates(gpu_ctx):
    """A scene deeper than 1: the clamp comes before the scale, every hit reports exactly `scale`."""
    b = AC._builder("distance", 0.7)
    b.shape_trianglemesh([(-3.0, -2.0, -2.5), (3.0, -2.0, -2.0), (0.0, 3.0, -3.0)], [0, 1, 2])
    gpu_ctx.upload(b.build())
    px, si, o, d, pf, ul, sb = _samples(gpu_ctx)
    got = gpu_ctx.radiance_samples(sb).reshape(-1, 3)
    h = gpu_ctx.trace_closest(o, d, np.full(len(o), np.inf, np.float32))
    hit = h["prim"] >= 0
    assert hit.sum() > 1000 and (~hit).sum() > 10
    assert np.array_equal(bits(got[hit]), bits(np.full((hit.sum(), 3), 0.7, np.float32))) and not got[~hit].any()


@pytest.mark.parametrize("filt", ["box", "gaussian"])
def test_film_is_the_fold_of_the_samples(gpu_ctx, filt):
    """pt_render's film (X, Y, Z, weight) against the float64 fold of the per-sample values through the scene's filter table."""
    sd = AC.case_frame("n", 1.0, filt=filt)
    gpu_ctx.upload(sd)
    px, si, o, d, pf, ul, sb = _samples(gpu_ctx)
    rgb = gpu_ctx.radiance_samples(sb).reshape(-1, 3)
    gpu_ctx.film_clear()
    gpu_ctx.render()
    film = gpu_ctx.film_xyzw().reshape(AC.YRES, AC.XRES, 4).astype(np.float64)
    want = AC.fold_film(sd, pf, rgb)
    assert want[..., 3].min() > 0
    assert np.abs(film[..., :3] - want[..., :3]).max() <= 1e-5 * np.abs(want[..., :3]).max()
    assert np.abs(film[..., 3] - want[..., 3]).max() <= 1e-5 * np.abs(want[..., 3]).max()


def test_tiles_equal_the_whole_frame(gpu_ctx, pkg):
    gpu_ctx.upload(AC.case_instances("dpdx", 1.0))
    gpu_ctx.film_clear()
    gpu_ctx.render()
    whole = gpu_ctx.film_xyzw().copy()
    gpu_ctx.film_clear()
    for t in pkg.scenes.all_tiles(gpu_ctx.info):
        gpu_ctx.render([t])
    assert np.array_equal(bits(gpu_ctx.film_xyzw()), bits(whole)) and whole.any()


def test_path_after_aov(gpu_ctx, pkg):
    """The side call does not leak into a later upload: `path` after `aov` on one context is `path` on a fresh one."""
    gpu_ctx.upload(AC.case_lens("dpdvs", 0.25))
    gpu_ctx.film_clear()
    gpu_ctx.render()
    sd = scenes.cornell_box(res=32, spp=4)
    films = []
    fresh = pkg.Context(0)
    try:
        for ctx in (gpu_ctx, fresh):
            ctx.upload(sd)
            ctx.film_clear()
            ctx.render()
            films.append(ctx.film_xyzw().copy())
    finally:
        fresh.close()
    assert films[0].any() and np.array_equal(bits(films[0]), bits(films[1]))
