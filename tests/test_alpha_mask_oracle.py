"""The oracle's restatement of AlphaMaskShape (shapes/alphamask.rs; orc_accel.hpp tri_shape_intersect / tri_shape_intersect_p) on the CPU,
held to two truths that do not come from it:

  * removal equivalence: where every masked triangle lies inside one region of constant mask value (the scenes of test_gpu_alpha_mask.py),
    the oracle's render of the masked scene equals its render of the scene with those triangles cut out, per sample, film weight and ray;
  * a float64 numpy mask (alpha_mask_ref.py) for masks that vary inside a triangle: trace_closest reaches the mesh exactly where alpha > 0,
    trace_any where alpha and shadowalpha both are, outside a band of float32 rounding whose share of the points is capped and printed;

and that no masked scene reaches the oracle with its masks dropped."""
import os

import numpy as np
import pytest

import alpha_mask_ref as am
import feature_scenes as fs
from helpers import bits, pkg
from test_gpu_alpha_mask import REMOVAL, hook_scene, removal_scene, whitted_scene


def _render(oracle, sd):
    osc = oracle.scene(sd)
    try:
        rs = osc.radiance_samples(tuple(osc.info.sample_bounds))
        x, cnt, _ = osc.render(threads=8)
    finally:
        osc.close()
    return rs, x, cnt


def _camera_hits(oracle, sd):
    """As test_gpu_alpha_mask.camera_hits, through the oracle: the primitive each (pixel, sample) camera ray hits."""
    osc = oracle.scene(sd)
    try:
        b = list(osc.info.sample_bounds)
        w, h, spp = b[2] - b[0], b[3] - b[1], osc.info.spp
        ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
        pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
        o, d, _ = osc.generate_camera_rays(pix, np.tile(np.arange(spp, dtype=np.uint32), w * h))
        return osc.trace_closest(o, d, np.full(len(d), np.inf, np.float32))[0]["prim"].reshape(w * h, spp)
    finally:
        osc.close()


# ---------------------------------------------------------------- removal equivalence
@pytest.mark.parametrize("integ,material,sampler,extra,mask", REMOVAL, ids=["-".join(str(x) for x in (c[0][0], c[0][1], *c[1:])) for c in REMOVAL])
def test_masked_render_equals_the_cut_scene(oracle, integ, material, sampler, extra, mask):
    """check_equivalent of test_gpu_alpha_mask.py with the oracle on both sides."""
    masked = removal_scene(False, integ, material, sampler, extra, mask)
    assert masked.alpha_masks
    ms, mx, mc = _render(oracle, masked)
    cs, cx, cc = _render(oracle, removal_scene(True, integ, material, sampler, extra, mask))
    assert np.array_equal(bits(ms), bits(cs)), np.abs(ms - cs).max()
    assert np.array_equal(bits(mx[..., 3]), bits(cx[..., 3]))
    assert np.allclose(mx[..., :3], cx[..., :3], rtol=1e-6, atol=1e-7)
    for k in ("camera_rays", "regular_rays", "shadow_rays"):
        assert mc[k] == cc[k], (k, mc[k], cc[k])


def test_shadowalpha_zero_blocker_under_whitted(oracle):
    sd = whitted_scene("shadow")
    hit = _camera_hits(oracle, sd)
    sees = (hit == 6) | (hit == 7)
    assert sees.any() and (~sees).any()
    gs, _, _ = _render(oracle, sd)
    none, _, _ = _render(oracle, whitted_scene(None))
    opaque, _, _ = _render(oracle, whitted_scene("opaque"))
    assert np.array_equal(bits(gs[~sees]), bits(none[~sees]))          # shadow rays pass through the blocker
    assert np.array_equal(bits(gs[sees]), bits(opaque[sees]))          # camera rays still see it
    assert not np.array_equal(bits(none), bits(opaque))


def test_invisible_emitter_keeps_lighting(oracle):
    visible = whitted_scene(None)
    hit = _camera_hits(oracle, visible)
    sees = (hit == 4) | (hit == 5)
    assert sees.any() and (~sees).any()
    masked = whitted_scene(None, emitter_alpha=0.0)
    osc = oracle.scene(masked)
    assert osc.info.n_lights == 4                                       # area, sampling and pdf ignore the mask (alphamask.rs:115-146)
    osc.close()
    gs, _, _ = _render(oracle, masked)
    rs, _, _ = _render(oracle, visible)
    assert np.array_equal(bits(gs[~sees]), bits(rs[~sees]))
    assert not np.array_equal(bits(gs[sees]), bits(rs[sees]))           # those samples look through it


def test_constants_cut_or_do_nothing(oracle):
    """alpha <= 0 takes the mesh out of every ray, shadowalpha <= 0 out of shadow rays only, a positive constant changes nothing
    (alphamask.rs:29-53); the hook scene of test_gpu_alpha_mask.py, rays into every quad."""
    from test_gpu_alpha_mask import hook_points
    pts, _ = hook_points()
    o = np.concatenate([pts, np.full((len(pts), 1), 2.0, np.float32)], 1)
    d = np.tile(np.array([[0, 0, -1]], np.float32), (len(pts), 1))
    for alpha, shadow, seen, blocks in ((None, None, True, True), (0.0, None, False, False), (-1.0, 2.0, False, False), (None, 0.0, True, False),
                                        (0.5, -1.0, True, False), (2.0, 0.3, True, True)):
        sd, _, n_grid = hook_scene(alpha, shadow)
        osc = oracle.scene(sd)
        try:
            h, _ = osc.trace_closest(o, d, np.full(len(pts), np.inf, np.float32))
            assert np.all((h["prim"] < n_grid) == seen) and np.all(h["prim"] >= 0)
            assert np.allclose(h["t"], 1.0 if seen else 3.0, rtol=1e-6, atol=0.0)
            occ, _ = osc.trace_any(o, d, np.full(len(pts), 2.5, np.float32))
            assert np.all(occ.astype(bool) == blocks)
            e, _ = osc.trace_closest(o, d, np.full(len(pts), np.inf, np.float32), exhaustive=True)
            assert np.array_equal(e["prim"], h["prim"]) and np.array_equal(bits(e["t"]), bits(h["t"]))
        finally:
            osc.close()


# ---------------------------------------------------------------- masks that vary inside a triangle, against float64 numpy
CASES = am.cases()
NAMES = list(CASES)


def _tracer(osc, n_plane):
    return (lambda o, d, t: osc.trace_closest(o, d, t)[0]), (lambda o, d, t: osc.trace_any(o, d, t)[0]), n_plane


@pytest.mark.parametrize("uv", [True, False], ids=["uv", "default_uv"])
@pytest.mark.parametrize("name", NAMES)
def test_varying_mask_against_float64(oracle, name, uv):
    """alpha = the case, shadowalpha = the next case of the list (two different textures on one mesh)."""
    alpha, shadow = CASES[name], CASES[NAMES[(NAMES.index(name) + 1) % len(NAMES)]]
    sd, n_plane = am.plane_scene(alpha, shadow, uv)
    assert len(sd.alpha_masks) == 1 and sd.alpha_masks[0].alpha_kind == pkg.capi.PT_ALPHA_TEXTURE and sd.alpha_masks[0].shadow_kind == pkg.capi.PT_ALPHA_TEXTURE
    osc = oracle.scene(sd)
    try:
        am.check_plane(_tracer(osc, n_plane), alpha, shadow, uv, "oracle %s %s" % (name, "uv" if uv else "default uv"))
        o, d = am.rays(am.points(20000))                                 # the exhaustive accelerator wraps the same shapes
        tm = np.full(len(o), np.inf, np.float32)
        h, e = osc.trace_closest(o, d, tm)[0], osc.trace_closest(o, d, tm, exhaustive=True)[0]
        assert np.array_equal(h["prim"], e["prim"]) and np.array_equal(bits(h["t"]), bits(e["t"]))
    finally:
        osc.close()


def test_shadowalpha_alone_leaves_closest_hits(oracle):
    """shadowalpha without alpha: every closest-hit ray sees the plane, shadow rays pass where the mask is <= 0."""
    shadow = CASES["image16_repeat"]
    sd, n_plane = am.plane_scene(None, shadow)
    osc = oracle.scene(sd)
    try:
        am.check_plane(_tracer(osc, n_plane), am.Const(1.0), shadow, True, "oracle shadowalpha only")
    finally:
        osc.close()


def test_no_masked_scene_reaches_the_oracle_unmasked(oracle):
    """OracleScene forwards sd.alpha_masks: the same descriptor with and without them traces differently, and a bad mask is refused."""
    alpha = CASES["image16_repeat"]
    sd, n_plane = am.plane_scene(alpha, None)
    o, d = am.rays(am.points(2000))
    tm = np.full(len(o), np.inf, np.float32)
    osc = oracle.scene(sd)
    masked = osc.trace_closest(o, d, tm)[0]["prim"]
    osc.close()
    masks, sd.alpha_masks = sd.alpha_masks, []
    osc = oracle.scene(sd)
    bare = osc.trace_closest(o, d, tm)[0]["prim"]
    osc.close()
    assert np.all(bare < n_plane) and 0.2 < (masked < n_plane).mean() < 0.8
    bad = pkg.capi.pt_alpha_mask.from_buffer_copy(masks[0])
    bad.alpha_texture = 99
    sd.alpha_masks = [bad]
    with pytest.raises(AssertionError):
        oracle.scene(sd)


def test_alpha_golden_fixture(oracle):
    """The oracle's masks frozen against accidental edits (tools/make_golden.py): film, per-sample radiance of the middle tile and the ray
    counters of the committed masked fixture, bit for bit -- and the masks are in it: the same scene without them renders differently."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alpha_path_halton_32x32_4spp.npz"))
    sd = fs.scene_alpha_golden()
    sc = oracle.scene(sd)
    xyzw, cnt, _ = sc.render(threads=4)
    assert np.array_equal(bits(xyzw), bits(g["xyzw"]))
    rad = sc.radiance_samples(fs.golden_tile(sc.info))
    assert np.array_equal(bits(rad), bits(g["radiance"]))
    assert [cnt[k] for k in ("camera_rays", "regular_rays", "shadow_rays", "path_vertices")] == list(g["counters"])
    assert np.isfinite(rad).all() and rad.max() > 0 and len(np.unique(rad)) > 10
    sc.close()
    sd.alpha_masks = []
    sc = oracle.scene(sd)
    assert not np.array_equal(bits(sc.radiance_samples(fs.golden_tile(sc.info))), bits(g["radiance"]))
    sc.close()


def test_render_matrix_is_pairwise(oracle):
    """feature_scenes.ALPHA_RENDERS, the render matrix of test_gpu_alpha_mask_parity.py: every pair of values of any two of its first five
    columns (integrator with strategy, material on the masked meshes, material under them, sampler, extra) is in some row; every mask kind
    is some row's "alpha"; and the oracle renders every row, masks seen, with finite output."""
    import itertools
    rows = [((r[0], r[1]),) + tuple(r[2:6]) for r in fs.ALPHA_RENDERS]
    values = [sorted(set(r[c] for r in rows), key=str) for c in range(5)]
    assert [len(v) for v in values] == [7, 4, 4, 2, 4]
    for a, b in itertools.combinations(range(5), 2):
        missing = set(itertools.product(values[a], values[b])) - {(r[a], r[b]) for r in rows}
        assert not missing, (a, b, missing)
    assert {r[6] for r in fs.ALPHA_RENDERS} == set(fs.ALPHA_MASKS)
    assert all(r[8] is None for r in fs.ALPHA_RENDERS if r[0] == "ao")
    assert len({fs.alpha_render_name(r) for r in fs.ALPHA_RENDERS}) == len(fs.ALPHA_RENDERS)
    for r in fs.ALPHA_RENDERS:
        sd = fs.alpha_render_scene(r)
        x, cnt, _ = oracle.scene(sd).render(threads=8)
        sd.alpha_masks = []
        bare, _, _ = oracle.scene(sd).render(threads=8)
        assert np.isfinite(x).all() and cnt["camera_rays"] > 0 and not np.array_equal(x, bare), r
