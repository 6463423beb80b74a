"""Alpha masks that vary inside their triangles, on the GPU against the oracle's restatement of shapes/alphamask.rs (orc_accel.hpp,
tri_shape_intersect), bit for bit: the trace hooks -- pt_trace_closest / pt_trace_any (k_trace_batch_alpha) and pt_trace_wavefront with
mixed work items (k_trace_alpha) -- on every texture kind, wrap mode, mapping, the default uv, instance space, two masks on one mesh,
masked and unmasked triangles in one leaf at every leaf size, split method and build mode; then renders over a matrix that is pairwise
in integrator, the materials on and under the masked meshes, sampler and scene extra (feature_scenes.ALPHA_RENDERS; each mask kind at least
once) as test_gpu_features._compare holds the other features.  The float64 numpy masks of
alpha_mask_ref.py are held against the device too: that check does not go through the oracle."""
import os

import numpy as np
import pytest

import alpha_mask_ref as am
import feature_scenes as fs
from helpers import bits, pkg, random_rays, rel_l2, scenes
from test_gpu_features import _compare
from test_gpu_wavefront import _check as wavefront_check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEVICE, AUTO = pkg.capi.BVH_BUILD_HOST, pkg.capi.BVH_BUILD_DEVICE, pkg.capi.BVH_BUILD_AUTO
CASES = am.cases()
NAMES = list(CASES)


@pytest.fixture(autouse=True)
def _clean_counters(gpu_ctx):
    """Leave the session's context as the other modules expect it: counters at zero, the build mode automatic."""
    yield
    gpu_ctx.reset_counters()
    gpu_ctx.set_bvh_build(AUTO)


def hold_hooks(ctx, osc, aimed=None, n_random=100000, seed=31, inst=False):
    """The three trace hooks against the oracle.  aimed: (o, d) rays dropped onto the masked geometry; random rays through the world bound
    (axis-aligned and unnormalised directions, finite t_max, shadow-like segments) are added.  Closest hits: prim equal, t bits equal;
    occlusion equal; the wavefront kernel with continuation, shadow and probe items mixed, counters included.  inst: the scene has
    instances -- as in test_gpu_wavefront.py, the wavefront hook reports no barycentrics for a hit inside one and its probe items keep the
    inner record, so those two are left to the renders."""
    ro, rd, rt = random_rays(ctx.info, n_random, seed)
    so, sd_, st = random_rays(ctx.info, n_random, seed + 1, shadow_like=True)
    if aimed is not None:
        ao, ad = aimed
        ext = float(np.max(np.array(list(ctx.info.world_bound)[3:]) - np.array(list(ctx.info.world_bound)[:3])))
        ro, rd, rt = np.concatenate([ao, ro]), np.concatenate([ad, rd]), np.concatenate([np.full(len(ao), np.inf, np.float32), rt])
        so, sd_, st = np.concatenate([ao, so]), np.concatenate([ad * np.float32(ext), sd_]), np.concatenate([np.full(len(ao), 1.0 - 1e-4, np.float32), st])
    g = ctx.trace_closest(ro, rd, rt)
    r, _ = osc.trace_closest(ro, rd, rt)
    bad = np.flatnonzero(g["prim"] != r["prim"])
    assert bad.size == 0, ("closest prim", bad.size, ro[bad[:3]], rd[bad[:3]], g["prim"][bad[:3]], r["prim"][bad[:3]])
    hit = r["prim"] >= 0
    assert np.array_equal(bits(g["t"][hit]), bits(r["t"][hit]))
    go, oo = ctx.trace_any(so, sd_, st), osc.trace_any(so, sd_, st)[0]
    bad = np.flatnonzero(go != oo)
    assert bad.size == 0, ("any", bad.size, so[bad[:3]], sd_[bad[:3]], go[bad[:3]], oo[bad[:3]])
    # k_trace_alpha: both sets in one launch, kinds dealt in turn
    o, d, t = np.concatenate([ro, so]), np.concatenate([rd, sd_]), np.concatenate([rt, st])
    perm = np.random.default_rng(seed + 2).permutation(len(t))
    kind = np.tile(np.array([1, 2, 3, 2, 1], np.uint8), len(t) // 5 + 1)[:len(t)]
    n_hit, n_occ = wavefront_check(ctx, osc, o[perm], d[perm], t[perm], kind, probe_prims=not inst, barycentrics=not inst)
    assert len(rt) >= 100000 and len(st) >= 100000           # per hook; the wavefront launch carries both sets
    return int(hit.sum()), int(oo.sum()), n_hit, n_occ


# ---------------------------------------------------------------- hooks
@pytest.mark.parametrize("uv", [True, False], ids=["uv", "default_uv"])
@pytest.mark.parametrize("name", NAMES)
def test_plane_hooks_match_oracle_and_float64(gpu_ctx, oracle, name, uv):
    """The masked plane of alpha_mask_ref.py, alpha = the case and shadowalpha = the next one: the device equals the oracle on the 414 161
    dropped rays (texel centres and edges, uv = 0 / 1, st outside [0, 1] on both sides) and 100 000 random ones per hook, and equals the float64 numpy masks outside
    their rounding band."""
    alpha, shadow = CASES[name], CASES[NAMES[(NAMES.index(name) + 1) % len(NAMES)]]
    sd, n_plane = am.plane_scene(alpha, shadow, uv)
    gpu_ctx.upload(sd)
    osc = oracle.scene(sd)
    try:
        n = hold_hooks(gpu_ctx, osc, aimed=am.rays(am.points()))
        assert min(n) > 1000
        am.check_plane((gpu_ctx.trace_closest, gpu_ctx.trace_any, n_plane), alpha, shadow, uv, "device %s %s" % (name, "uv" if uv else "default uv"))
    finally:
        osc.close()


def _aimed(info, n=120000, seed=5):
    """Rays from above the room straight down and slanted through it: every masked surface of fs.scene_alpha lies below."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(0.0, 8.0, n), rng.uniform(0.0, 8.5, n), np.full(n, 3.5)], 1).astype(np.float32)
    d = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), np.full(n, -1.0)], 1).astype(np.float32)
    d[: n // 4, :2] = 0.0
    return o, d


@pytest.mark.parametrize("extra", [None, "instance"])
@pytest.mark.parametrize("mask", fs.ALPHA_MASKS)
def test_scene_hooks_match_oracle(gpu_ctx, oracle, mask, extra):
    """Every mask kind on the canopy, the foliage, a mesh without uv and a masked emitter -- in world space and under a rotated, non-uniformly
    scaled, mirrored instance (the masks see object space) -- with a different texture as "shadowalpha"."""
    shadow = fs.ALPHA_MASKS[(fs.ALPHA_MASKS.index(mask) + 5) % len(fs.ALPHA_MASKS)]
    sd = fs.scene_alpha(mask=mask, shadow=shadow, emitter=mask, extra=extra)
    gpu_ctx.upload(sd)
    osc = oracle.scene(sd)
    try:
        n = hold_hooks(gpu_ctx, osc, aimed=_aimed(gpu_ctx.info), inst=extra == "instance")
        assert min(n) > 1000
    finally:
        osc.close()


def interleaved_scene(split, maxnodeprims, n=400):
    """Two triangle soups in the same volume, one masked (default uv: every triangle carries the whole mask) and one not, created in
    alternating slices so that leaves mix their triangles; a masked mesh with uv among them."""
    rng = np.random.default_rng(77)
    b = fs.base(res=16, spp=1)
    b.accelerator_bvh(splitmethod=split, maxnodeprims=maxnodeprims)
    a_tex, s_tex = fs.alpha_mask_texture(b, "image16_repeat"), fs.alpha_mask_texture(b, "checker_closedform")
    b.material_matte((0.5, 0.5, 0.5))
    for k in range(4):
        c = rng.uniform(-1.0, 1.0, (n // 4, 1, 3)).astype(np.float32)
        P = (c + rng.uniform(-0.25, 0.25, (n // 4, 3, 3)).astype(np.float32)).reshape(-1, 3)
        kw = [{}, {"alpha": a_tex}, {"alpha": a_tex, "shadowalpha": s_tex}, {"shadowalpha": s_tex}][k]
        b.shape_trianglemesh(P, np.arange(len(P)), **kw)
        c = rng.uniform(-1.0, 1.0, (n // 4, 1, 3)).astype(np.float32)
        P = (c + rng.uniform(-0.25, 0.25, (n // 4, 3, 3)).astype(np.float32)).reshape(-1, 3)
        b.shape_trianglemesh(P, np.arange(len(P)))
    Pq, idx, uv = fs.leaf_quads(4, z=0.0, size=0.2)
    b.shape_trianglemesh((Pq - np.float32([4.0, 4.0, 0.0])) * np.float32(0.3), idx, uv=uv, alpha=s_tex)
    b.area_light_source_diffuse(L=(5, 5, 5))
    b.shape_trianglemesh([(-0.5, 1.9, -0.5), (0.5, 1.9, -0.5), (0.5, 1.9, 0.5), (-0.5, 1.9, 0.5)], [0, 2, 1, 0, 3, 2])
    b.no_area_light()
    return b.build()


@pytest.mark.parametrize("build", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("maxnodeprims", [1, 4, 13, 255])
@pytest.mark.parametrize("split", ["sah", "hlbvh", "middle", "equal"])
def test_interleaved_meshes_match_oracle(gpu_ctx, oracle, split, maxnodeprims, build):
    """PT_TRI_ALPHA rides in the per-mesh record flags on both build paths: leaves of 1 ... 255 primitives holding masked and unmasked
    triangles side by side, under every split method."""
    sd = interleaved_scene(split, maxnodeprims)
    gpu_ctx.set_bvh_build(build)
    gpu_ctx.upload(sd)
    osc = oracle.scene(sd)
    try:
        n = hold_hooks(gpu_ctx, osc)
        assert min(n) > 1000
        if maxnodeprims == 13:
            _, frac = _compare(gpu_ctx, osc, exact_film=True)
            assert frac == 0.0
    finally:
        osc.close()


# ---------------------------------------------------------------- renders
@pytest.mark.parametrize("row", fs.ALPHA_RENDERS, ids=[fs.alpha_render_name(r) for r in fs.ALPHA_RENDERS])
def test_masked_render_matches_oracle(gpu_ctx, oracle, row):
    """fs.ALPHA_RENDERS: pairwise over integrator, the two materials, sampler and extra; each mask kind at least once."""
    sd = fs.alpha_render_scene(row)
    assert any(m.alpha_kind == pkg.capi.PT_ALPHA_TEXTURE for m in sd.alpha_masks)
    gpu_ctx.upload(sd)
    osc = oracle.scene(sd)
    try:
        assert gpu_ctx.info.n_lights == osc.info.n_lights
        oracle.reference_panics()
        err, frac = _compare(gpu_ctx, osc, exact_film=True)
        assert frac == 0.0
        assert oracle.reference_panics() == 0
        print("%s: rel-L2 %.2e" % (fs.alpha_render_name(row), err))
    finally:
        osc.close()


def test_masked_emitter_is_sampled_everywhere_and_seen_through_its_mask(gpu_ctx, oracle):
    """Q37: the light of a masked emitter is built from the bare triangles -- the same light count, area and sampling with and without the
    mask -- while a closest-hit ray reaches it only where the mask passes (the float64 checkerboard of alpha_mask_ref.py)."""
    masked = fs.scene_alpha("directlighting", "all", emitter="checker_closedform")
    em = masked.alpha_masks[0]                             # the emitter is the first masked mesh declared: alpha only, on an area light
    assert em.alpha_kind == pkg.capi.PT_ALPHA_TEXTURE and em.shadow_kind == pkg.capi.PT_ALPHA_NONE and masked.desc.meshes[em.mesh].area_light >= 0
    prims = [t for t in range(masked.desc.n_triangles) if masked.desc.tri_mesh[t] == em.mesh]
    assert len(prims) == 2
    gpu_ctx.upload(masked)
    n_lights = gpu_ctx.info.n_lights
    # seen: rays dropped onto the emitter's parallelogram from 0.01 in front of it; uv is affine over it
    uv = np.random.default_rng(8).uniform(0.02, 0.98, (20000, 2))
    p0, e1, e2 = np.array([0.5, 7.5, 0.4]), np.array([3.0, 0.0, 0.0]), np.array([0.0, 0.7, 2.2])
    n = np.cross(e1, e2) / np.linalg.norm(np.cross(e1, e2))
    p = p0 + uv[:, :1] * e1 + uv[:, 1:] * e2
    h = gpu_ctx.trace_closest((p + 0.01 * n).astype(np.float32), np.tile((-n).astype(np.float32), (len(p), 1)), np.full(len(p), np.inf, np.float32))
    a, edge = CASES["checker_closedform"].val(uv[:, 0], uv[:, 1])
    assert edge.mean() < 0.01 and 0.3 < (a > 0).mean() < 0.7
    assert np.array_equal(np.isin(h["prim"], prims)[~edge], (a > 0)[~edge]) and np.all(h["prim"] >= 0)
    # sampled: the last light of the list is the emitter's second triangle
    u = np.random.default_rng(3).random((4096, 2), dtype=np.float32)
    ref = np.tile(np.float32([[4.0, 4.0, 0.5]]), (len(u), 1))
    light = n_lights - 1
    got = gpu_ctx.light_sample_li(light, ref, u)
    osc = oracle.scene(masked)
    want = osc.light_sample_li(light, ref, u)
    osc.close()
    bare = fs.scene_alpha("directlighting", "all", emitter="checker_closedform")
    bare.alpha_masks = [m for m in bare.alpha_masks if m.mesh != em.mesh]
    assert len(bare.alpha_masks) == len(masked.alpha_masks) - 1
    gpu_ctx.upload(bare)
    assert gpu_ctx.info.n_lights == n_lights
    plain = gpu_ctx.light_sample_li(light, ref, u)
    for x, y, z in zip(got, want, plain):
        assert np.array_equal(bits(x), bits(y)) and np.array_equal(bits(x), bits(z))
    assert (got[2] > 0).mean() > 0.9
    assert np.all(np.isin(gpu_ctx.trace_closest((p + 0.01 * n).astype(np.float32), np.tile((-n).astype(np.float32), (len(p), 1)),
                                                np.full(len(p), np.inf, np.float32))["prim"], prims))          # unmasked, it is seen everywhere


def test_alpha_golden_fixture(gpu_ctx):
    """The committed masked fixture (tools/make_golden.py, from the oracle): per-sample radiance of the middle tile bit for bit, the ray
    counters, the film weights bit for bit and its colour within tolerance -- a change to oracle and kernel together still shows."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "alpha_path_halton_32x32_4spp.npz"))
    gpu_ctx.upload(fs.scene_alpha_golden())
    rad = gpu_ctx.radiance_samples(fs.golden_tile(gpu_ctx.info))
    assert np.array_equal(bits(rad), bits(g["radiance"]))
    gpu_ctx.film_clear(); gpu_ctx.reset_counters(); gpu_ctx.render()
    c = gpu_ctx.counters()
    assert [c[k] for k in ("camera_rays", "regular_rays", "shadow_rays", "path_vertices")] == list(g["counters"])
    got = gpu_ctx.film_xyzw()
    assert np.array_equal(bits(got[..., 3]), bits(g["xyzw"][..., 3])) and rel_l2(got[..., :3], g["xyzw"][..., :3]) <= 1e-3
