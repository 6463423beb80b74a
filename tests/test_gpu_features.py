"""GPU parity on the feature-matrix scenes (tests/feature_scenes.py) and on the code paths that
need special builds or sizes: the HBM stack spill, the one-leaf scene, and BASELINE sizes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import feature_scenes as fs
from helpers import bits, pkg, random_rays, rel_l2, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compare(ctx, osc, exact_film, frac_limit=0.0, weight_tol=None):
    info = ctx.info
    o, d, tmax = random_rays(info, 30000, 21)
    g = ctx.trace_closest(o, d, tmax)
    r, _ = osc.trace_closest(o, d, tmax)
    assert np.array_equal(g["prim"], r["prim"])
    hit = r["prim"] >= 0
    assert np.array_equal(bits(g["t"][hit]), bits(r["t"][hit]))
    so, sd_, st = random_rays(info, 30000, 22, shadow_like=True)
    assert np.array_equal(ctx.trace_any(so, sd_, st), osc.trace_any(so, sd_, st)[0])
    sb = list(info.sample_bounds)
    cx, cy = (sb[0] + sb[2]) // 2, (sb[1] + sb[3]) // 2
    tile = (cx - 8, cy - 8, cx + 8, cy + 8)
    gs, rs = ctx.radiance_samples(tile), osc.radiance_samples(tile)
    frac = 1.0 - np.all(bits(gs) == bits(rs), axis=-1).mean()
    assert frac <= frac_limit, frac     # per-sample radiance: bit-identical
    ctx.film_clear(); ctx.reset_counters(); ctx.render()
    gx, grgb, gc = ctx.film_xyzw(), ctx.film_rgb(), ctx.counters()
    ox, oc, _ = osc.render(threads=8)
    orgb = osc.resolve_rgb(ox)
    if weight_tol is not None and not exact_film:
        # negative-lobed filters leave pixels whose weights cancel to almost nothing; their colour is a quotient of two rounding residues and
        # moves with the order of the film's float atomics (as it does with the reference's tile merge order): the image is compared where
        # it is conditioned, the weighted sums everywhere
        ok = np.abs(ox[..., 3]) > 1e-2 * np.abs(ox[..., 3]).max()
        err = rel_l2(grgb[ok], orgb[ok])
        assert np.abs(gx[..., :3] - ox[..., :3]).max() <= weight_tol * np.abs(ox[..., :3]).max()
    else:
        err = rel_l2(grgb, orgb)
    assert err <= 1e-3, err            # north_star tolerance; observed ~1e-7
    assert gc["camera_rays"] == oc["camera_rays"]
    for k in ("regular_rays", "shadow_rays", "path_vertices", "nodes_visited", "tris_tested"):
        assert gc[k] == oc[k], (k, gc[k], oc[k])
    if exact_film:
        assert np.array_equal(bits(gx[..., 3]), bits(ox[..., 3]))
    elif weight_tol is None:      # wide filters: float atomics, summation order differs in the last bits
        assert np.allclose(gx[..., 3], ox[..., 3], rtol=1e-5, atol=1e-6)
    else:      # ... and with negative lobes (Mitchell, sinc) a pixel's weights cancel: the order shows relative to the largest weight, not to the sum
        assert np.abs(gx[..., 3] - ox[..., 3]).max() <= weight_tol * np.abs(ox[..., 3]).max()
    return err, frac


@pytest.mark.parametrize("name,make,exact", [
    ("attributes", fs.scene_attributes, True),
    ("materials_spatial", lambda: fs.scene_materials_lights("spatial"), True),
    ("materials_power", lambda: fs.scene_materials_lights("power"), True),
    ("materials_uniform", lambda: fs.scene_materials_lights("uniform"), True),
    ("lens_gaussian", lambda: fs.scene_camera_film("gaussian"), False),
    ("lens_mitchell", lambda: fs.scene_camera_film("mitchell"), False),
    ("lens_triangle", lambda: fs.scene_camera_film("triangle"), False),
    ("lens_sinc", lambda: fs.scene_camera_film("sinc"), False),
    ("accel_middle_1", lambda: fs.scene_accel("middle", 1), True),
    ("accel_equal_8", lambda: fs.scene_accel("equal", 8), True),
    ("accel_sah_2", lambda: fs.scene_accel("sah", 2), True),
    ("accel_middle_16", lambda: fs.scene_accel("middle", 16), True),     # leaves of more than 8 triangles: k_trace_seq
    ("accel_hlbvh_4", lambda: fs.scene_accel("hlbvh", 4), True),
    ("accel_hlbvh_1", lambda: fs.scene_accel("hlbvh", 1), True),
    # analytic spheres (shapes/sphere.rs) as objects and as lights, next to triangles
    ("spheres_spatial", lambda: fs.scene_spheres("spatial"), True),
    ("spheres_power_hlbvh", lambda: fs.scene_spheres("power", split="hlbvh"), True),
    ("spheres_uniform_halton", lambda: fs.scene_spheres("uniform", split="middle", sampler="halton"), True),
    ("sphere_lights_only", lambda: fs.scene_spheres("spatial", lights_only=True), True),
    # procedural textures on material parameters, filtered with the camera ray's differentials
    ("textures_closedform", lambda: fs.scene_textures(), True),
    ("textures_point_halton", lambda: fs.scene_textures(sampler="halton", aamode="none"), True),
    ("textures_thin_lens", lambda: fs.scene_textures(lens=True), True),
    ("roughness_textures", lambda: fs.scene_roughness_textures(), True),
    ("roughness_textures_halton", lambda: fs.scene_roughness_textures(sampler="halton", spp=6), True),
    ("textures_noise", lambda: fs.scene_noise_textures(), True),
    ("textures_noise_halton", lambda: fs.scene_noise_textures(sampler="halton"), True),
    # object instancing: TransformedPrimitive over per-object accelerators
    ("instances_sah", lambda: fs.scene_instances(), True),
    ("instances_hlbvh_halton", lambda: fs.scene_instances(split="hlbvh", sampler="halton"), True),
    ("imagemaps_ewa", lambda: fs.scene_imagemaps(), True),
    ("imagemaps_trilinear_halton", lambda: fs.scene_imagemaps(trilinear=True, sampler="halton"), True),
    ("imagemaps_ewa_thin_lens", lambda: fs.scene_imagemaps(lens=True), True),
    ("bump", lambda: fs.scene_bump(), True),
    ("bump_thin_lens", lambda: fs.scene_bump(lens=True), True),
])
def test_feature_scene(gpu_ctx, oracle, name, make, exact):
    sd = make()
    osc = oracle.scene(sd)
    gpu_ctx.upload(sd)
    err, frac = _compare(gpu_ctx, osc, exact)
    print("\n[%s] image rel-L2 %.2e, samples not bit-identical %.3f%%" % (name, err, 100 * frac))
    osc.close()


def test_single_leaf_scene(gpu_ctx, oracle):
    """n <= maxnodeprims: the whole scene is one leaf and the root reference is a leaf."""
    b = fs.base(res=16, spp=2)
    b.area_light_source_diffuse(L=(5, 5, 5), twosided=True)
    scenes._quad(b, (-1, -1, 2), (1, -1, 2), (1, 1, 2), (-1, 1, 2))
    sd = b.build()
    osc = oracle.scene(sd)
    gpu_ctx.upload(sd)
    assert gpu_ctx.info.n_nodes == 0 and gpu_ctx.info.n_leaves == 1
    _compare(gpu_ctx, osc, True)
    osc.close()


def test_no_lights_renders_black(gpu_ctx, oracle):
    """create_light_sample_distribution fails without lights and li() returns zero (path.rs:71-74)."""
    b = fs.base(res=16, spp=2)
    scenes._quad(b, (-1, -1, 2), (1, -1, 2), (1, 1, 2), (-1, 1, 2))
    sd = b.build()
    osc = oracle.scene(sd)
    gpu_ctx.upload(sd)
    gpu_ctx.film_clear(); gpu_ctx.render()
    gx = gpu_ctx.film_xyzw()
    ox, _, _ = osc.render(threads=2)
    assert np.array_equal(bits(gx), bits(ox))
    assert gx[..., :3].max() == 0.0 and gx[..., 3].min() > 0
    osc.close()


def test_stack_spill_build(oracle, tmp_path):
    """Force the HBM spill path of the traversal stack: a build with a 3-entry LDS stack must
    give the same hits and counters as the oracle."""
    so = tmp_path / "libpbrtgpu_stack3.so"
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "pbrt-r3_amd", "csrc"), "OUT=%s" % so, "EXTRA=-DPT_LDS_STACK=3", str(so)])
    lib = pkg.capi.load_library(str(so))
    ctx = pkg.Context(0, lib=lib)
    sd = scenes.rt1m(20000, res=32, spp=2)
    osc = oracle.scene(sd)
    ctx.upload(sd)
    o, d, tmax = random_rays(ctx.info, 40000, 31)
    ctx.reset_counters()
    g = ctx.trace_closest(o, d, tmax)
    gc = ctx.counters()
    r, oc = osc.trace_closest(o, d, tmax)
    assert np.array_equal(g["prim"], r["prim"])
    assert gc["nodes_visited"] == oc["nodes_visited"] and gc["tris_tested"] == oc["tris_tested"]
    # the same rays as mixed work items through the wavefront kernel (its predicated pushes take the spill-aware form)
    from test_gpu_wavefront import _check
    kind = (1 + np.arange(len(tmax)) % 3).astype(np.uint8)
    _check(ctx, osc, o, d, tmax, kind)
    ctx.film_clear(); ctx.render()
    ox, _, _ = osc.render(threads=8)
    assert rel_l2(ctx.film_rgb(), osc.resolve_rgb(ox)) <= 1e-3
    osc.close()
    # ... and rays that enter instances with their way back (the rest of the leaf, the slab interval, the marker) in the HBM part of the stack
    sd = fs.scene_instance_swarm("sah", 4, n_inst=12, res=32, spp=4)
    osc = oracle.scene(sd)
    ctx.upload(sd)
    _compare(ctx, osc, exact_film=True)
    ctx.close(); osc.close()


def test_golden_fixtures(gpu_ctx):
    """Committed oracle fixtures (tools/make_golden.py): camera rays / closest hits exact, film within tolerance."""
    G = os.path.join(ROOT, "tests", "golden")
    gpu_ctx.upload(scenes.cornell_box(res=32, spp=8))
    g = np.load(os.path.join(G, "cornell_32x32_8spp_rays.npz"))
    o, d, pf = gpu_ctx.generate_camera_rays(g["pixel"], np.zeros(len(g["pixel"]), np.uint32))
    assert np.array_equal(bits(o), bits(g["o"])) and np.array_equal(bits(d), bits(g["d"])) and np.array_equal(bits(pf), bits(g["p_film"]))
    h = gpu_ctx.trace_closest(o, d, np.full(len(o), np.inf, np.float32))
    assert np.array_equal(h["prim"], g["prim"]) and np.array_equal(bits(h["t"]), bits(g["t"]))
    assert np.array_equal(bits(h["b0"]), bits(g["b0"])) and np.array_equal(bits(h["b1"]), bits(g["b1"]))
    gpu_ctx.film_clear(); gpu_ctx.render()
    want = np.load(os.path.join(G, "cornell_32x32_8spp_xyzw.npy"))
    got = gpu_ctx.film_xyzw()
    assert np.array_equal(bits(got[..., 3]), bits(want[..., 3]))
    assert rel_l2(got[..., :3], want[..., :3]) <= 1e-3
    gpu_ctx.upload(scenes.rt1m(2000, res=32, spp=4))
    gpu_ctx.film_clear(); gpu_ctx.render()
    want = np.load(os.path.join(G, "rt2k_32x32_4spp_xyzw.npy"))
    assert rel_l2(gpu_ctx.film_xyzw()[..., :3], want[..., :3]) <= 1e-3
    # material lobes + Halton + HLBVH
    sd3 = fs.scene_materials_render(["plastic", "mirror", "glass"], spp=6, sampler="halton")
    sd3.desc.split_method = 1
    gpu_ctx.upload(sd3)
    gpu_ctx.film_clear(); gpu_ctx.render()
    want = np.load(os.path.join(G, "materials_halton_40x40_6spp_xyzw.npy"))
    got = gpu_ctx.film_xyzw()
    assert np.array_equal(bits(got[..., 3]), bits(want[..., 3]))
    assert rel_l2(got[..., :3], want[..., :3]) <= 1e-3
    gpu_ctx.upload(fs.scene_materials_render(["metal", "uber", "substrate"], spp=8))
    sb = list(gpu_ctx.info.sample_bounds)
    rad = gpu_ctx.radiance_samples((sb[0] + 14, sb[1] + 14, sb[0] + 26, sb[1] + 26))
    assert np.array_equal(bits(rad), bits(np.load(os.path.join(G, "materials_sobol_40x40_8spp_samples.npy"))))


def test_deferred_store_build_is_bit_exact(oracle, tmp_path):
    """The textured / instanced shading kernels store each output where it is made; the plain ones hold all stores back to the end of the
    iteration.  Round 2 found the held-back form of the wide kernels wrong for a few samples per film and parked it; round 3 traced it to
    a register-allocation miscompile (hipcc 7.2, -O2 and -O3: profiles/r03_deferred_store_miscompile.md) that hit paths surviving
    Russian roulette (bounces > 3), and removed the trigger in the source (an opaque zero in the continuation direction's .w).  This test
    builds the held-back variant (-DPT_DEFER_WIDE=1) and holds it to the oracle on the seven scenes that showed the divergence, every
    camera sample of the film, at the depth where roulette runs -- both placements must be bit-exact."""
    so = tmp_path / "libpbrtgpu_defer.so"
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "pbrt-r3_amd", "csrc"), "OUT=%s" % so, "EXTRA=-DPT_DEFER_WIDE=1", str(so)])
    lib = pkg.capi.load_library(str(so))
    ctx = pkg.Context(0, lib=lib)
    seven = [lambda: fs.scene_textures(), lambda: fs.scene_textures(lens=True), lambda: fs.scene_roughness_textures(), lambda: fs.scene_instances(),
             lambda: fs.scene_instances(split="hlbvh", sampler="halton"), lambda: fs.scene_bump(), lambda: fs.scene_bump(lens=True)]
    roulette_ran = 0
    for make in seven:
        sd = make()
        sd.desc.max_depth = 5            # the first depth at which a vertex with bounces > 3 is shaded: Russian roulette runs
        osc = oracle.scene(sd)
        ctx.upload(sd)
        sb = list(ctx.info.sample_bounds)
        g, r = ctx.radiance_samples(tuple(sb)), osc.radiance_samples(tuple(sb))
        assert np.array_equal(bits(g), bits(r))
        # the depth matters: the same film at maxdepth 4 (no vertex with bounces > 3 is shaded) must differ from it somewhere
        sd4 = make()
        sd4.desc.max_depth = 4
        o4 = oracle.scene(sd4)
        roulette_ran += int((bits(o4.radiance_samples(tuple(sb))) != bits(r)).any())
        o4.close(); osc.close()
    assert roulette_ran >= 5
    ctx.close()


@pytest.mark.parametrize("name", ["directlighting_all_ns3_40x40_4spp", "whitted_depth4_40x40_4spp", "ao_16cos_cornell_32x32_4spp"])
def test_golden_fixtures_other_integrators(gpu_ctx, name):
    """The committed fixtures of the directlighting / whitted / ao integrators (tools/make_golden.py, from the oracle): per-sample radiance
    of the middle tile bit for bit, the ray counters, the film within tolerance."""
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    gpu_ctx.upload(fs.GOLDEN_INTEGRATORS[name]())
    rad = gpu_ctx.radiance_samples(fs.golden_tile(gpu_ctx.info))
    assert np.array_equal(bits(rad), bits(g["radiance"]))
    gpu_ctx.film_clear(); gpu_ctx.reset_counters(); gpu_ctx.render()
    c = gpu_ctx.counters()
    assert [c[k] for k in ("camera_rays", "regular_rays", "shadow_rays", "path_vertices")] == list(g["counters"])
    got = gpu_ctx.film_xyzw()
    assert np.array_equal(bits(got[..., 3]), bits(g["xyzw"][..., 3])) and rel_l2(got[..., :3], g["xyzw"][..., :3]) <= 1e-3


def test_baseline_size_properties(gpu_ctx, oracle):
    """BASELINE.json full size (RT1M: 1M triangles, 1024x1024): size-independent checks that need no
    full CPU render -- camera rays of a pixel sample exact, closest hits of 200k rays exact against the
    oracle, film weights = spp inside the image, disjoint tile subsets add up, energy non-negative."""
    sd = scenes.rt1m(1000000, res=1024, spp=4)
    osc = oracle.scene(sd)
    gpu_ctx.upload(sd)
    assert list(gpu_ctx.info.sample_bounds) == [-1, -1, 1025, 1025]
    rng = np.random.default_rng(5)
    px = rng.integers(-1, 1025, (100000, 2)).astype(np.int32)
    si = rng.integers(0, 4, 100000).astype(np.uint32)
    go, gd, _ = gpu_ctx.generate_camera_rays(px, si)
    oo, od, _ = osc.generate_camera_rays(px, si)
    assert np.array_equal(bits(go), bits(oo)) and np.array_equal(bits(gd), bits(od))
    ro, rd, rt = random_rays(gpu_ctx.info, 100000, 6)
    o = np.concatenate([go, ro]); d = np.concatenate([gd, rd]); t = np.concatenate([np.full(len(go), np.inf, np.float32), rt])
    gpu_ctx.reset_counters()
    g = gpu_ctx.trace_closest(o, d, t)
    gc = gpu_ctx.counters()
    r, oc = osc.trace_closest(o, d, t)
    assert np.array_equal(g["prim"], r["prim"]) and np.array_equal(bits(g["t"]), bits(r["t"]))
    assert gc["nodes_visited"] == oc["nodes_visited"] and gc["tris_tested"] == oc["tris_tested"]
    gpu_ctx.film_clear(); gpu_ctx.render()
    full = gpu_ctx.film_xyzw()
    # every pixel receives its own 4 samples except where a sample sits exactly on a pixel edge and is
    # shared with the neighbours (normalised footprint, quirk Q1): weights stay near spp and sum to ~spp*pixels
    assert np.isfinite(full).all() and full[..., :3].min() >= -1e-6
    assert full[..., 3].min() >= 2.0 and abs(float(full[..., 3].mean()) - 4.0) < 0.01
    tiles = scenes.all_tiles(gpu_ctx.info)
    gpu_ctx.film_clear(); gpu_ctx.render(tiles[0::2]); gpu_ctx.render(tiles[1::2])
    both = gpu_ctx.film_xyzw()
    assert np.allclose(both, full, rtol=4e-6, atol=1e-7)
    # one tile of the full-size scene against the oracle, sample by sample
    tile = (512, 512, 528, 528)
    gs, rs = gpu_ctx.radiance_samples(tile), osc.radiance_samples(tile)
    assert np.array_equal(bits(gs), bits(rs))
    osc.close()


def test_cli_renders_pbrt_file(oracle, tmp_path):
    """`pbrt_gpu -i scene.pbrt` (the `pbrt-r3 -i` counterpart): parse -> upload -> render -> PFM,
    compared with the oracle's render of the same parsed scene."""
    exe = os.path.join(ROOT, "pbrt-r3_amd", "csrc", "pbrt_gpu")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbrt-r3_amd", "csrc"), "pbrt_gpu"])
    scene = os.path.join(ROOT, "tests", "scenes", "cornell.pbrt")
    out = tmp_path / "cornell.pfm"
    r = subprocess.run([exe, "-i", scene, "--outfile", str(out), "--pixelsamples", "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    header, rest = raw.split(b"\n", 3)[:3], raw.split(b"\n", 3)[3]
    assert header[0] == b"PF" and header[1] == b"64 64"
    img = np.frombuffer(rest, "<f4").reshape(64, 64, 3)[::-1]
    ps = pkg.capi.ParsedScene(filename=scene)
    ps.set_pixelsamples(8)
    osc = oracle.scene(ps)
    ox, _, _ = osc.render(threads=8)
    assert rel_l2(img, osc.resolve_rgb(ox)) <= 1e-3
    osc.close()


def test_pbrt_text_with_ply_spectra_and_materials(gpu_ctx, oracle, tmp_path):
    """Front end -> device for everything added after the first slice: Halton (no Sampler line: the reference's
    default), a gzip PLY mesh, metal with its copper defaults, glass, substrate, a blackbody light, HLBVH,
    the sinc filter.  Per-sample radiance must equal the oracle's on the same flattened scene."""
    import gzip, struct
    rng = np.random.default_rng(9)
    # an icosphere-ish blob as binary little-endian PLY with normals
    nt, nphi = 8, 12
    P, N, F = [], [], []
    for t in range(nt + 1):
        th = np.pi * t / nt
        for k in range(nphi):
            ph = 2 * np.pi * k / nphi
            n = np.array([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)], np.float32)
            P.append(n * 0.8); N.append(n)
    for t in range(nt):
        for k in range(nphi):
            a, b = t * nphi + k, t * nphi + (k + 1) % nphi
            F.append((a, b, b + nphi, a + nphi))
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
           "property float nx\nproperty float ny\nproperty float nz\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(P), len(F)))
    body = b"".join(struct.pack("<6f", *p, *n) for p, n in zip(P, N)) + b"".join(struct.pack("<B4i", 4, *f) for f in F)
    gzip.open(tmp_path / "blob.ply.gz", "wb").write(hdr.encode() + body)
    text = '''
    LookAt 0 0 -6.5  0 0 0  0 1 0
    Camera "perspective" "float fov" 40
    Film "image" "integer xresolution" 40 "integer yresolution" 40
    PixelFilter "sinc" "float xwidth" 2 "float ywidth" 2
    Integrator "path" "integer maxdepth" 6
    Accelerator "bvh" "string splitmethod" "hlbvh"
    WorldBegin
      AttributeBegin
        AreaLightSource "diffuse" "blackbody L" [5500 12]
        Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0.6 1.99 -0.6  0.6 1.99 0.6  -0.6 1.99 0.6  -0.6 1.99 -0.6]
      AttributeEnd
      Material "matte" "rgb Kd" [0.7 0.7 0.7]
      Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [2 -2 -2  -2 -2 -2  -2 -2 2  2 -2 2]
      Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [2 -2 2  -2 -2 2  -2 2 2  2 2 2]
      Material "substrate" "rgb Kd" [0.6 0.2 0.2]
      Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -2 2  -2 -2 -2  -2 2 -2  -2 2 2]
      Material "glass" "float eta" 1.45
      Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [2 -2 -2  2 -2 2  2 2 2  2 2 -2]
      AttributeBegin
        Material "metal" "float roughness" 0.08
        Translate -0.3 -1.1 0.2
        Shape "plymesh" "string filename" "blob.ply.gz"
      AttributeEnd
    WorldEnd
    '''
    ps = pkg.capi.ParsedScene(text=text, work_dir=str(tmp_path))
    d = ps.desc
    assert d.sampler == pkg.capi.PT_SAMPLER_HALTON and d.spp == 16 and d.split_method == 1
    assert d.n_triangles == 2 + 8 + 2 * len(F) - 2 * nphi          # the pole rows yield one zero-area triangle per quad (dropped, triangle.rs:726)
    osc = oracle.scene(ps)
    gpu_ctx.upload(ps)
    sb = list(gpu_ctx.info.sample_bounds)
    tile = (sb[0] + 8, sb[1] + 8, sb[0] + 36, sb[1] + 36)
    g, r = gpu_ctx.radiance_samples(tile), osc.radiance_samples(tile)
    assert r.sum() > 0
    same = np.all(bits(g) == bits(r), axis=-1)
    assert same.all(), float(1 - same.mean())
    gpu_ctx.film_clear(); gpu_ctx.render()
    ox, _, _ = osc.render(threads=8)
    assert rel_l2(gpu_ctx.film_rgb(), osc.resolve_rgb(ox)) <= 1e-3
    osc.close()


def test_killeroo_simple_shaped_scene(gpu_ctx, oracle, tmp_path):
    """BASELINE config 4 names pbrt-v3's killeroo-simple.pbrt, which is not in this tree; this scene has its
    shape: Halton sampler, a black-matte *sphere* area light far above two large uv-mapped quads,
    two instances of an Included mesh with vertex normals under Scale / Rotate / Translate, plastic materials given as
    "color" parameters, default integrator depth.  Front end -> device must equal front end -> oracle per sample."""
    (tmp_path / "geometry").mkdir()
    P, N, UV, idx = fs.uv_sphere((0, 0, 0), 60.0, nt=10, nphi=14)
    P[:, 2] *= 1.6                                     # an elongated blob standing in for the killeroo mesh
    with open(tmp_path / "geometry" / "killeroo.pbrt", "w") as f:
        f.write('Shape "trianglemesh" "integer indices" [%s]\n "point P" [%s]\n "normal N" [%s]\n' % (
            " ".join(map(str, idx)), " ".join("%.9g" % v for v in P.reshape(-1)), " ".join("%.9g" % v for v in N.reshape(-1))))
    text = '''
    LookAt 400 20 30   0 63 -110   0 0 1
    Rotate -5 0 0 1
    Camera "perspective" "float fov" [39]
    Film "image" "integer xresolution" [56] "integer yresolution" [56] "string filename" "killeroo-simple.exr"
    Sampler "halton" "integer pixelsamples" [8]
    Integrator "path"
    WorldBegin
    AttributeBegin
      Material "matte" "color Kd" [0 0 0]
      Translate 150 0 20
      Translate 0 120 0
      AreaLightSource "area" "color L" [2000 2000 2000] "integer nsamples" [8]
      Shape "sphere" "float radius" [3]
    AttributeEnd
    AttributeBegin
      Material "matte" "color Kd" [.5 .5 .8]
      Translate 0 0 -140
      Shape "trianglemesh" "point P" [ -1000 -1000 0 1000 -1000 0 1000 1000 0 -1000 1000 0 ]
          "float uv" [ 0 0 5 0 5 5 0 5 ] "integer indices" [ 0 1 2 2 3 0]
      Shape "trianglemesh" "point P" [ -400 -1000 -1000   -400 1000 -1000   -400 1000 1000 -400 -1000 1000 ]
          "float uv" [ 0 0 5 0 5 5 0 5 ] "integer indices" [ 0 1 2 2 3 0]
    AttributeEnd
    AttributeBegin
      Scale .5 .5 .5
      Rotate -60 0 0 1
      Material "plastic" "color Kd" [.4 .2 .2] "color Ks" [.5 .5 .5] "float roughness" [.025]
      Translate 100 200 -140
      Include "geometry/killeroo.pbrt"
      Material "plastic" "color Ks" [.3 .3 .3] "color Kd" [.4 .5 .4] "float roughness" [.15]
      Translate -200 0 0
      Include "geometry/killeroo.pbrt"
    AttributeEnd
    WorldEnd
    '''
    ps = pkg.capi.ParsedScene(text=text, work_dir=str(tmp_path))
    d = ps.desc
    assert d.sampler == pkg.capi.PT_SAMPLER_HALTON and d.spp == 8 and d.max_depth == 5
    assert d.n_spheres == 1 and d.spheres[0].before_triangle == 0 and d.spheres[0].area_light == 0
    assert d.n_triangles > 400 and ps.output_filename == "killeroo-simple.exr"
    osc = oracle.scene(ps)
    gpu_ctx.upload(ps)
    assert gpu_ctx.info.n_lights == 1
    sb = list(gpu_ctx.info.sample_bounds)
    tile = (sb[0] + 12, sb[1] + 12, sb[0] + 44, sb[1] + 44)
    g, r = gpu_ctx.radiance_samples(tile), osc.radiance_samples(tile)
    assert r.sum() > 0
    same = np.all(bits(g) == bits(r), axis=-1)
    assert same.all(), float(1 - same.mean())
    gpu_ctx.film_clear(); gpu_ctx.reset_counters(); gpu_ctx.render()
    ox, oc, _ = osc.render(threads=8)
    gc = gpu_ctx.counters()
    assert rel_l2(gpu_ctx.film_rgb(), osc.resolve_rgb(ox)) <= 1e-3
    for k in ("regular_rays", "shadow_rays", "path_vertices", "nodes_visited", "tris_tested"):
        assert gc[k] == oc[k], (k, gc[k], oc[k])
    osc.close()


def test_pbrt_text_with_textures(gpu_ctx, oracle):
    """Texture directives -> pt_texture nodes -> device evaluation with camera-ray differentials, against the oracle on the
    same flattened scene."""
    ps = pkg.capi.ParsedScene(text=fs.TEXTURED_PBRT)
    assert ps.desc.n_textures == 10
    osc = oracle.scene(ps)
    gpu_ctx.upload(ps)
    sb = list(gpu_ctx.info.sample_bounds)
    tile = (sb[0] + 2, sb[1] + 2, sb[0] + 30, sb[1] + 30)
    g, r = gpu_ctx.radiance_samples(tile), osc.radiance_samples(tile)
    assert r.sum() > 0
    same = np.all(bits(g) == bits(r), axis=-1)
    assert same.all(), float(1 - same.mean())
    osc.close()


def test_pbrt_text_with_imagemap(gpu_ctx, oracle, tmp_path):
    """Texture "imagemap" end to end: a 13 x 6 PNG (resampled to 16 x 8, inverse gamma) on Kd with EWA filtering, a float
    PFM as a trilinear bump map; front end -> device against front end -> oracle."""
    from test_image_textures import write_png
    rng = np.random.default_rng(21)
    write_png(tmp_path / "tiles.png", rng.integers(0, 256, (6, 13, 3)))
    g = fs.test_image(8, 8, 1, seed=4)[..., 0]
    with open(tmp_path / "height_bump.pfm", "wb") as f:
        f.write(b"Pf\n8 8\n-1.0\n")
        f.write(g.astype("<f4").tobytes())
    text = '''
    LookAt 0 0 -6.5  0 0 0  0 1 0
    Camera "perspective" "float fov" 40
    Film "image" "integer xresolution" 40 "integer yresolution" 40
    Sampler "sobol" "integer pixelsamples" 4
    Integrator "path" "integer maxdepth" 4
    WorldBegin
      AttributeBegin
        AreaLightSource "diffuse" "rgb L" [10 9 8]
        Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0.5 1.99 -0.5  0.5 1.99 0.5  -0.5 1.99 0.5  -0.5 1.99 -0.5]
      AttributeEnd
      Texture "tiles" "spectrum" "imagemap" "string filename" "tiles.png" "float uscale" 2 "float vscale" 2
      Texture "h" "float" "imagemap" "string filename" "height_bump.pfm" "bool trilinear" "true" "float scale" 0.1 "float uscale" 3 "float vscale" 3
      Material "matte" "texture Kd" "tiles" "texture bumpmap" "h"
      Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [2 -2 -2  -2 -2 -2  -2 -2 2  2 -2 2]
      Material "plastic" "texture Kd" "tiles"
      Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [2 -2 2  -2 -2 2  -2 2 2  2 2 2] "float uv" [0 0 1 0 1 1 0 1]
    WorldEnd
    '''
    ps = pkg.capi.ParsedScene(text=text, work_dir=str(tmp_path))
    d = ps.desc
    assert d.n_images == 2 and (d.images[0].width, d.images[0].height, d.images[0].channels) == (16, 8, 3) and d.images[1].channels == 1
    osc = oracle.scene(ps)
    gpu_ctx.upload(ps)
    sb = list(gpu_ctx.info.sample_bounds)
    tile = (sb[0] + 4, sb[1] + 4, sb[0] + 38, sb[1] + 38)
    g_, r_ = gpu_ctx.radiance_samples(tile), osc.radiance_samples(tile)
    assert r_.sum() > 0
    same = np.all(bits(g_) == bits(r_), axis=-1)
    assert same.all(), float(1 - same.mean())
    osc.close()


def test_pass_structure_does_not_change_the_film(gpu_ctx):
    """The pool size only decides how the samples are cut into passes / pixel chunks (render_tiles): a film rendered
    in 1 pass, in 3 unequal-looking passes (7 spp -> 3,2,2) and in pixel chunks must agree -- bit for bit where a
    sample's footprint is its own pixel (sample-ordered sums), to float-atomic order elsewhere."""
    sd = scenes.rt1m(3000, res=300, spp=3, max_depth=4, sampler="halton")        # 302 x 302 = 91 204 sample pixels
    gpu_ctx.upload(sd)
    films = []
    try:
        for pool in ("67108864", "200000", "65536"):        # one pass | 2 spp per pass -> passes of 2 and 1 | two pixel chunks x 1 spp
            os.environ["PBRTGPU_POOL_PATHS"] = pool
            gpu_ctx.film_clear(); gpu_ctx.reset_counters(); gpu_ctx.render()
            films.append((gpu_ctx.film_xyzw().copy(), gpu_ctx.counters()))
    finally:
        os.environ.pop("PBRTGPU_POOL_PATHS", None)
    (a, ca), (b, cb), (c, cc) = films
    for k in ("camera_rays", "regular_rays", "shadow_rays", "nodes_visited", "tris_tested", "path_vertices"):
        assert ca[k] == cb[k] == cc[k], k
    assert cb["trace_launches"] > ca["trace_launches"]
    for other in (b, c):
        assert np.array_equal(bits(a[..., 3]), bits(other[..., 3]))
        same = np.all(bits(a) == bits(other), axis=-1)
        assert same.mean() > 0.9 and rel_l2(other, a) < 1e-6


@pytest.mark.parametrize("split", ["sah", "hlbvh"])
def test_crown_class_3p5m_triangles(gpu_ctx, oracle, split):
    """BASELINE config 5's scale (crown: ~3.5 M triangles, deep BVH) with the stand-in geometry -- the real asset is not in this
    image.  Both builders; tree size equal to the oracle's; one 16x16 tile of per-sample radiance bit-identical; 300 k mixed
    work items through the wavefront traversal kernel with equal hits and node / triangle counters."""
    from test_gpu_wavefront import _check, _rays
    sd = scenes.rt1m(3500000, res=256, spp=8, max_depth=8)
    sd.desc.split_method = {"sah": 0, "hlbvh": 1}[split]
    gpu_ctx.upload(sd)
    osc = oracle.scene(sd)
    info = gpu_ctx.info
    assert (osc.info.n_nodes, osc.info.n_leaves) == (info.n_nodes, info.n_leaves)
    sb = list(info.sample_bounds)
    tile = (sb[0] + 120, sb[1] + 120, sb[0] + 136, sb[1] + 136)
    g, r = gpu_ctx.radiance_samples(tile), osc.radiance_samples(tile)
    assert r.sum() > 0 and np.array_equal(bits(g), bits(r))
    o, d, t, kind = _rays(gpu_ctx, osc, 300007, 77)
    n_hit, n_occ = _check(gpu_ctx, osc, o, d, t, kind)
    assert n_hit > 10000 and n_occ > 10000
    osc.close()


def _mesh_light_scene(n_side=32, res=12, spp=1, depth=2):
    """A room lit by ONE emissive mesh of 2 n_side^2 triangles -- 2 048 lights: the dense 64^3 light grid would be 4.3 GB of tables."""
    b = fs.base(res=res, spp=spp, depth=depth)
    b.integrator_path(maxdepth=depth, lightsamplestrategy="spatial")
    fs.room(b)
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=(3, 3, 2.5))
    xs = np.linspace(-1.5, 1.5, n_side + 1, dtype=np.float32)
    P = [(float(x), 1.9, float(z)) for z in xs for x in xs]
    idx = []
    for j in range(n_side):
        for i in range(n_side):
            a = j * (n_side + 1) + i
            idx += [a, a + 1, a + n_side + 2, a, a + n_side + 2, a + n_side + 1]
    b.shape_trianglemesh(P, idx)
    b.no_area_light()
    return b.build()


@pytest.mark.parametrize("name,make", [("cornell", lambda: scenes.cornell_box(res=48, spp=8)), ("materials", lambda: fs.scene_materials_lights("spatial")),
                                       ("spheres", lambda: fs.scene_spheres("spatial")), ("instances", lambda: fs.scene_instances())])
def test_lazy_light_grid_is_the_dense_grid(oracle, monkeypatch, name, make):
    """The light grid filled voxel by voxel on first touch, as the reference fills its hash table (spatial.rs:199-260) -- what scenes with
    thousands of lights get instead of the dense grid -- forced on for small scenes (PBRTGPU_LIGHT_GRID_DENSE_MAX=0): per-sample radiance, film
    and every counter are still the oracle's, bit for bit (a voxel's tables depend on the voxel alone)."""
    monkeypatch.setenv("PBRTGPU_LIGHT_GRID_DENSE_MAX", "0")
    sd = make()
    ctx = pkg.Context(0)
    try:
        ctx.upload(sd)
        osc = oracle.scene(sd)
        _compare(ctx, osc, exact_film=True)
        osc.close()
    finally:
        ctx.close()


def test_mesh_light_of_two_thousand_triangles_uses_the_lazy_grid(oracle):
    """2 048 emissive triangles: the dense grid (64 x 64 x 64 voxels x 16 KB) would be 4.3 GB and is not made; rows appear for the voxels the
    frame's hits fall in.  Per-sample radiance of the whole (small) film bit-identical to the oracle, counters equal."""
    sd = _mesh_light_scene()
    ctx = pkg.Context(0)
    try:
        info = ctx.upload(sd)
        assert info.n_lights == 2050          # the mesh + the room's own quad
        osc = oracle.scene(sd)
        sb = list(info.sample_bounds)
        tile = (sb[0], sb[1], sb[2], sb[3])
        g, r = ctx.radiance_samples(tile), osc.radiance_samples(tile)
        assert r.sum() > 0 and np.array_equal(bits(g), bits(r))
        ctx.film_clear(); ctx.reset_counters(); ctx.render()
        gc = ctx.counters()
        ox, oc, _ = osc.render(threads=8)
        for k in ("camera_rays", "regular_rays", "shadow_rays", "nodes_visited", "tris_tested", "path_vertices"):
            assert gc[k] == oc[k], (k, gc[k], oc[k])
        assert rel_l2(ctx.film_xyzw(), ox) < 1e-6
        osc.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["always", "trial"])
@pytest.mark.parametrize("name,make", [("cornell", lambda: scenes.cornell_box(res=64, spp=16)), ("materials", lambda: fs.scene_materials_lights("spatial")),
                                       ("rt20k", lambda: scenes.rt1m(20000, res=48, spp=8, max_depth=6)), ("textures", lambda: fs.scene_textures())])
def test_far_traversal_kernel_changes_nothing(oracle, monkeypatch, name, make, mode):
    """k_trace_far -- a lane pair fetches its two nodes together, for scenes whose rays miss the caches -- forced on (PBRTGPU_TRACE_FAR=1), and the
    timed trial that picks it per scene (forced to run on these small scenes: bounce 1 of the first pass traced twice, once by each kernel,
    counters put back): per-sample radiance, film and every counter are the oracle's either way -- who fetches a row changes no result."""
    if mode == "always":
        monkeypatch.setenv("PBRTGPU_TRACE_FAR", "1")
    else:
        monkeypatch.setenv("PBRTGPU_TRACE_FAR_MIN_BYTES", "0")
    sd = make()
    ctx = pkg.Context(0)
    try:
        ctx.upload(sd)
        osc = oracle.scene(sd)
        _compare(ctx, osc, exact_film=True)
        osc.close()
    finally:
        ctx.close()


LOCAL_SORT_SCENES = {
    "textures": lambda: fs.scene_textures(),
    "sphere_lit_mixed": lambda: fs.scene_sphere_lit_mixed(),
    # textured and WITHOUT an analytic shape: the scenes whose local sort had kernels of its own (a texture half and a shading half over the
    # whole queue) before those were retired
    "textured_triangles": lambda: _textured_triangles(),
}


def _textured_triangles():
    b = fs.base()
    fs.room(b)
    b.material_matte(b.texture_checkerboard((0.8, 0.2, 0.2), (0.2, 0.8, 0.2), uscale=4.0, vscale=4.0))
    scenes._quad(b, (-1.5, -1.2, 1.0), (-0.3, -1.2, 1.0), (-0.3, -1.2, -0.4), (-1.5, -1.2, -0.4))
    b.material_plastic(Kd=(0.3, 0.4, 0.5), Ks=(0.3, 0.3, 0.3), roughness=0.2)
    scenes._quad(b, (0.2, -1.0, 1.0), (1.5, -1.0, 1.0), (1.5, -1.0, -0.4), (0.2, -1.0, -0.4))
    return b.build()


def _radiance_samples(sd):
    ctx = pkg.Context(0)
    try:
        info = ctx.upload(sd)
        return ctx.radiance_samples(tuple(info.sample_bounds))
    finally:
        ctx.close()


LOCAL_SORT_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_features as t
np.savez(sys.argv[2], **{name: t._radiance_samples(make()) for name, make in t.LOCAL_SORT_SCENES.items()})
"""


def test_local_sort_switch_keeps_textured_scenes_on_the_sorted_path(tmp_path):
    """PBRTGPU_SHADE_LOCAL=1 asks for the local material sort wherever possible.  For a scene with textured materials it is not: the textured
    segment needs a list of its own (k_tex_resolve, k_shade_general_res), so such a scene takes the global sort whatever the variable says --
    with or without analytic shapes, with a sphere light, with constant lobe-list materials next to the textured ones.  Every camera sample
    of a fresh process that runs under the variable is the default render's, bit for bit."""
    out = str(tmp_path / "r.npz")
    r = subprocess.run([sys.executable, "-c", LOCAL_SORT_SCRIPT, ROOT, out], env=dict(os.environ, PBRTGPU_SHADE_LOCAL="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    for name, make in LOCAL_SORT_SCENES.items():
        base = _radiance_samples(make())
        assert base.any(), name
        assert np.array_equal(got[name], base), name


def test_crown_class_3p5m_textured_tiles(gpu_ctx, oracle):
    """BASELINE config 5's CONTENT at its scale, not only its size: the 3.5 M-triangle stand-in with the textured material split of the
    crown-class bench line (`bench.py --triangles 3500000 --materials textured`: image-mapped Matte under a bump map, a checkerboard-driven
    plastic, metal, glass, a bump-mapped mirror, an fbm-mixed substrate) -- k_tex_resolve + k_shade_general_res next to the Matte and
    lobe-list kernels over a material-sorted queue.  Three 16x16 tiles of per-sample radiance bit-identical to the oracle, every ray /
    node / triangle / vertex counter of a four-tile render equal, film weights bit-equal."""
    sd = scenes.rt1m(3500000, res=256, spp=8, max_depth=8, materials="textured")
    gpu_ctx.upload(sd)
    osc = oracle.scene(sd)
    info = gpu_ctx.info
    assert (osc.info.n_nodes, osc.info.n_leaves) == (info.n_nodes, info.n_leaves)
    sb = list(info.sample_bounds)
    tiles = [(sb[0] + 16 * i, sb[1] + 16 * j, sb[0] + 16 * i + 16, sb[1] + 16 * j + 16) for i, j in ((7, 7), (3, 11), (12, 5))]
    lit = 0.0
    for tile in tiles:
        g, r = gpu_ctx.radiance_samples(tile), osc.radiance_samples(tile)
        lit += float(r.sum())
        assert np.array_equal(bits(g), bits(r)), tile
    assert lit > 0
    four = tiles + [(sb[0] + 128, sb[1] + 128, sb[0] + 144, sb[1] + 144)]
    gpu_ctx.film_clear(); gpu_ctx.reset_counters()
    gpu_ctx.render(four)
    gx, gc = gpu_ctx.film_xyzw(), gpu_ctx.counters()
    ox, oc, _ = osc.render(four, threads=8)
    for k in ("camera_rays", "regular_rays", "shadow_rays", "nodes_visited", "tris_tested", "path_vertices"):
        assert gc[k] == oc[k], (k, gc[k], oc[k])
    assert np.array_equal(bits(gx[..., 3]), bits(ox[..., 3])) and rel_l2(gx, ox) < 1e-6
    osc.close()


@pytest.mark.parametrize("mode", ["1", "2"])
@pytest.mark.parametrize("name,make", [("cornell", lambda: scenes.cornell_box(res=64, spp=16)), ("materials", lambda: fs.scene_materials_lights("spatial")),
                                       ("spheres", lambda: fs.scene_spheres()), ("instances", lambda: fs.scene_instances()),
                                       ("textures", lambda: fs.scene_textures())])
def test_continuation_ray_sorting_changes_nothing(oracle, monkeypatch, name, make, mode):
    """Scenes larger than the Infinity Cache get their CONTINUATION rays ordered by origin cell and direction octant as well (mode 1: the
    ordered copy feeds the traversal kernel, shading keeps path order; mode 2: both walk the ordered list).  Forced on for these small
    scenes, every bounce: per-sample radiance, film and every counter must still be the oracle's, bit for bit -- only work lists move."""
    monkeypatch.setenv("PBRTGPU_SORT_SHADOW_MIN", "2")
    monkeypatch.setenv("PBRTGPU_SORT_CONT", mode)
    ctx = pkg.Context(0)
    try:
        sd = make()
        osc = oracle.scene(sd)
        ctx.upload(sd)
        _compare(ctx, osc, exact_film=True)
        osc.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("name,make", [("cornell", lambda: scenes.cornell_box(res=64, spp=16)), ("materials", lambda: fs.scene_materials_lights("spatial")),
                                       ("spheres", lambda: fs.scene_spheres()), ("instances", lambda: fs.scene_instances()),
                                       ("textures", lambda: fs.scene_textures())])
def test_shadow_ray_sorting_changes_nothing(oracle, monkeypatch, name, make):
    """pt_raysort.hip orders each bounce's shadow rays by origin cell and direction octant before they are traced -- from a million rays
    up, which no test scene reaches.  With the threshold at two (a context reads it when it is created) every bounce of these small scenes
    is sorted: per-sample radiance, film and every counter must still be the oracle's, bit for bit."""
    monkeypatch.setenv("PBRTGPU_SORT_SHADOW_MIN", "2")
    ctx = pkg.Context(0)
    try:
        sd = make()
        osc = oracle.scene(sd)
        ctx.upload(sd)
        _compare(ctx, osc, exact_film=True)
        osc.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("split,maxprims", [("sah", 4), ("hlbvh", 4), ("sah", 1), ("middle", 8)])
def test_rays_enter_instances_and_come_back(oracle, split, maxprims):
    """k_trace_inst's instance entry (a ray turns into the instance-space ray with the rest of its leaf, its slab interval and a marker left on its
    stack, and walks the object's tree in the wave's common phases) on a swarm of overlapping instances sharing world leaves with each other and with
    triangles: hits of plain ray batches (the blocking form), per-sample radiance, film and every counter are the oracle's."""
    sd = fs.scene_instance_swarm(split, maxprims)
    ctx = pkg.Context(0)
    try:
        ctx.upload(sd)
        assert sd.desc.n_instances == 36
        osc = oracle.scene(sd)
        _compare(ctx, osc, exact_film=True)
        osc.close()
    finally:
        ctx.close()
