"""Alpha masks on the GPU (shapes/alphamask.rs) where exact truth needs no mask evaluation at all: every masked triangle lies strictly
inside one region of constant mask value, which makes "alpha <= 0" mean exactly "these triangles are absent", and the truth comes from the
equivalent scene without them.  That proves the plumbing (flags, the per-mesh table, t_max restored, shadowalpha for any-hit rays only,
lights ignoring masks); masks that vary inside a triangle are held in test_gpu_alpha_mask_parity.py, and the oracle's own masks in
test_alpha_mask_oracle.py.

  * hooks: rays aimed into the masked quads through pt_trace_closest / pt_trace_any against the expected hit / occlusion;
  * removal: the masked scene rendered on the device equals the oracle's render of the scene without the cut-out triangles AND the oracle's
    render of the masked scene itself, per sample and film weight, bit for bit, over integrators, materials, samplers, spheres, object
    instances (mask in object space) and an environment;
  * shadowalpha 0 under whitted, an invisible emitter (alpha 0 on an area light), and the command-line front end."""
import os
import subprocess

import numpy as np
import pytest

from helpers import bits, pkg, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 8           # quads per side of the masked grid


@pytest.fixture(autouse=True)
def _clean_counters(gpu_ctx):
    """Leave the session's context as the other modules expect it: counters at zero."""
    yield
    gpu_ctx.reset_counters()


def oracle_scene(sd):
    """The oracle's scene, masks included (tests/oracle_lib.OracleScene forwards sd.alpha_masks)."""
    import oracle_lib
    return oracle_lib.load().scene(sd)


def grid_quads(z=1.0, keep=None, off=(0.0, 0.0)):
    """G x G quads, quad (i, j) over [i + .1, i + .9] x [j + .1, j + .9] at height z, uv = its (x, y): P, indices, uv.  keep(i, j) -> bool."""
    P, idx, uv = [], [], []
    for j in range(G):
        for i in range(G):
            if keep is not None and not keep(i, j):
                continue
            x0, x1, y0, y1 = i + 0.1, i + 0.9, j + 0.1, j + 0.9
            b = len(P)
            P += [(x0 + off[0], y0 + off[1], z), (x1 + off[0], y0 + off[1], z), (x1 + off[0], y1 + off[1], z), (x0 + off[0], y1 + off[1], z)]
            uv += [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
            idx += [b, b + 1, b + 2, b, b + 2, b + 3]
    return np.array(P, np.float32), np.array(idx, np.int64), np.array(uv, np.float32)


def block_image(seed=7):
    """64 x 64, 8 x 8 blocks of 0 or 1 (row 0 = t 0): quad (i, j) reads block (i, j) only on level 0."""
    rng = np.random.default_rng(seed)
    blocks = (rng.random((G, G)) < 0.5).astype(np.float32)          # [j, i]
    return np.kron(blocks, np.ones((8, 8), np.float32)), blocks


def mask_cases(sb):
    """name -> (alpha Tex, expected value > 0 per quad [j, i])."""
    ij = np.add.outer(np.arange(G), np.arange(G))
    img, blocks = block_image()
    im = sb.image_pyramid(img)
    ck = sb.texture_checkerboard(tex1=1.0, tex2=0.0)
    ck_none = sb.texture_checkerboard(tex1=0.0, tex2=2.0, aamode="none")
    ewa = sb.texture_imagemap(im, uscale=1.0 / G, vscale=1.0 / G)
    tri = sb.texture_imagemap(im, trilinear=True, uscale=1.0 / G, vscale=1.0 / G)
    return {
        "checker": (ck, ij % 2 == 0),
        "checker_none": (ck_none, ij % 2 == 1),
        "image_ewa": (ewa, blocks > 0),
        "image_trilinear": (tri, blocks > 0),
        "scale": (sb.texture_scale(ck, tri), (ij % 2 == 0) & (blocks > 0)),
        "mix": (sb.texture_mix(ck, ewa, amount=sb.texture_constant(0.25)), (ij % 2 == 0) | (blocks > 0)),
    }


def hook_points():
    """Points inside every quad, near its edges too (an image level above 0 mixes in the neighbouring blocks there)."""
    pts, quad = [], []
    for j in range(G):
        for i in range(G):
            for du in (0.12, 0.3, 0.7, 0.88):
                for dv in (0.14, 0.5, 0.86):
                    pts.append((i + du, j + dv)); quad.append((i, j))
    return np.array(pts, np.float32), np.array(quad)


def hook_scene(alpha, shadowalpha):
    sb = scenes.SceneBuilder()
    sb.look_at((4, 4, 10), (4, 4, 0), (0, 1, 0))
    sb.camera_perspective(fov=60)
    sb.film(xresolution=8, yresolution=8)
    sb.sampler_sobol(pixelsamples=1)
    sb.integrator_path()
    cases = mask_cases(sb)
    P, idx, uv = grid_quads()
    kw = {}
    if alpha is not None:
        kw["alpha"] = cases[alpha][0] if isinstance(alpha, str) else alpha
    if shadowalpha is not None:
        kw["shadowalpha"] = cases[shadowalpha][0] if isinstance(shadowalpha, str) else shadowalpha
    sb.shape_trianglemesh(P, idx, uv=uv, **kw)
    n_grid = len(idx) // 3
    sb.shape_trianglemesh([-1, -1, -1, 9, -1, -1, 9, 9, -1, -1, 9, -1], [0, 1, 2, 0, 2, 3])        # backdrop, unmasked
    return sb.build(), cases, n_grid


def expect(spec, cases):
    if spec is None:
        return np.ones((G, G), bool)
    if isinstance(spec, str):
        return cases[spec][1]
    return np.full((G, G), spec > 0.0)


HOOK_CASES = [(None, None), (0.0, None), (None, 0.0), (0.5, -1.0), (2.0, 0.3), ("checker", None), ("checker_none", None), ("image_ewa", None),
              ("image_trilinear", None), ("scale", None), ("mix", None), (None, "image_ewa"), ("checker", "image_trilinear"), (1.0, "mix")]


@pytest.mark.parametrize("alpha,shadowalpha", HOOK_CASES)
def test_hooks_see_the_masks(gpu_ctx, alpha, shadowalpha):
    sd, cases, n_grid = hook_scene(alpha, shadowalpha)
    gpu_ctx.upload(sd)
    a_ok, s_ok = expect(alpha, cases), expect(shadowalpha, cases)
    pts, quad = hook_points()
    o = np.concatenate([pts, np.full((len(pts), 1), 2.0, np.float32)], 1)
    d = np.tile(np.array([[0, 0, -1]], np.float32), (len(pts), 1))
    vis = a_ok[quad[:, 1], quad[:, 0]]
    h = gpu_ctx.trace_closest(o, d, np.full(len(pts), np.inf, np.float32))
    assert np.array_equal(h["prim"] < n_grid, vis)                     # the quad, or the backdrop behind it (a rejected hit keeps t_max)
    assert np.all(h["prim"] >= 0)
    assert np.allclose(h["t"], np.where(vis, 1.0, 3.0), rtol=1e-6, atol=0.0)
    occ = gpu_ctx.trace_any(o, d, np.full(len(pts), 2.5, np.float32))
    assert np.array_equal(occ.astype(bool), vis & s_ok[quad[:, 1], quad[:, 0]])
    # the wavefront's own traversal kernel: closest, shadow and probe items in one launch
    kind = np.tile(np.array([1, 2, 3], np.uint8), len(pts) // 3 + 1)[:len(pts)]
    tm = np.where(kind == 2, 2.5, np.inf).astype(np.float32)
    w_hit, w_occ = gpu_ctx.trace_wavefront(o, d, tm, kind)
    cl = kind != 2
    assert np.array_equal((w_hit["prim"][cl] < n_grid) & (w_hit["prim"][cl] >= 0), vis[cl])
    assert np.array_equal(w_occ[~cl].astype(bool), (vis & s_ok[quad[:, 1], quad[:, 0]])[~cl])


def test_upload_validates_the_masks(gpu_ctx):
    sd, _, _ = hook_scene(None, None)
    for field, value, match in (("mesh", 7, "mesh index"), ("alpha_texture", 99, "texture index")):
        am = pkg.capi.pt_alpha_mask()
        am.alpha_kind = pkg.capi.PT_ALPHA_TEXTURE
        am.alpha_texture = 0
        setattr(am, field, value)
        sd.alpha_masks = [am]
        with pytest.raises(pkg.capi.PtError, match=match):
            gpu_ctx.upload(sd)
    sb = scenes.SceneBuilder()
    sb.look_at((0, 0, 5), (0, 0, 0), (0, 1, 0)); sb.camera_perspective(); sb.film(8, 8); sb.sampler_sobol(1); sb.integrator_path()
    t = sb.texture_uv()
    sb.shape_trianglemesh([0, 0, 0, 1, 0, 0, 1, 1, 0], [0, 1, 2], alpha=t)
    with pytest.raises(pkg.capi.PtError, match="not a float texture"):
        gpu_ctx.upload(sb.build())


# ---------------------------------------------------------------- removal equivalence
def render_all(ctx, sd):
    info = ctx.upload(sd)
    sb = tuple(info.sample_bounds)
    rs = ctx.radiance_samples(sb)
    ctx.film_clear(); ctx.reset_counters(); ctx.render()
    return rs, ctx.film_xyzw(), ctx.counters(), info


def check_equivalent(ctx, sd_masked, sd_cut):
    gs, gx, gc, info = render_all(ctx, sd_masked)
    osc = oracle_scene(sd_cut)
    try:
        rs = osc.radiance_samples(tuple(info.sample_bounds))
        ox, oc, _ = osc.render(threads=8)
    finally:
        osc.close()
    assert np.array_equal(bits(gs), bits(rs)), np.abs(gs - rs).max()
    assert np.array_equal(bits(gx[..., 3]), bits(ox[..., 3]))
    assert np.allclose(gx[..., :3], ox[..., :3], rtol=1e-6, atol=1e-7)
    for k in ("camera_rays", "regular_rays", "shadow_rays"):
        assert gc[k] == oc[k], (k, gc[k], oc[k])
    # the third side: the oracle's render of the masked scene itself -- the same tree, so the traversal counters agree as well
    osc = oracle_scene(sd_masked)
    try:
        ms = osc.radiance_samples(tuple(info.sample_bounds))
        mx, mc, _ = osc.render(threads=8)
    finally:
        osc.close()
    assert np.array_equal(bits(gs), bits(ms)), np.abs(gs - ms).max()
    assert np.array_equal(bits(gx[..., 3]), bits(mx[..., 3]))
    assert np.allclose(gx[..., :3], mx[..., :3], rtol=1e-6, atol=1e-7)
    for k in ("camera_rays", "regular_rays", "shadow_rays", "path_vertices", "nodes_visited", "tris_tested"):
        assert gc[k] == mc[k], (k, gc[k], mc[k])


def removal_scene(cut, integ, material, sampler, extra, mask="checker"):
    """A room-sized box (floor, an emitter above, two walls) around the masked grid, so the world bound does not depend on the grid."""
    sb = scenes.SceneBuilder()
    sb.look_at((4, -3, 7), (4, 4, 0.5), (0, 0, 1))
    sb.camera_perspective(fov=60)
    sb.film(xresolution=24, yresolution=24)
    sb.pixel_filter_box()
    (sb.sampler_sobol if sampler == "sobol" else sb.sampler_halton)(pixelsamples=4)
    kind, opt = integ
    if kind == "path":
        sb.integrator_path(maxdepth=4, lightsamplestrategy=opt)
    elif kind == "directlighting":
        sb.integrator_directlighting(maxdepth=3, strategy=opt)
    elif kind == "whitted":
        sb.integrator_whitted(maxdepth=3)
    else:
        sb.integrator_ao(nsamples=4)
    cases = mask_cases(sb)
    tex, ok = cases[mask]
    sb.material_matte(Kd=(0.5, 0.45, 0.4))
    sb.shape_trianglemesh([-1, -1, 0, 9, -1, 0, 9, 9, 0, -1, 9, 0], [0, 1, 2, 0, 2, 3])
    sb.shape_trianglemesh([-1, 9, 0, 9, 9, 0, 9, 9, 4, -1, 9, 4], [0, 1, 2, 0, 2, 3])
    sb.shape_trianglemesh([9, -1, 0, 9, 9, 0, 9, 9, 4, 9, -1, 4], [0, 1, 2, 0, 2, 3])
    if kind != "ao":
        sb.area_light_source_diffuse(L=(6, 6, 5))
        sb.shape_trianglemesh([2, 2, 3.9, 6, 2, 3.9, 6, 6, 3.9, 2, 6, 3.9], [0, 2, 1, 0, 3, 2])
        sb.no_area_light()
        sb.area_light_source_diffuse(L=(2, 1, 1))
        sb.shape_trianglemesh([8, 0, 0.5, 8.5, 0, 0.5, 8.5, 0, 1.5], [0, 1, 2])
        sb.no_area_light()
    {"matte": lambda: sb.material_matte(Kd=(0.2, 0.6, 0.3)), "mirror": lambda: sb.material_mirror(),
     "glass": lambda: sb.material_glass(), "plastic": lambda: sb.material_plastic()}[material]()
    if extra == "instance":
        # the grid as an object (z = 0.5 in object space), instanced one unit along x (and 0.4 up): the 3-D checkerboard parity flips between
        # object and world space, so a mask evaluated in world space cuts the other half (transformed_primitive.rs:26-45)
        ck3 = sb.texture_checkerboard(tex1=1.0, tex2=0.0, dimension=3)
        sb.object_begin("grid")
        keep3 = lambda i, j: (i + j) % 2 == 1          # floor(x) = i - 1 in object space
        P, idx, uv = grid_quads(z=0.5, keep=keep3 if cut else None, off=(-1.0, 0.0))
        sb.shape_trianglemesh(P, idx, uv=uv, **({} if cut else {"alpha": ck3}))
        sb.object_end()
        m = np.eye(4, dtype=np.float32); m[0, 3] = 1.0; m[2, 3] = 0.4
        mi = np.eye(4, dtype=np.float32); mi[0, 3] = -1.0; mi[2, 3] = -0.4
        sb.object_instance("grid", (m.reshape(-1), mi.reshape(-1)))
    else:
        P, idx, uv = grid_quads(z=1.0, keep=(lambda i, j: ok[j, i]) if cut else None)
        sb.shape_trianglemesh(P, idx, uv=uv, **({} if cut else {"alpha": tex}))
        # a whole mesh cut by a constant
        if not cut:
            sb.shape_trianglemesh([1, 1, 2.5, 3, 1, 2.5, 3, 3, 2.5], [0, 1, 2], alpha=0.0)
    if extra == "sphere":
        sb.material_glass() if material != "glass" else sb.material_matte()
        sb.shape_sphere(radius=0.6, object_to_world=translate(6.5, 2.5, 2.0), world_to_object=translate(-6.5, -2.5, -2.0), alpha=0.0)
    if extra == "env":
        sb.light_infinite(L=(0.3, 0.35, 0.4))
    return sb.build()


def translate(x, y, z):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = (x, y, z)
    return m.reshape(-1)


REMOVAL = [
    (("path", "uniform"), "matte", "sobol", None, "checker"),
    (("path", "power"), "mirror", "halton", "sphere", "image_ewa"),
    (("path", "spatial"), "glass", "sobol", "instance", "checker"),
    (("path", "spatial"), "plastic", "halton", "env", "mix"),
    (("directlighting", "all"), "mirror", "sobol", "instance", "checker"),
    (("directlighting", "one"), "plastic", "halton", None, "image_trilinear"),
    (("directlighting", "one"), "glass", "sobol", "sphere", "checker_none"),
    (("whitted", None), "glass", "halton", "env", "image_ewa"),
    (("whitted", None), "mirror", "sobol", "instance", "checker"),
    (("ao", None), "matte", "sobol", "sphere", "scale"),
    (("ao", None), "matte", "halton", "instance", "checker"),
]


@pytest.mark.parametrize("integ,material,sampler,extra,mask", REMOVAL, ids=["-".join(str(x) for x in (c[0][0], c[0][1], *c[1:])) for c in REMOVAL])
def test_masked_render_equals_the_cut_scene(gpu_ctx, integ, material, sampler, extra, mask):
    check_equivalent(gpu_ctx, removal_scene(False, integ, material, sampler, extra, mask), removal_scene(True, integ, material, sampler, extra, mask))


# ---------------------------------------------------------------- shadowalpha, invisible emitters
def camera_hits(ctx, sd):
    """Per (pixel, sample), pixel-major like pt_radiance_samples: the primitive the camera ray hits."""
    info = ctx.upload(sd)
    b = list(info.sample_bounds)
    w, h, spp = b[2] - b[0], b[3] - b[1], info.spp
    ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
    pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
    o, d, _ = ctx.generate_camera_rays(pix, np.tile(np.arange(spp, dtype=np.uint32), w * h))
    return ctx.trace_closest(o, d, np.full(len(d), np.inf, np.float32))["prim"].reshape(w * h, spp)


def whitted_scene(blocker, emitter_alpha=None):
    """blocker: None, "opaque" or "shadow" (shadowalpha 0).  emitter_alpha: alpha of the small emitter facing the camera."""
    sb = scenes.SceneBuilder()
    sb.look_at((0, -5, 3), (0, 0, 0.5), (0, 0, 1))
    sb.camera_perspective(fov=50)
    sb.film(xresolution=32, yresolution=32)
    sb.pixel_filter_box(0.5, 0.5)
    sb.sampler_sobol(pixelsamples=4)
    sb.integrator_whitted(maxdepth=2)
    sb.material_matte(Kd=(0.6, 0.6, 0.6))
    sb.shape_trianglemesh([-3, -3, 0, 3, -3, 0, 3, 2.4, 0, -3, 2.4, 0], [0, 1, 2, 0, 2, 3])            # floor: prims 0, 1
    sb.area_light_source_diffuse(L=(8, 8, 8))
    sb.shape_trianglemesh([-1, -1, 3, 1, -1, 3, 1, 1, 3, -1, 1, 3], [0, 2, 1, 0, 3, 2])                # ceiling light: prims 2, 3
    sb.no_area_light()
    sb.area_light_source_diffuse(L=(3, 2, 1), twosided=True)
    # a small emitter behind the floor's far edge: no shadow ray of the floor crosses it, prims 4, 5
    sb.shape_trianglemesh([-0.4, 2.5, 0.3, 0.4, 2.5, 0.3, 0.4, 2.5, 1.1, -0.4, 2.5, 1.1], [0, 1, 2, 0, 2, 3],
                          **({} if emitter_alpha is None else {"alpha": emitter_alpha}))
    sb.no_area_light()
    sb.material_matte(Kd=(0.2, 0.3, 0.7))
    if blocker is not None:
        sb.shape_trianglemesh([-0.6, -0.6, 1.5, 0.6, -0.6, 1.5, 0.6, 0.6, 1.5, -0.6, 0.6, 1.5], [0, 1, 2, 0, 2, 3],
                              **({"shadowalpha": 0.0} if blocker == "shadow" else {}))               # prims 6, 7 (inside the bound)
    return sb.build()


def test_shadowalpha_zero_blocker_under_whitted(gpu_ctx):
    sd = whitted_scene("shadow")
    hit = camera_hits(gpu_ctx, sd)
    sees = (hit == 6) | (hit == 7)
    assert sees.any() and (~sees).any()
    gs, gx, gc, info = render_all(gpu_ctx, sd)
    tile = tuple(info.sample_bounds)
    outs = {}
    for name in ("none", "opaque"):
        osc = oracle_scene(whitted_scene(None if name == "none" else "opaque"))
        try:
            outs[name] = osc.radiance_samples(tile)
        finally:
            osc.close()
    assert np.array_equal(bits(gs[~sees]), bits(outs["none"][~sees]))        # shadow rays pass through the blocker
    assert np.array_equal(bits(gs[sees]), bits(outs["opaque"][sees]))        # camera rays still see it
    assert not np.array_equal(bits(outs["none"]), bits(outs["opaque"]))


def test_invisible_emitter_keeps_lighting(gpu_ctx):
    visible = whitted_scene(None)
    hit = camera_hits(gpu_ctx, visible)
    sees = (hit == 4) | (hit == 5)
    assert sees.any() and (~sees).any()
    gs, _, _, info = render_all(gpu_ctx, whitted_scene(None, emitter_alpha=0.0))
    assert info.n_lights == 4                                                 # area, sampling and pdf ignore the mask (alphamask.rs:115-146)
    osc = oracle_scene(visible)
    try:
        rs = osc.radiance_samples(tuple(info.sample_bounds))
    finally:
        osc.close()
    assert np.array_equal(bits(gs[~sees]), bits(rs[~sees]))
    assert not np.array_equal(bits(gs[sees]), bits(rs[sees]))              # those samples look through it


# ---------------------------------------------------------------- command line
def test_cli_matches_parsed_scene(tmp_path):
    img, _ = block_image(seed=11)
    with open(tmp_path / "mask.pfm", "wb") as f:
        f.write(b"PF\n64 64\n-1.0\n")
        rgb = np.repeat(img[:, :, None], 3, axis=2)
        f.write(np.ascontiguousarray(rgb[::-1]).astype("<f4").tobytes())
    P, idx, uv = grid_quads(z=1.0)
    mesh = ('Shape "trianglemesh" "integer indices" [%s] "point P" [%s] "float uv" [%s] "texture alpha" "m"\n'
            % (" ".join(map(str, idx.tolist())), " ".join("%g" % v for v in P.reshape(-1)), " ".join("%g" % v for v in uv.reshape(-1))))
    (tmp_path / "s.pbrt").write_text("""LookAt 4 -3 7  4 4 0.5  0 0 1
Camera "perspective" "float fov" [60]
Film "image" "integer xresolution" [24] "integer yresolution" [24] "string filename" "o.pfm"
Sampler "sobol" "integer pixelsamples" [4]
Integrator "path" "integer maxdepth" [3]
WorldBegin
Texture "m" "float" "imagemap" "string filename" "mask.pfm" "float uscale" [0.125] "float vscale" [0.125]
AttributeBegin
AreaLightSource "diffuse" "rgb L" [6 6 5]
Shape "trianglemesh" "integer indices" [0 2 1 0 3 2] "point P" [2 2 3.9 6 2 3.9 6 6 3.9 2 6 3.9]
AttributeEnd
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 9 -1 0 9 9 0 -1 9 0]
""" + mesh + "WorldEnd\n")
    ps = pkg.capi.ParsedScene(filename=str(tmp_path / "s.pbrt"))
    assert len(ps.alpha_masks) == 1 and ps.alpha_masks[0].alpha_kind == pkg.capi.PT_ALPHA_TEXTURE
    ctx = pkg.Context(0)
    try:
        ctx.upload(ps)
        ctx.film_clear(); ctx.render()
        want = ctx.film_rgb()
    finally:
        ctx.close()
    exe = os.path.join(ROOT, "pbrt-r3_amd", "csrc", "pbrt_gpu")
    out = tmp_path / "cli.pfm"
    r = subprocess.run([exe, "-i", str(tmp_path / "s.pbrt"), "--outfile", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    body = out.read_bytes().split(b"\n", 3)[3]
    got = np.frombuffer(body, "<f4").reshape(24, 24, 3)[::-1]
    assert np.array_equal(bits(got), bits(want))
    # and the mask did something: the same scene without it differs
    ps2 = pkg.capi.ParsedScene(text=(tmp_path / "s.pbrt").read_text().replace(' "texture alpha" "m"', ""), work_dir=str(tmp_path))
    ctx = pkg.Context(0)
    try:
        ctx.upload(ps2)
        ctx.film_clear(); ctx.render()
        assert not np.array_equal(ctx.film_rgb(), want)
    finally:
        ctx.close()
