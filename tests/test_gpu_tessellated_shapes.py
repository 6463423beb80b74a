"""Tessellated shapes on the GPU.  Once tessellated, "loopsubdiv", "nurbs" and "heightfield" are triangle meshes, so the oracle
renders them as it renders any mesh: every scene here goes to the device and to the oracle with the same descriptor, and the
per-sample radiance must agree bit for bit (and the film weights too, under the box filter).

  * integrators path, directlighting, whitted and ao, both samplers, box and Gaussian filters;
  * a subdivided area light, a glass subdivided object, an instanced one, a one-sided emitter under ReverseOrientation, the NURBS
    sphere whose pole normals are NaN;
  * an icosahedron at levels 6 (81 920 triangles) through the device BVH build;
  * the command-line front end on a file with all three shapes."""
import os
import subprocess

import numpy as np
import pytest

import tess_inputs as ti
from helpers import bits, pkg, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _clean_counters(gpu_ctx):
    yield
    gpu_ctx.reset_counters()


def render_all(ctx, sd):
    info = ctx.upload(sd)
    rs = ctx.radiance_samples(tuple(info.sample_bounds))
    ctx.film_clear(); ctx.reset_counters(); ctx.render()
    return rs, ctx.film_xyzw(), ctx.counters(), info


def check_oracle(ctx, oracle, sd, exact_film=True):
    """Per-sample radiance bit for bit.  The film: with the box filter each sample adds weight 1, so the weights are exact; a wider
    filter adds float weights through atomics, whose order differs from the oracle's in the last bits (as in test_gpu_features.py)."""
    gs, gx, gc, info = render_all(ctx, sd)
    osc = oracle.scene(sd)
    try:
        rs = osc.radiance_samples(tuple(info.sample_bounds))
        ox, oc, _ = osc.render(threads=8)
    finally:
        osc.close()
    assert np.array_equal(bits(gs), bits(rs)), np.nanmax(np.abs(gs - rs))
    if exact_film:
        assert np.array_equal(bits(gx[..., 3]), bits(ox[..., 3]))
        assert np.allclose(gx[..., :3], ox[..., :3], rtol=1e-6, atol=1e-7)
    else:
        assert np.allclose(gx, ox, rtol=1e-5, atol=1e-6)
    for k in ("camera_rays", "regular_rays", "shadow_rays"):
        assert gc[k] == oc[k], (k, gc[k], oc[k])
    return gs


def xf(t):
    m, mi = scenes.transform_translate(*t)
    return m, mi


def scene(integ="path", sampler="halton", filt="box", variant=None, res=16, spp=4):
    sb = scenes.SceneBuilder()
    sb.look_at((0.5, -4.5, 3.2), (0.5, 0.8, 0.6), (0, 0, 1))
    sb.camera_perspective(fov=55)
    sb.film(xresolution=res, yresolution=res)
    (sb.pixel_filter_box if filt == "box" else sb.pixel_filter_gaussian)()
    (sb.sampler_sobol if sampler == "sobol" else sb.sampler_halton)(pixelsamples=spp)
    {"path": lambda: sb.integrator_path(maxdepth=4), "directlighting": lambda: sb.integrator_directlighting(maxdepth=3),
     "whitted": lambda: sb.integrator_whitted(maxdepth=3), "ao": lambda: sb.integrator_ao(nsamples=4)}[integ]()
    sb.material_matte(Kd=(0.5, 0.45, 0.4))
    sb.shape_trianglemesh([-4, -4, 0, 5, -4, 0, 5, 5, 0, -4, 5, 0], [0, 1, 2, 0, 2, 3])
    sb.shape_trianglemesh([-4, 5, 0, 5, 5, 0, 5, 5, 5, -4, 5, 5], [0, 1, 2, 0, 2, 3])
    if integ != "ao":
        sb.area_light_source_diffuse(L=(5, 5, 4.5))
        sb.shape_trianglemesh([-1, -1, 4.5, 2, -1, 4.5, 2, 2, 4.5, -1, 2, 4.5], [0, 2, 1, 0, 3, 2])
        sb.no_area_light()
    P, I = ti.icosahedron(0.8)
    sb.material_plastic(Kd=(0.6, 0.2, 0.2))
    if variant == "glass":
        sb.material_glass()
    if variant == "instances":
        sb.object_begin("blob")
        sb.shape_loopsubdiv(P, I, levels=2)
        sb.object_end()
        for t in ((-1.5, 0, 0.9), (0.5, 1.5, 0.9), (2.5, 0, 0.9)):
            sb.object_instance("blob", xf(t))
    else:
        m, mi = xf((-1.5, 0, 0.9))
        sb.shape_loopsubdiv(P, I, levels=2, object_to_world=m, world_to_object=mi)
    if variant == "loop_light" and integ != "ao":
        sb.area_light_source_diffuse(L=(3, 2.5, 2))
        Pt, It = ti.tetrahedron()
        m, mi = xf((2.2, -1.0, 0.4))
        sb.shape_loopsubdiv(Pt * 0.8, It, levels=2, object_to_world=m, world_to_object=mi)
        sb.no_area_light()
    if variant == "one_sided_reversed" and integ != "ao":
        sb.area_light_source_diffuse(L=(3, 3, 3))
        sb.reverse_orientation = True
        m, mi = xf((2.2, -1.0, 0.6))
        sb.shape_loopsubdiv(*ti.icosahedron(0.5), levels=1, twosided=False, object_to_world=m, world_to_object=mi)
        sb.reverse_orientation = False
        sb.no_area_light()
    sb.material_matte(Kd=(0.2, 0.5, 0.3))
    kw = dict(ti.nurbs_sphere(0.7), diceu=12, dicev=9) if variant == "nurbs_sphere" else dict(
        nu=4, nv=4, uorder=3, vorder=4, uknots=[0, 0, 0, 0.4, 1, 1, 1], vknots=[0, 0, 0, 0, 1, 1, 1, 1],
        P=(np.stack(np.meshgrid(np.linspace(0, 1.6, 4), np.linspace(0, 1.6, 4)), -1).reshape(-1, 2).tolist()), diceu=9, dicev=7)
    if "P" in kw:
        xy = np.asarray(kw["P"], np.float32)
        kw["P"] = np.concatenate([xy, (0.4 * np.sin(3 * xy[:, :1]) * np.cos(2 * xy[:, 1:]))], 1).astype(np.float32).reshape(-1)
    m, mi = xf((0.2, 0.8, 0.9) if variant == "nurbs_sphere" else (0.0, 0.3, 0.2))
    sb.shape_nurbs(object_to_world=m, world_to_object=mi, **kw)
    sb.material_matte(Kd=(0.3, 0.3, 0.6))
    z = (0.3 * np.sin(np.arange(30) * 0.7)).astype(np.float32)
    m = np.diag([2.0, 2.0, 1.0, 1.0]).astype(np.float32); m[:3, 3] = [1.4, 1.8, 0.01]
    sb.shape_heightfield(6, 5, z, object_to_world=m.reshape(-1))
    return sb.build()


@pytest.mark.parametrize("filt", ["box", "gaussian"])
@pytest.mark.parametrize("sampler", ["halton", "sobol"])
@pytest.mark.parametrize("integ", ["path", "directlighting", "whitted", "ao"])
def test_integrators_match_oracle(gpu_ctx, oracle, integ, sampler, filt):
    check_oracle(gpu_ctx, oracle, scene(integ, sampler, filt), exact_film=filt == "box")


@pytest.mark.parametrize("variant", ["loop_light", "glass", "instances", "one_sided_reversed", "nurbs_sphere"])
def test_scene_variants_match_oracle(gpu_ctx, oracle, variant):
    sd = scene("path", "halton", "box", variant)
    if variant == "nurbs_sphere":
        assert np.isnan(sd.buffers["N"]).any()          # the pole normals reach the device as NaN
    if variant == "loop_light":
        assert sd.desc.n_area_lights == 2
    check_oracle(gpu_ctx, oracle, sd)


def test_subdivided_icosahedron_takes_the_device_bvh_build(oracle):
    sb = scenes.SceneBuilder()
    sb.look_at((0, -3.5, 1.5), (0, 0, 0), (0, 0, 1))
    sb.camera_perspective(fov=45)
    sb.film(xresolution=16, yresolution=16)
    sb.sampler_halton(pixelsamples=2)
    sb.integrator_path(maxdepth=3)
    sb.accelerator_bvh(splitmethod="hlbvh")
    sb.area_light_source_diffuse(L=(4, 4, 4))
    sb.shape_trianglemesh([-2, -2, 3, 2, -2, 3, 2, 2, 3, -2, 2, 3], [0, 2, 1, 0, 3, 2])
    sb.no_area_light()
    sb.material_plastic(Kd=(0.4, 0.5, 0.6))
    sb.shape_loopsubdiv(*ti.icosahedron(), levels=6)
    sd = sb.build()
    assert sd.desc.n_triangles == 2 + 81920
    ctx = pkg.Context(0)
    try:
        ctx.set_bvh_build(pkg.capi.BVH_BUILD_HOST)
        info = ctx.upload(sd)
        assert info.bvh_on_device == 0
        host = (ctx.bvh_digest(), info.n_nodes, info.n_leaves)
        ctx.set_bvh_build(pkg.capi.BVH_BUILD_AUTO)
        info = ctx.upload(sd)
        assert info.bvh_on_device == 1
        assert (ctx.bvh_digest(), info.n_nodes, info.n_leaves) == host
        check_oracle(ctx, oracle, sd)
    finally:
        ctx.close()


def test_cli_matches_library_render(tmp_path):
    P, I = ti.icosahedron(0.8)
    z = (0.3 * np.sin(np.arange(20) * 0.9)).astype(np.float32)
    (tmp_path / "s.pbrt").write_text("""LookAt 0.5 -4.5 3.2  0.5 0.8 0.6  0 0 1
Camera "perspective" "float fov" [55]
Film "image" "integer xresolution" [20] "integer yresolution" [20] "string filename" "o.pfm"
Sampler "halton" "integer pixelsamples" [4]
Integrator "path" "integer maxdepth" [3]
WorldBegin
AttributeBegin
AreaLightSource "diffuse" "rgb L" [5 5 4.5]
Shape "trianglemesh" "integer indices" [0 2 1 0 3 2] "point P" [-1 -1 4.5 2 -1 4.5 2 2 4.5 -1 2 4.5]
AttributeEnd
Material "matte" "rgb Kd" [0.5 0.45 0.4]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-4 -4 0 5 -4 0 5 5 0 -4 5 0]
AttributeBegin
Translate -1.5 0 0.9
Material "plastic" "rgb Kd" [0.6 0.2 0.2]
""" + ti.loopsubdiv_text(P, I, 2) + """AttributeEnd
AttributeBegin
Translate 0.2 0.8 0.9
""" + ti.nurbs_text(dict(ti.nurbs_sphere(0.7), diceu=10, dicev=8)) + """AttributeEnd
AttributeBegin
Translate 1.4 1.8 0.01
Scale 2 2 1
""" + ti.heightfield_text(5, 4, z) + "AttributeEnd\nWorldEnd\n")
    ps = pkg.capi.ParsedScene(filename=str(tmp_path / "s.pbrt"))
    assert ps.desc.n_meshes == 5
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
    got = np.frombuffer(body, "<f4").reshape(20, 20, 3)[::-1]
    assert np.array_equal(bits(got), bits(want))
    assert np.isfinite(want).all() and want.max() > 0
