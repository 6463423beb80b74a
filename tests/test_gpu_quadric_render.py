"""Cylinders and disks through the renderer (pt_radiance_samples): emitters seen directly, the irradiance under a disk light against its
closed form, and a parsed .pbrt scene through every integrator."""
import numpy as np
import pytest

import feature_scenes as fs
from helpers import pkg, scenes

pytestmark = pytest.mark.gpu
T = scenes
capi = pkg.capi


def _pixel_samples(info):
    sb = tuple(info.sample_bounds)
    xs, ys = np.meshgrid(np.arange(sb[0], sb[2]), np.arange(sb[1], sb[3]))
    px = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.int32)
    return np.repeat(px, info.spp, 0), np.tile(np.arange(info.spp, dtype=np.uint32), len(px)), sb


# ------------------------------------------------------------------------------------------------------ emitters seen directly
L_DISK, L_CYL = (3.0, 5.0, 7.0), (2.0, 0.5, 0.25)


def _emitter_scene(eye):
    """A one-sided disk emitter facing +y and a one-sided cylinder emitter, nothing else that emits; `path` with maxdepth 0."""
    b = scenes.SceneBuilder()
    b.look_at(eye, (0, 0, 0), (0, 0, 1))
    b.camera_perspective(fov=50.0)
    b.film(xresolution=24, yresolution=24)
    b.pixel_filter_box()
    b.sampler_sobol(4)
    b.integrator_path(maxdepth=0)
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=L_DISK)
    t = T.transform_mul(T.transform_translate(-0.7, 0.0, 0.0), T.transform_rotate_x(-90.0))          # object +z -> world +y
    b.shape_disk(height=0.0, radius=0.6, innerradius=0.1, phimax=300.0, object_to_world=t[0], world_to_object=t[1])
    b.area_light_source_diffuse(L=L_CYL)
    t = T.transform_translate(0.8, 0.0, 0.0)
    b.shape_cylinder(radius=0.4, zmin=-0.5, zmax=0.5, phimax=270.0, object_to_world=t[0], world_to_object=t[1])
    b.no_area_light()
    scenes._quad(b, (-3, -3, -2), (3, -3, -2), (3, 3, -2), (-3, 3, -2))
    return b.build()


@pytest.mark.parametrize("eye", [(0.0, 4.0, 0.5), (0.0, -4.0, 0.5)], ids=["front", "behind"])
def test_emitter_seen_directly_returns_L(gpu_ctx, eye):
    """Every camera sample whose ray hits the disk equals its L exactly -- from behind too, although the light is one-sided: the
    interaction's normal always faces the ray (disk.rs:95-98), so Le sees the emitting side from either face.  The cylinder's normal does
    not turn: its outside emits, its inside (seen through the phimax gap) is black."""
    sd = _emitter_scene(eye)
    info = gpu_ctx.upload(sd)
    px, si, sb = _pixel_samples(info)
    o, d, _ = gpu_ctx.generate_camera_rays(px, si)
    hits = gpu_ctx.trace_closest(o, d, np.full(len(o), np.inf, np.float32))
    rad = gpu_ctx.radiance_samples(sb).reshape(-1, 3)
    disk, cyl = hits["prim"] == 0, hits["prim"] == 1
    assert disk.sum() >= 100 and cyl.sum() >= 100
    assert (rad[disk] == np.float32(L_DISK)).all()
    # the cylinder: outside faces emit L, inside faces nothing; which is which by the object-space geometry in float64
    centre = np.array([0.8, 0.0, 0.0])
    p = o[cyl].astype(np.float64) + hits["t"][cyl].astype(np.float64)[:, None] * d[cyl].astype(np.float64)
    radial = p - centre
    radial[:, 2] = 0.0
    cosv = (radial * -d[cyl].astype(np.float64)).sum(1) / np.linalg.norm(radial, axis=1) / np.linalg.norm(d[cyl].astype(np.float64), axis=1)
    out = cosv > 1e-3
    assert out.sum() >= 50
    assert (rad[cyl][out] == np.float32(L_CYL)).all()
    assert (rad[cyl][cosv < -1e-3] == 0).all()
    assert (rad[~disk & ~cyl] == 0).all()


# -------------------------------------------------------------------------------------------- irradiance under a disk light
KD, L_LAMP, R_LAMP, H_LAMP = 0.6, 8.0, 0.75, 1.25


def _lamp_scene(integrator):
    b = scenes.SceneBuilder()
    b.look_at((2.5, -2.5, 1.5), (0, 0, 0), (0, 0, 1))
    b.camera_perspective(fov=3.0)
    b.film(xresolution=16, yresolution=16)
    b.pixel_filter_box()
    b.sampler_sobol(64)
    if integrator == "path":
        b.integrator_path(maxdepth=1)
    else:
        b.integrator_directlighting(maxdepth=1, strategy="all")
    b.material_matte((0.0, 0.0, 0.0))
    b.area_light_source_diffuse(L=(L_LAMP, L_LAMP, L_LAMP))
    b.reverse_orientation = True                       # the disk's normal is +z of its object space: reversed, it emits downwards
    t = T.transform_translate(0.0, 0.0, H_LAMP)
    b.shape_disk(height=0.0, radius=R_LAMP, object_to_world=t[0], world_to_object=t[1])
    b.reverse_orientation = False
    b.no_area_light()
    b.material_matte((KD, KD, KD))
    scenes._quad(b, (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    return b.build()


def _disk_form_factor(a, h, r):
    """The form factor of a disk of radius r, parallel to the receiver and h above it, seen from a point at distance a from its axis:
    r^2 / (h^2 + r^2) on the axis."""
    a = np.maximum(a, 1e-9)
    H, R = h / a, r / a
    z = 1.0 + H * H + R * R
    return 0.5 * (1.0 - (1.0 + H * H - R * R) / np.sqrt(z * z - 4.0 * R * R))


@pytest.mark.parametrize("integrator", ["directlighting", "path"])
def test_irradiance_under_a_disk_light(gpu_ctx, integrator):
    """A matte quad under a parallel full disk light: the mean radiance of a 16 x 16 patch around the axis at 64 spp against
    Kd L F(p), F the disk's form factor at each sample's own point (r^2 / (h^2 + r^2) on the axis), within five standard errors of the
    per-sample radiances themselves."""
    sd = _lamp_scene(integrator)
    info = gpu_ctx.upload(sd)
    px, si, sb = _pixel_samples(info)
    o, d, _ = gpu_ctx.generate_camera_rays(px, si)
    hits = gpu_ctx.trace_closest(o, d, np.full(len(o), np.inf, np.float32))
    rad = gpu_ctx.radiance_samples(sb).reshape(-1, 3).astype(np.float64)
    quad = hits["prim"] >= 1
    assert quad.all()
    p = o.astype(np.float64) + hits["t"].astype(np.float64)[:, None] * d.astype(np.float64)
    a = np.hypot(p[:, 0], p[:, 1])
    assert a.max() < R_LAMP                                # the patch lies around the axis, inside the lamp's footprint
    expect = KD * L_LAMP * _disk_form_factor(a, H_LAMP, R_LAMP)
    on_axis = KD * L_LAMP * R_LAMP ** 2 / (H_LAMP ** 2 + R_LAMP ** 2)
    diff = rad[:, 0] - expect
    se = diff.std(ddof=1) / np.sqrt(len(diff))
    print("%s: mean radiance %.6f  expected %.6f (on the axis %.6f)  off %.3g  standard error %.3g  (%d samples)" % (
        integrator, rad[:, 0].mean(), expect.mean(), on_axis, diff.mean(), se, len(diff)))
    assert np.isfinite(rad).all() and se > 0
    assert abs(diff.mean()) <= 5.0 * se
    assert np.array_equal(rad[:, 0], rad[:, 1]) and np.array_equal(rad[:, 0], rad[:, 2])


# ------------------------------------------------------------------------------------------------------ validation at upload
def _one_shape(edit):
    b = fs.base(res=8, spp=1)
    fs.room(b)
    b.shape_cylinder(radius=0.5)
    b.shape_disk(radius=0.5, innerradius=0.1)
    sd = b.build()
    edit(sd.buffers["spheres"][0], sd.buffers["spheres"][1])
    return sd


def _set(obj, **kw):
    for k, v in kw.items():
        if k == "row3":
            obj.object_to_world[12] = v
        else:
            setattr(obj, k, v)


@pytest.mark.parametrize("edit,needle", [
    (lambda c, d: _set(c, kind=3), "unknown kind"),
    (lambda c, d: _set(c, zmax=float("inf")), "cylinder parameters must be finite"),
    (lambda c, d: _set(d, zmin=float("nan")), "disk parameters must be finite"),
    (lambda c, d: _set(c, radius=0.0), "cylinder radius must be positive"),
    (lambda c, d: _set(d, radius=-1.0), "disk radius must be positive"),
    (lambda c, d: _set(d, inner_radius=-0.1), "disk inner_radius"),
    (lambda c, d: _set(d, inner_radius=0.5), "disk inner_radius"),
    (lambda c, d: _set(c, row3=0.5), "cylinder under a projective transform"),
    (lambda c, d: _set(d, row3=0.5), "disk under a projective transform"),
], ids=["kind", "cylinder-inf", "disk-nan", "cylinder-r0", "disk-r-negative", "disk-ri-negative", "disk-ri-radius", "cylinder-projective", "disk-projective"])
def test_upload_refuses_with_a_message_that_names_the_shape(gpu_ctx, edit, needle):
    with pytest.raises(capi.PtError) as e:
        gpu_ctx.upload(_one_shape(edit))
    assert needle in str(e.value)
    gpu_ctx.upload(_one_shape(lambda c, d: None))          # the unedited scene uploads, and the context is usable afterwards


# --------------------------------------------------------------------------------------------------------------- parsed scene
PBRT = '''
LookAt 0 -6 1.5  0 0 0.8  0 0 1
Camera "perspective" "float fov" 40
Film "image" "integer xresolution" 32 "integer yresolution" 32
PixelFilter "box"
Sampler "sobol" "integer pixelsamples" 4
%s
WorldBegin
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [12 11 9]
  Translate 0 0 2.8
  ReverseOrientation
  Shape "disk" "float radius" 0.8
AttributeEnd
Material "matte" "rgb Kd" [0.6 0.6 0.6]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 -3 0  3 -3 0  3 3 0  -3 3 0]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 3 0  3 3 0  3 3 3  -3 3 3]
AttributeBegin
  Material "plastic" "rgb Kd" [0.2 0.5 0.7]
  Translate -1.2 0.5 0
  Shape "cylinder" "float radius" 0.4 "float zmin" 0 "float zmax" 1.6
  Translate 0 0 1.6
  Shape "disk" "float radius" 0.4
AttributeEnd
ObjectBegin "pipe"
  Material "matte" "rgb Kd" [0.8 0.3 0.2]
  Shape "cylinder" "float radius" 0.25 "float zmin" -0.9 "float zmax" 0.9 "float phimax" 300
  Shape "disk" "float height" 0.9 "float radius" 0.25 "float innerradius" 0.1
ObjectEnd
AttributeBegin
  Translate 1.0 -0.3 0.5
  Rotate 90 0 1 0
  ObjectInstance "pipe"
AttributeEnd
AttributeBegin
  Translate 0.2 1.2 1.4
  Rotate 35 1 0 0
  Scale 1 1 0.6
  ObjectInstance "pipe"
AttributeEnd
WorldEnd
'''
INTEGRATORS = {"path": 'Integrator "path" "integer maxdepth" 4', "directlighting": 'Integrator "directlighting"', "whitted": 'Integrator "whitted" "integer maxdepth" 3',
               "ao": 'Integrator "ao" "integer nsamples" 8'}


@pytest.mark.parametrize("integrator", list(INTEGRATORS))
def test_parsed_scene_renders(gpu_ctx, integrator):
    """One .pbrt text with both shapes, an AreaLightSource on a disk and a cylinder inside an ObjectInstance: finite, not black, and the
    same film bit for bit when rendered again."""
    ps = capi.ParsedScene(text=PBRT % INTEGRATORS[integrator], quadric_shapes=True)
    kinds = sorted(ps.desc.spheres[i].kind for i in range(ps.desc.n_spheres))
    assert kinds == [1, 1, 2, 2, 2] and ps.desc.n_instances == 2
    films = []
    for _ in range(2):
        gpu_ctx.upload(ps)
        gpu_ctx.film_clear()
        gpu_ctx.render()
        films.append(gpu_ctx.film_rgb().copy())
    assert np.isfinite(films[0]).all() and films[0].max() > 0.05 and (films[0] > 0).mean() > 0.5
    assert np.array_equal(films[0], films[1])
    gpu_ctx.reset_counters()


def test_cli_renders_a_disk_lamp_over_cylinders(gpu_ctx, tmp_path):
    """`pbrt_gpu -i` takes both directives: the PFM it writes is the film the library renders from the same text parsed with
    quadric_shapes=True, bit for bit."""
    import os
    import subprocess
    from helpers import bits
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = PBRT % INTEGRATORS["path"]
    (tmp_path / "s.pbrt").write_text(text)
    gpu_ctx.upload(capi.ParsedScene(filename=str(tmp_path / "s.pbrt"), quadric_shapes=True))
    gpu_ctx.film_clear()
    gpu_ctx.render()
    want = gpu_ctx.film_rgb().copy()
    gpu_ctx.reset_counters()
    out = tmp_path / "cli.pfm"
    r = subprocess.run([os.path.join(root, "pbrt-r3_amd", "csrc", "pbrt_gpu"), "-i", str(tmp_path / "s.pbrt"), "--outfile", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer(out.read_bytes().split(b"\n", 3)[3], "<f4").reshape(32, 32, 3)[::-1]
    assert np.array_equal(bits(got), bits(want)) and want.max() > 0


PBRT_TEXTURED = '''
LookAt 0 -5 1.6  0 0 0.7  0 0 1
Camera "perspective" "float fov" 40
Film "image" "integer xresolution" 32 "integer yresolution" 32
PixelFilter "box"
Sampler "sobol" "integer pixelsamples" 4
Integrator "%s" "integer maxdepth" 4
WorldBegin
LightSource "infinite" "rgb L" [0.8 0.9 1.0]
LightSource "spot" "point from" [2 -3 4] "point to" [0 0 0.5] "rgb I" [30 30 30] "float coneangle" 40
Texture "ck" "spectrum" "checkerboard" "float uscale" 8 "float vscale" 4 "rgb tex1" [0.8 0.2 0.1] "rgb tex2" [0.1 0.3 0.8]
Texture "bumps" "float" "checkerboard" "float uscale" 16 "float vscale" 8 "float tex1" 0.0 "float tex2" 0.02
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 -3 0  3 -3 0  3 3 0  -3 3 0]
AttributeBegin
  Material "matte" "texture Kd" "ck" "texture bumpmap" "bumps"
  Translate -0.9 0 0
  Shape "cylinder" "float radius" 0.5 "float zmin" 0 "float zmax" 1.5
AttributeEnd
AttributeBegin
  MakeNamedMaterial "a" "string type" "plastic" "texture Kd" "ck"
  MakeNamedMaterial "b" "string type" "mirror"
  Material "mix" "string namedmaterial1" "a" "string namedmaterial2" "b" "rgb amount" [0.4 0.4 0.4]
  Translate 0.9 0 0.8
  Rotate 70 1 0 0
  Shape "disk" "float radius" 0.7 "float innerradius" 0.2
AttributeEnd
WorldEnd
'''


@pytest.mark.parametrize("integrator", ["path", "directlighting", "whitted"])
def test_textured_and_mixed_shapes_under_infinite_and_delta_lights(gpu_ctx, integrator):
    """The rest of the second kernel set: a cylinder with a uv-textured, bump-mapped material (the texture kernels read its uv, dpdu and
    dndu), a disk with a mix material, an infinite light and a spot light.  The checkerboard shows on the cylinder (pixels on it differ in
    hue), the film is finite and the same bit for bit when rendered again."""
    ps = capi.ParsedScene(text=PBRT_TEXTURED % integrator, quadric_shapes=True, mix_materials=True, delta_lights=True)
    assert sorted(ps.desc.spheres[i].kind for i in range(ps.desc.n_spheres)) == [1, 2]
    films = []
    for _ in range(2):
        gpu_ctx.upload(ps)
        gpu_ctx.film_clear()
        gpu_ctx.render()
        films.append(gpu_ctx.film_rgb().copy())
    gpu_ctx.reset_counters()
    f = films[0]
    assert np.isfinite(f).all() and f.max() > 0.05 and (f > 0).mean() > 0.5
    assert np.array_equal(films[0], films[1])
    hue = f[..., 0] / np.maximum(f.sum(-1), 1e-6)
    assert hue.max() > 0.45 and hue.min() < 0.25          # the red and the blue checks both show
