"""Small scenes that switch on every branch of the accelerated path that the two BASELINE
scenes leave cold (vertex normals / tangents / uvs, one-sided and reversed meshes, Oren-Nayar,
black and absent materials, several lights with each sampling strategy, thin lens, wide
reconstruction filters, crop window, luminance clamp, every BVH split method and leaf size)."""
import numpy as np

from helpers import pkg, scenes

f32 = np.float32


def uv_sphere(center, radius, nt=8, nphi=12):
    P, N, UV, idx = [], [], [], []
    for t in range(nt + 1):
        th = np.pi * t / nt
        for p in range(nphi):
            ph = 2 * np.pi * p / nphi
            n = np.array([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)])
            P.append(np.array(center) + radius * n); N.append(n); UV.append([p / nphi, t / nt])
    for t in range(nt):
        for p in range(nphi):
            a, b = t * nphi + p, t * nphi + (p + 1) % nphi
            c, d = a + nphi, b + nphi
            idx += [a, c, b, b, c, d]
    return np.array(P, np.float32), np.array(N, np.float32), np.array(UV, np.float32), idx


def room(b, size=2.0, light_L=(10, 9, 8), two_sided_light=False, open_top=False):
    """Floor, ceiling, back and side walls, open towards the camera; open_top leaves the ceiling out (an environment then lights the room
    from above too)."""
    s = size
    b.material_matte((0.7, 0.7, 0.7))
    scenes._quad(b, (s, -s, -s), (-s, -s, -s), (-s, -s, s), (s, -s, s))
    if not open_top:
        scenes._quad(b, (s, s, -s), (s, s, s), (-s, s, s), (-s, s, -s))
    scenes._quad(b, (s, -s, s), (-s, -s, s), (-s, s, s), (s, s, s))
    b.material_matte((0.2, 0.6, 0.3))
    scenes._quad(b, (-s, -s, s), (-s, -s, -s), (-s, s, -s), (-s, s, s))
    b.material_matte((0.7, 0.2, 0.2))
    scenes._quad(b, (s, -s, -s), (s, -s, s), (s, s, s), (s, s, -s))
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=light_L, twosided=two_sided_light)
    h = 0.999 * s
    scenes._quad(b, (0.5, h, -0.5), (0.5, h, 0.5), (-0.5, h, 0.5), (-0.5, h, -0.5))
    b.no_area_light()


def base(res=48, spp=8, depth=5):
    b = scenes.SceneBuilder()
    b.look_at((0, 0, -6.5), (0, 0, 0), (0, 1, 0))
    b.camera_perspective(fov=40.0)
    b.film(xresolution=res, yresolution=res)
    b.pixel_filter_box()
    b.sampler_sobol(spp)
    b.integrator_path(maxdepth=depth)
    return b


def scene_attributes():
    """Smooth-shaded sphere (N + uv), a tangent-carrying quad (S), a one-sided quad, a reversed one."""
    b = base()
    room(b)
    b.material_matte((0.6, 0.6, 0.8))
    P, N, UV, idx = uv_sphere((-0.7, -1.2, 0.3), 0.8)
    b.shape_trianglemesh(P, idx, N=N, uv=UV)
    b.material_matte((0.8, 0.7, 0.3))
    q = [(0.3, -2 + 0.01, -0.5), (1.5, -2 + 0.01, -0.5), (1.5, -0.9, 0.6), (0.3, -0.9, 0.6)]
    S = [(1, 0.2, 0)] * 4
    b.shape_trianglemesh(q, [0, 1, 2, 0, 2, 3], S=S)
    b.material_matte((0.3, 0.3, 0.9))
    b.shape_trianglemesh([(-1.9, 0.2, 1.0), (-0.6, 0.2, 1.5), (-0.6, 1.5, 1.5), (-1.9, 1.5, 1.0)], [0, 1, 2, 0, 2, 3], twosided=False)
    b.reverse_orientation = True
    b.shape_trianglemesh([(0.6, 0.2, 1.5), (1.9, 0.2, 1.0), (1.9, 1.5, 1.0), (0.6, 1.5, 1.5)], [0, 1, 2, 0, 2, 3], twosided=False)
    b.reverse_orientation = False
    P2, N2, UV2, idx2 = uv_sphere((1.0, 1.0, -0.5), 0.4, 5, 8)
    b.shape_trianglemesh(P2, idx2, N=N2)            # normals, auto uv rule (not fillable -> default uvs)
    return b.build()


def scene_materials_lights(strategy="spatial"):
    """Oren-Nayar, a black matte, a material-less occluder, three lights (one two-sided, one mesh light)."""
    b = base(depth=6)
    b.integrator_path(maxdepth=6, lightsamplestrategy=strategy)
    room(b, light_L=(6, 6, 6))
    b.material_matte((0.7, 0.6, 0.5), sigma=35.0)
    P, N, UV, idx = uv_sphere((-0.8, -1.2, 0.0), 0.8, 6, 10)
    b.shape_trianglemesh(P, idx)
    b.material_matte((0.0, 0.0, 0.0))
    scenes._cuboid(b, [(0.4, -1.0, -0.4), (0.4, -1.0, 0.6), (1.4, -1.0, 0.6), (1.4, -1.0, -0.4)], 1.0)
    b.material_none()
    scenes._quad(b, (-1.5, -0.5, -1.5), (1.5, -0.5, -1.5), (1.5, 1.0, -1.5), (-1.5, 1.0, -1.5))   # invisible pane in front
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=(4, 1, 1), twosided=True)
    scenes._quad(b, (-1.99, 0.0, -0.3), (-1.99, 0.0, 0.3), (-1.99, 0.6, 0.3), (-1.99, 0.6, -0.3))
    b.area_light_source_diffuse(L=(0.5, 0.5, 3))
    P3, N3, UV3, idx3 = uv_sphere((1.2, 1.2, 0.8), 0.25, 3, 5)
    b.shape_trianglemesh(P3, idx3)                    # 30-triangle mesh light
    b.no_area_light()
    return b.build()


def scene_camera_film(filt="gaussian"):
    """Thin lens, wide reconstruction filter, crop window, film scale, luminance clamp."""
    b = base(res=40, spp=4)
    b.camera_perspective(fov=40.0, lensradius=0.15, focaldistance=6.0)
    b.film(xresolution=40, yresolution=32, cropwindow=(0.2, 0.85, 0.1, 0.9), scale=2.0, maxsampleluminance=3.0)
    if filt == "gaussian":
        b.pixel_filter_gaussian(2.0, 2.0, 2.0)
    elif filt == "mitchell":
        b.pixel_filter_mitchell(2.0, 1.5)
    elif filt == "sinc":
        b.pixel_filter_sinc(3.0, 2.5, 2.0)
    else:
        b.pixel_filter_triangle(1.5, 2.0)
    room(b)
    b.material_matte((0.6, 0.6, 0.6))
    P, N, UV, idx = uv_sphere((0.0, -1.0, 0.0), 1.0, 6, 10)
    b.shape_trianglemesh(P, idx, N=N)
    return b.build()


def scene_accel(method, leaf):
    sd = scenes.rt1m(4000, res=32, spp=4, max_depth=4)
    sd.desc.split_method = {"sah": 0, "hlbvh": 1, "middle": 2, "equal": 3}[method]
    sd.desc.max_node_prims = leaf
    return sd


# ---- materials beyond matte (SURVEY.md section 8, rows a10/a11 "later")
MATERIAL_KINDS = ["plastic", "mirror", "glass", "glass_rough", "glass_reflect_only", "glass_black", "metal", "metal_aniso",
                  "uber", "uber_translucent", "substrate", "substrate_aniso", "plastic_noremap"]


def apply_material(b, kind):
    if kind == "plastic":
        b.material_plastic(Kd=(0.3, 0.1, 0.1), Ks=(0.4, 0.4, 0.4), roughness=0.15)
    elif kind == "plastic_noremap":
        b.material_plastic(Kd=(0.0, 0.0, 0.0), Ks=(0.6, 0.5, 0.4), roughness=0.2, remaproughness=False)
    elif kind == "mirror":
        b.material_mirror(Kr=(0.9, 0.85, 0.8))
    elif kind == "glass":
        b.material_glass(eta=1.5)
    elif kind == "glass_rough":
        b.material_glass(Kr=(0.9, 0.9, 0.9), Kt=(0.8, 0.9, 0.8), eta=1.33, uroughness=0.1, vroughness=0.2)
    elif kind == "glass_reflect_only":
        b.material_glass(Kr=(1.0, 1.0, 1.0), Kt=(0.0, 0.0, 0.0), eta=1.5, uroughness=0.05, vroughness=0.05)
    elif kind == "glass_black":
        b.material_glass(Kr=(0.0, 0.0, 0.0), Kt=(0.0, 0.0, 0.0))
    elif kind == "metal":
        b.material_metal(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), roughness=0.05)
    elif kind == "metal_aniso":
        b.material_metal(eta=(0.14, 0.37, 1.44), k=(3.98, 2.38, 1.6), uroughness=0.02, vroughness=0.2)
    elif kind == "uber":
        b.material_uber(Kd=(0.3, 0.3, 0.5), Ks=(0.2, 0.2, 0.2), Kr=(0.1, 0.1, 0.1), Kt=(0.2, 0.2, 0.2), eta=1.4, roughness=0.1)
    elif kind == "uber_translucent":
        b.material_uber(Kd=(0.5, 0.4, 0.3), Ks=(0.3, 0.3, 0.3), opacity=(0.6, 0.7, 0.8), uroughness=0.05, vroughness=0.15)
    elif kind == "substrate":
        b.material_substrate(Kd=(0.4, 0.2, 0.1), Ks=(0.3, 0.3, 0.3), uroughness=0.1, vroughness=0.1)
    elif kind == "substrate_aniso":
        b.material_substrate(Kd=(0.1, 0.3, 0.4), Ks=(0.5, 0.5, 0.5), uroughness=0.02, vroughness=0.3)
    else:
        raise ValueError(kind)


def scene_material_palette():
    """One small triangle per material kind: the scene only carries the material table for the BSDF hooks."""
    b = base(res=16, spp=1)
    room(b)
    index = {}
    for k, kind in enumerate(MATERIAL_KINDS):
        apply_material(b, kind)
        index[kind] = b.cur_material
        x = -1.8 + 0.25 * k
        b.shape_trianglemesh([(x, -1.9, 0), (x + 0.2, -1.9, 0), (x, -1.7, 0)], [0, 1, 2])
    index["matte"] = 1
    b.material_matte((0.5, 0.4, 0.3), sigma=25.0)
    index["oren_nayar"] = b.cur_material
    b.shape_trianglemesh([(1.6, -1.9, 0), (1.8, -1.9, 0), (1.6, -1.7, 0)], [0, 1, 2])
    sd = b.build()
    sd.material_index = index
    return sd


def scene_materials_render(kinds, res=40, spp=8, depth=6, sampler="sobol"):
    """Room with a sphere and two slabs carrying the given materials (smooth-shaded sphere: shading != geometric normal)."""
    b = base(res=res, spp=spp, depth=depth)
    if sampler == "halton":
        b.sampler_halton(spp)
    room(b)
    apply_material(b, kinds[0])
    P, N, UV, idx = uv_sphere((-0.6, -1.1, 0.2), 0.9, 10, 16)
    b.shape_trianglemesh(P, idx, N=N, uv=UV)
    apply_material(b, kinds[1 % len(kinds)])
    b.shape_trianglemesh([(0.3, -1.99, -0.8), (1.7, -1.99, -0.8), (1.7, -0.6, 0.9), (0.3, -0.6, 0.9)], [0, 1, 2, 0, 2, 3])
    apply_material(b, kinds[2 % len(kinds)])
    b.shape_trianglemesh([(-1.9, 0.0, 1.2), (-0.5, 0.0, 1.6), (-0.5, 1.4, 1.6), (-1.9, 1.4, 1.2)], [0, 1, 2, 0, 2, 3])
    return b.build()


def scene_spheres(strategy="spatial", split="sah", res=40, spp=8, depth=6, sampler="sobol", lights_only=False):
    """Analytic spheres in the triangle BVH (shapes/sphere.rs): two sphere lights (one rotated and non-uniformly scaled, one
    two-sided and reversed), and as scene objects a matte full sphere, a glass sphere, a mirror sphere clipped in z and phi and a
    plastic sphere under a handedness-swapping transform.  The room's own quad light stays, so light sampling mixes shapes."""
    b = base(res=res, spp=spp, depth=depth)
    if sampler == "halton":
        b.sampler_halton(spp)
    b.integrator_path(maxdepth=depth, lightsamplestrategy=strategy)
    b.accelerator_bvh(splitmethod=split)
    T = scenes
    # a sphere light ahead of every triangle in the primitive list
    b.area_light_source_diffuse(L=(30, 26, 20))
    t = T.transform_mul(T.transform_translate(-1.2, 1.3, 0.4), T.transform_mul(T.transform_rotate_x(30.0), T.transform_scale(0.25, 0.15, 0.2)))
    b.shape_sphere(radius=1.0, object_to_world=t[0], world_to_object=t[1])
    b.no_area_light()
    room(b, light_L=(4, 4, 4))
    if not lights_only:
        b.material_matte((0.3, 0.4, 0.8), sigma=20.0)
        t = T.transform_translate(-0.9, -1.4, 0.6)
        b.shape_sphere(radius=0.6, object_to_world=t[0], world_to_object=t[1])
        b.material_glass()
        t = T.transform_translate(0.9, -1.3, -0.3)
        b.shape_sphere(radius=0.7, object_to_world=t[0], world_to_object=t[1])
        b.material_mirror()
        t = T.transform_mul(T.transform_translate(0.2, 0.1, 1.1), T.transform_rotate_x(-70.0))
        b.shape_sphere(radius=0.55, zmin=-0.3, zmax=0.45, phimax=250.0, object_to_world=t[0], world_to_object=t[1])
        b.material_plastic()
        t = T.transform_mul(T.transform_translate(-0.2, -0.6, -0.9), T.transform_scale(0.4, -0.4, 0.4))
        b.shape_sphere(radius=1.0, object_to_world=t[0], world_to_object=t[1])
    # a two-sided light sphere with reversed orientation, after the triangles
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=(6, 8, 12), twosided=True)
    b.reverse_orientation = True
    t = T.transform_translate(1.3, 0.9, 0.8)
    b.shape_sphere(radius=0.2, object_to_world=t[0], world_to_object=t[1])
    b.reverse_orientation = False
    b.no_area_light()
    return b.build()


def scene_textures(res=48, spp=8, depth=5, sampler="sobol", aamode="closedform", lens=False):
    """Procedural textures (src/textures/) driving material parameters: a closed-form filtered checkerboard floor (uv mapping
    with scale / offset) whose checks are themselves a mix and a uv texture, a 3-D checkerboard under a transform on a matte
    sphere mesh with Oren-Nayar sigma from a bilerp float texture, a planar-mapped checkerboard on plastic Kd with a scale
    texture on Ks, spherical / cylindrical mappings on two analytic spheres (uber Kd / opacity, metal eta)."""
    b = base(res=res, spp=spp, depth=depth)
    if sampler == "halton":
        b.sampler_halton(spp)
    if lens:        # thin lens: the offset rays start at the lens sample (perspective.rs:146-165)
        b.camera_perspective(fov=40.0, lensradius=0.08, focaldistance=6.0)
    T = scenes
    s = 2.0
    uvt = b.texture_uv(uscale=3.0, vscale=2.0)
    mixt = b.texture_mix((0.8, 0.2, 0.1), (0.1, 0.3, 0.8), amount=b.texture_bilerp(0.1, 0.9, 0.6, 0.3))
    floor = b.texture_checkerboard(mixt, uvt, uscale=6.0, vscale=6.0, udelta=0.25, vdelta=0.1, aamode=aamode)
    b.material_matte(floor)
    scenes._quad(b, (s, -s, -s), (-s, -s, -s), (-s, -s, s), (s, -s, s))
    b.material_matte((0.7, 0.7, 0.7))
    scenes._quad(b, (s, s, -s), (s, s, s), (-s, s, s), (-s, s, -s))
    planar = b.texture_checkerboard((0.9, 0.9, 0.2), (0.2, 0.2, 0.2), mapping="planar", v1=(1.5, 0.0, 0.0), v2=(0.0, 1.5, 0.3), udelta=0.2, vdelta=0.4)
    b.material_plastic(Kd=planar, Ks=b.texture_scale((0.5, 0.5, 0.5), b.texture_checkerboard(1.0, 0.2, uscale=10.0, vscale=10.0)), roughness=0.05)
    scenes._quad(b, (s, -s, s), (-s, -s, s), (-s, s, s), (s, s, s))
    b.material_matte((0.2, 0.6, 0.3))
    scenes._quad(b, (-s, -s, s), (-s, -s, -s), (-s, s, -s), (-s, s, s))
    b.material_matte((0.7, 0.2, 0.2))
    scenes._quad(b, (s, -s, -s), (s, -s, s), (s, s, s), (s, s, -s))
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=(10, 9, 8))
    h = 0.999 * s
    scenes._quad(b, (0.5, h, -0.5), (0.5, h, 0.5), (-0.5, h, 0.5), (-0.5, h, -0.5))
    b.no_area_light()
    # 3-D checkerboard under a rotation + scale, sigma from a float texture
    t3 = T.transform_mul(T.transform_rotate_x(25.0), T.transform_scale(3.0, 3.0, 3.0))
    c3 = b.texture_checkerboard((0.9, 0.5, 0.1), (0.1, 0.1, 0.4), dimension=3, to_world=t3)
    b.material_matte(c3, sigma=b.texture_bilerp(0.0, 40.0, 10.0, 60.0))
    P, N, UV, idx = uv_sphere((-1.0, -1.2, 0.4), 0.7)
    b.shape_trianglemesh(P, idx, N=N, uv=UV)
    # analytic spheres with spherical / cylindrical mappings (their own world_to_texture)
    ts = T.transform_translate(0.9, -1.3, -0.2)
    sph_tex = b.texture_checkerboard((0.8, 0.8, 0.8), (0.15, 0.3, 0.15), mapping="spherical", uscale=1.0, to_world=ts, aamode=aamode)
    b.material_uber(Kd=b.texture_scale(sph_tex, (8.0, 8.0, 8.0)) if False else sph_tex, Ks=(0.2, 0.2, 0.2),
                    opacity=b.texture_checkerboard((1.0, 1.0, 1.0), (0.3, 0.3, 0.3), mapping="cylindrical", to_world=ts))
    b.shape_sphere(radius=0.65, object_to_world=ts[0], world_to_object=ts[1])
    tm = T.transform_translate(0.1, 0.2, 1.2)
    b.material_metal(eta=b.texture_checkerboard((0.2, 0.92, 1.1), (1.5, 0.9, 0.4), uscale=4.0, vscale=8.0), k=(3.9, 2.45, 2.14), roughness=0.1)
    b.shape_sphere(radius=0.5, object_to_world=tm[0], world_to_object=tm[1])
    return b.build()


def scene_sphere_lit_mixed(res=48, spp=8, depth=5):
    """A sphere light over the room, with a textured Matte, a constant plastic and a constant mirror quad in it: every segment of the
    material-sorted queue (Matte | constant lobe lists | textured) is non-empty and goes through the sphere-capable kernels."""
    b = base(res=res, spp=spp, depth=depth)
    T = scenes
    b.area_light_source_diffuse(L=(30, 26, 20))
    t = T.transform_translate(-1.0, 1.2, 0.2)
    b.shape_sphere(radius=0.25, object_to_world=t[0], world_to_object=t[1])
    b.no_area_light()
    room(b, light_L=(4, 4, 4))
    b.material_matte(b.texture_checkerboard((0.8, 0.2, 0.2), (0.2, 0.8, 0.2), uscale=4.0, vscale=4.0))
    scenes._quad(b, (-1.5, -1.2, 1.0), (-0.3, -1.2, 1.0), (-0.3, -1.2, -0.4), (-1.5, -1.2, -0.4))
    b.material_plastic(Kd=(0.3, 0.4, 0.5), Ks=(0.3, 0.3, 0.3), roughness=0.2)
    scenes._quad(b, (0.2, -1.0, 1.0), (1.5, -1.0, 1.0), (1.5, -1.0, -0.4), (0.2, -1.0, -0.4))
    b.material_mirror()
    scenes._quad(b, (-0.8, -0.6, 1.8), (0.8, -0.6, 1.8), (0.8, 0.9, 1.8), (-0.8, 0.9, 1.8))
    return b.build()


def scene_roughness_textures(res=48, spp=8, depth=6, sampler="sobol"):
    """Float textures behind "roughness" / "uroughness" / "vroughness" / "eta" (ABI 6): evaluated at every hit, roughness through
    roughness_to_alpha's `ln` on the device (plastic.rs:57-62, glass.rs:57-81, metal.rs:58-69, uber.rs:66,96-104,
    substrate.rs:45-54, trowbridge_reitz.rs:113-121).  A plastic wall whose roughness is a checkerboard, a rough-glass sphere with
    bilerp u/v roughness and a checkerboard index (its smooth checks make the glass specular there), a metal sphere whose only
    "roughness" is a texture (uroughness / vroughness fall back to it) with remapping off, an uber mesh with a textured vroughness
    beside a constant uroughness, and a substrate floor with fbm roughness."""
    b = base(res=res, spp=spp, depth=depth)
    if sampler == "halton":
        b.sampler_halton(spp)
    T = scenes
    s = 2.0
    b.material_substrate(Kd=(0.4, 0.3, 0.2), Ks=(0.3, 0.3, 0.3), uroughness=b.texture_scale(b.texture_fbm(octaves=4, roughness=0.6), 0.4),
                         vroughness=b.texture_bilerp(0.02, 0.3, 0.3, 0.02))
    scenes._quad(b, (s, -s, -s), (-s, -s, -s), (-s, -s, s), (s, -s, s))
    b.material_matte((0.7, 0.7, 0.7))
    scenes._quad(b, (s, s, -s), (s, s, s), (-s, s, s), (-s, s, -s))
    b.material_plastic(Kd=(0.3, 0.4, 0.7), Ks=(0.5, 0.5, 0.5), roughness=b.texture_checkerboard(0.02, 0.4, uscale=5.0, vscale=5.0, aamode="none"))
    scenes._quad(b, (s, -s, s), (-s, -s, s), (-s, s, s), (s, s, s))
    b.material_matte((0.2, 0.6, 0.3))
    scenes._quad(b, (-s, -s, s), (-s, -s, -s), (-s, s, -s), (-s, s, s))
    b.material_matte((0.7, 0.2, 0.2))
    scenes._quad(b, (s, -s, -s), (s, -s, s), (s, s, s), (s, s, -s))
    b.material_matte((0.5, 0.5, 0.5))
    b.area_light_source_diffuse(L=(10, 9, 8))
    h = 0.999 * s
    scenes._quad(b, (0.5, h, -0.5), (0.5, h, 0.5), (-0.5, h, 0.5), (-0.5, h, -0.5))
    b.no_area_light()
    tg = T.transform_translate(0.9, -1.3, -0.2)
    b.material_glass(eta=b.texture_checkerboard(1.3, 1.7, uscale=3.0, vscale=3.0, aamode="none"),
                     uroughness=b.texture_checkerboard(0.0, 0.15, uscale=2.0, vscale=4.0, aamode="none"),
                     vroughness=b.texture_checkerboard(0.0, 0.05, uscale=2.0, vscale=4.0, aamode="none"))
    b.shape_sphere(radius=0.65, object_to_world=tg[0], world_to_object=tg[1])
    tm = T.transform_translate(0.1, 0.2, 1.2)
    b.material_metal(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), roughness=b.texture_bilerp(0.01, 0.2, 0.08, 0.3), remaproughness=False)
    b.shape_sphere(radius=0.5, object_to_world=tm[0], world_to_object=tm[1])
    b.material_uber(Kd=(0.3, 0.3, 0.1), Ks=(0.4, 0.4, 0.4), Kr=(0.1, 0.1, 0.1), uroughness=0.05, vroughness=b.texture_checkerboard(0.02, 0.3, uscale=6.0, vscale=6.0),
                    eta=b.texture_bilerp(1.2, 1.6, 1.4, 1.8))
    P, N, UV, idx = uv_sphere((-1.0, -1.2, 0.4), 0.7)
    b.shape_trianglemesh(P, idx, N=N, uv=UV)
    return b.build()


# The scene of test_host_frontend.py::test_texture_directives_equal_programmatic_scene as .pbrt text (also rendered on the
# device by test_gpu_features.py): every texture class on the path, bound through shape and material parameter lists.
TEXTURED_PBRT = '''
    LookAt 0 0 -6.5  0 0 0  0 1 0
    Camera "perspective" "float fov" 40
    Film "image" "integer xresolution" 32 "integer yresolution" 32
    Sampler "sobol" "integer pixelsamples" 4
    Integrator "path" "integer maxdepth" 4
    WorldBegin
      AttributeBegin
        AreaLightSource "diffuse" "rgb L" [10 9 8]
        Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0.5 1.99 -0.5  0.5 1.99 0.5  -0.5 1.99 0.5  -0.5 1.99 -0.5]
      AttributeEnd
      Texture "uvt" "spectrum" "uv" "float uscale" 3 "float vscale" 2
      Texture "amt" "float" "bilerp" "float v00" 0.1 "float v01" 0.9 "float v10" 0.6 "float v11" 0.3
      Texture "mixt" "color" "mix" "rgb tex1" [0.8 0.2 0.1] "rgb tex2" [0.1 0.3 0.8] "texture amount" "amt"
      Texture "floor" "spectrum" "checkerboard" "texture tex1" "mixt" "texture tex2" "uvt" "float uscale" 6 "float vscale" 6
              "float udelta" 0.25 "float vdelta" 0.1
      Material "matte" "texture Kd" "floor"
      Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [2 -2 -2  -2 -2 -2  -2 -2 2  2 -2 2]
      Texture "planar" "spectrum" "checkerboard" "rgb tex1" [0.9 0.9 0.2] "rgb tex2" [0.2 0.2 0.2] "string mapping" "planar"
              "vector v1" [1.5 0 0] "vector v2" [0 1.5 0.3] "float udelta" 0.2 "float vdelta" 0.4 "string aamode" "none"
      Texture "fine" "spectrum" "checkerboard" "rgb tex1" [1 1 1] "rgb tex2" [0.2 0.2 0.2] "float uscale" 10 "float vscale" 10
      Texture "ks" "spectrum" "scale" "rgb tex1" [0.5 0.5 0.5] "texture tex2" "fine"
      Material "plastic" "texture Kd" "planar" "texture Ks" "ks" "float roughness" 0.05
      Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [2 -2 2  -2 -2 2  -2 2 2  2 2 2]
      AttributeBegin
        Rotate 25 1 0 0
        Scale 3 3 3
        Texture "c3" "spectrum" "checkerboard" "integer dimension" 3 "rgb tex1" [0.9 0.5 0.1] "rgb tex2" [0.1 0.1 0.4]
      AttributeEnd
      AttributeBegin
        Translate 0.9 -1.3 -0.2
        Texture "sph" "spectrum" "checkerboard" "string mapping" "spherical" "rgb tex1" [0.8 0.8 0.8] "rgb tex2" [0.15 0.3 0.15]
        Texture "sig" "float" "bilerp" "float v00" 0 "float v01" 40 "float v10" 10 "float v11" 60
        Material "matte" "texture Kd" "c3"
        Shape "sphere" "float radius" 0.65 "texture sigma" "sig"
      AttributeEnd
      Material "uber" "texture Kd" "sph" "rgb Ks" [0.2 0.2 0.2]
      Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-2 -2 2  -2 -2 -2  -2 2 0]
    WorldEnd
    '''


def scene_noise_textures(res=48, spp=8, depth=4, sampler="sobol"):
    """Perlin-noise textures (core/texture/noise.rs): dots on the floor, fbm / wrinkled / windy as Matte sigma and as colours
    through scale / mix, marble on a sphere; each under its own 3-D mapping transform (the octave count of fbm follows the
    camera ray's differentials at the first hit and is max_octaves afterwards)."""
    b = base(res=res, spp=spp, depth=depth)
    if sampler == "halton":
        b.sampler_halton(spp)
    T = scenes
    s = 2.0
    dots = b.texture_dots((0.8, 0.8, 0.7), (0.7, 0.1, 0.1), uscale=5.0, vscale=5.0)
    b.material_matte(dots)
    scenes._quad(b, (s, -s, -s), (-s, -s, -s), (-s, -s, s), (s, -s, s))
    t1 = T.transform_scale(2.0, 2.0, 2.0)
    wr = b.texture_wrinkled(octaves=6, roughness=0.6, to_world=t1)
    b.material_matte(b.texture_scale((0.9, 0.8, 0.5), wr))
    scenes._quad(b, (s, -s, s), (-s, -s, s), (-s, s, s), (s, s, s))
    t2 = T.transform_mul(T.transform_rotate_x(40.0), T.transform_scale(1.5, 1.5, 1.5))
    fb = b.texture_fbm(octaves=8, roughness=0.5, to_world=t2)
    b.material_plastic(Kd=b.texture_mix((0.1, 0.2, 0.7), (0.9, 0.9, 0.9), amount=fb), Ks=(0.2, 0.2, 0.2), roughness=0.1)
    scenes._quad(b, (-s, -s, s), (-s, -s, -s), (-s, s, -s), (-s, s, s))
    b.material_matte(b.texture_scale((0.4, 0.6, 0.9), b.texture_windy(to_world=T.transform_scale(3.0, 3.0, 3.0))), sigma=b.texture_scale(60.0, b.texture_fbm(octaves=3)))
    scenes._quad(b, (s, -s, -s), (s, -s, s), (s, s, s), (s, s, -s))
    b.material_matte((0.7, 0.7, 0.7))
    scenes._quad(b, (s, s, -s), (s, s, s), (-s, s, s), (-s, s, -s))
    b.area_light_source_diffuse(L=(10, 9, 8))
    h = 0.999 * s
    scenes._quad(b, (0.5, h, -0.5), (0.5, h, 0.5), (-0.5, h, 0.5), (-0.5, h, -0.5))
    b.no_area_light()
    tm = T.transform_translate(0.0, -1.0, 0.3)
    b.material_matte(b.texture_marble(octaves=8, roughness=0.5, scale=4.0, variation=0.4, to_world=tm))
    b.shape_sphere(radius=0.9, object_to_world=tm[0], world_to_object=tm[1])
    return b.build()


def scene_bump(res=48, spp=8, depth=4, lens=False):
    """Bump mapping (core/material.rs:31-72): displacement textures bending the shading frame of a plain quad (zero dndu),
    a smooth-shaded mesh (dndu / dndv from vertex normals, triangle.rs:405-437), an analytic sphere (Weingarten dndu / dndv)
    and a mirror; a constant bump map given as a number; displacement evaluated at the shifted points with the camera ray's
    differentials at the first hit and with the 0.0005 fallback afterwards."""
    b = base(res=res, spp=spp, depth=depth)
    if lens:
        b.camera_perspective(fov=40.0, lensradius=0.05, focaldistance=6.0)
    T = scenes
    s = 2.0
    wr = b.texture_scale(0.05, b.texture_wrinkled(octaves=5, roughness=0.5, to_world=T.transform_scale(4.0, 4.0, 4.0)))
    b.material_matte((0.6, 0.6, 0.6), bumpmap=wr)
    scenes._quad(b, (s, -s, -s), (-s, -s, -s), (-s, -s, s), (s, -s, s))
    chk = b.texture_checkerboard(0.03, 0.0, uscale=8.0, vscale=8.0)
    b.material_plastic(Kd=(0.7, 0.3, 0.2), Ks=(0.3, 0.3, 0.3), roughness=0.1, bumpmap=chk)
    scenes._quad(b, (s, -s, s), (-s, -s, s), (-s, s, s), (s, s, s))
    b.material_mirror(bumpmap=b.texture_scale(0.02, b.texture_dots(1.0, 0.0, uscale=6.0, vscale=6.0)))
    scenes._quad(b, (-s, -s, s), (-s, -s, -s), (-s, s, -s), (-s, s, s))
    b.material_matte((0.7, 0.2, 0.2), bumpmap=0.1)
    scenes._quad(b, (s, -s, -s), (s, -s, s), (s, s, s), (s, s, -s))
    b.material_matte((0.7, 0.7, 0.7))
    scenes._quad(b, (s, s, -s), (s, s, s), (-s, s, s), (-s, s, -s))
    b.area_light_source_diffuse(L=(10, 9, 8))
    h = 0.999 * s
    scenes._quad(b, (0.5, h, -0.5), (0.5, h, 0.5), (-0.5, h, 0.5), (-0.5, h, -0.5))
    b.no_area_light()
    fb = b.texture_scale(0.2, b.texture_fbm(octaves=6, to_world=T.transform_scale(5.0, 5.0, 5.0)))
    b.material_matte((0.3, 0.5, 0.8), sigma=30.0, bumpmap=fb)
    P, N, UV, idx = uv_sphere((-0.9, -1.2, 0.3), 0.75)
    b.shape_trianglemesh(P, idx, N=N, uv=UV)
    ts = T.transform_translate(0.9, -1.25, -0.3)
    b.material_plastic(Kd=(0.2, 0.6, 0.3), Ks=(0.4, 0.4, 0.4), roughness=0.05, bumpmap=b.texture_scale(0.1, b.texture_windy(to_world=T.transform_scale(6.0, 6.0, 6.0))))
    b.shape_sphere(radius=0.7, object_to_world=ts[0], world_to_object=ts[1])
    return b.build()


def test_image(w, h, channels=3, seed=3):
    """A deterministic image with structure at several scales (so MIP levels differ) in texture orientation."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 0.5 + 0.5 * np.sin(x * (2 * np.pi * 3 / w)) * np.cos(y * (2 * np.pi * 2 / h))
    stripes = ((x.astype(np.int32) // max(1, w // 16) + y.astype(np.int32) // max(1, h // 8)) % 2).astype(np.float32)
    noise = rng.random((h, w), dtype=np.float32)
    chans = [0.6 * base + 0.3 * stripes + 0.1 * noise, 0.3 * base + 0.5 * noise + 0.2 * stripes, 0.8 * stripes * base + 0.2 * noise]
    img = np.stack(chans[:channels], -1).astype(np.float32)
    return img


def scene_imagemaps(res=48, spp=8, depth=4, sampler="sobol", trilinear=False, lens=False):
    """Image-map textures (textures/imagemap.rs, core/texture/mipmap.rs) over caller-built pyramids: EWA (default) or trilinear
    lookups, repeat / clamp / black wrap modes, a non-square RGB image on the floor under a uv scale, a float image driving
    Matte sigma and a bump map, spherical mapping on an analytic sphere, a planar mapping on the back wall."""
    b = base(res=res, spp=spp, depth=depth)
    if sampler == "halton":
        b.sampler_halton(spp)
    if lens:
        b.camera_perspective(fov=40.0, lensradius=0.05, focaldistance=6.0)
    T = scenes
    s = 2.0
    rgb = b.image_pyramid(test_image(64, 32, 3))
    gray = b.image_pyramid(test_image(32, 32, 1, seed=7)[..., 0])
    small = b.image_pyramid(test_image(8, 16, 3, seed=11))
    b.material_matte(b.texture_imagemap(rgb, trilinear=trilinear, uscale=3.0, vscale=2.0, udelta=0.13, vdelta=0.4))
    scenes._quad(b, (s, -s, -s), (-s, -s, -s), (-s, -s, s), (s, -s, s))
    b.material_plastic(Kd=b.texture_imagemap(small, trilinear=trilinear, wrap="clamp", mapping="planar", v1=(0.4, 0.0, 0.0), v2=(0.0, 0.4, 0.0), udelta=0.5, vdelta=0.5),
                       Ks=(0.2, 0.2, 0.2), roughness=0.1)
    scenes._quad(b, (s, -s, s), (-s, -s, s), (-s, s, s), (s, s, s))
    b.material_matte(b.texture_scale((0.9, 0.6, 0.3), b.texture_imagemap(rgb, trilinear=trilinear, swrap="black", twrap="repeat", uscale=1.6, vscale=1.6, udelta=-0.3)),
                     sigma=b.texture_scale(60.0, b.texture_imagemap(gray, trilinear=trilinear, maxanisotropy=2.0)))
    scenes._quad(b, (-s, -s, s), (-s, -s, -s), (-s, s, -s), (-s, s, s))
    b.material_matte((0.7, 0.3, 0.3), bumpmap=b.texture_scale(0.08, b.texture_imagemap(gray, trilinear=trilinear, uscale=2.0, vscale=2.0)))
    scenes._quad(b, (s, -s, -s), (s, -s, s), (s, s, s), (s, s, -s))
    b.material_matte((0.7, 0.7, 0.7))
    scenes._quad(b, (s, s, -s), (s, s, s), (-s, s, s), (-s, s, -s))
    b.area_light_source_diffuse(L=(10, 9, 8))
    h = 0.999 * s
    scenes._quad(b, (0.5, h, -0.5), (0.5, h, 0.5), (-0.5, h, 0.5), (-0.5, h, -0.5))
    b.no_area_light()
    ts = T.transform_translate(0.3, -1.1, 0.2)
    b.material_uber(Kd=b.texture_imagemap(rgb, trilinear=trilinear, mapping="spherical", to_world=ts), Ks=(0.3, 0.3, 0.3), roughness=0.05)
    b.shape_sphere(radius=0.85, object_to_world=ts[0], world_to_object=ts[1])
    return b.build()


def scene_instances(split="sah", res=48, spp=8, depth=5, sampler="sobol"):
    """Object instancing (scene_context.rs:1327-1391, core/primitive/transformed_primitive.rs): an object of a smooth-shaded
    blob + an analytic glass sphere + a plastic quad instanced four times (translate, rotate + non-uniform scale, a mirrored
    = handedness-swapping transform, a tiny far copy), a one-triangle object (wrapped without an accelerator), instances
    interleaved with world triangles and spheres in the primitive order, a light inside an object (ignored)."""
    b = base(res=res, spp=spp, depth=depth)
    if sampler == "halton":
        b.sampler_halton(spp)
    b.accelerator_bvh(splitmethod=split)
    T = scenes
    b.object_begin("thing")
    b.material_matte((0.3, 0.5, 0.8), sigma=20.0)
    P, N, UV, idx = uv_sphere((0.0, 0.0, 0.0), 0.45, nt=6, nphi=8)
    b.shape_trianglemesh(P, idx, N=N, uv=UV)
    b.material_glass()
    ts = T.transform_translate(0.0, 0.75, 0.0)
    b.shape_sphere(radius=0.3, object_to_world=ts[0], world_to_object=ts[1])
    b.material_plastic(Kd=b.texture_checkerboard((0.9, 0.8, 0.2), (0.2, 0.2, 0.2), uscale=4.0, vscale=4.0), Ks=(0.3, 0.3, 0.3), roughness=0.1)
    b.area_light_source_diffuse(L=(50, 50, 50))             # "Area lights not supported with object instancing": ignored
    scenes._quad(b, (-0.6, -0.46, -0.6), (0.6, -0.46, -0.6), (0.6, -0.46, 0.6), (-0.6, -0.46, 0.6))
    b.no_area_light()
    b.object_end()
    b.object_begin("shard")
    b.material_mirror()
    b.shape_trianglemesh([(-0.5, 0.0, 0.0), (0.5, 0.0, 0.1), (0.0, 0.9, 0.05)], [0, 1, 2])
    b.object_end()
    # an instance ahead of every world triangle
    b.object_instance("thing", T.transform_translate(-1.1, -1.5, 0.5))
    room(b)
    b.object_instance("thing", T.transform_mul(T.transform_translate(1.0, -1.3, 0.2), T.transform_mul(T.transform_rotate_x(35.0), T.transform_scale(1.2, 0.7, 1.0))))
    b.material_matte((0.6, 0.6, 0.6))
    ts2 = T.transform_translate(0.0, 1.2, 1.2)
    b.shape_sphere(radius=0.25, object_to_world=ts2[0], world_to_object=ts2[1])
    b.object_instance("thing", T.transform_mul(T.transform_translate(-0.2, 0.3, 1.4), T.transform_scale(-0.8, 0.8, 0.8)))
    b.object_instance("shard", T.transform_translate(0.2, -1.9, -0.9))
    b.object_instance("shard", T.transform_mul(T.transform_translate(-1.5, -0.5, 1.6), T.transform_rotate_x(-20.0)))
    b.object_instance("thing", T.transform_mul(T.transform_translate(1.6, 1.5, 1.7), T.transform_scale(0.2, 0.2, 0.2)))
    return b.build()


def scene_hlbvh_cluster():
    """More than maxnodeprims primitives in one Morton cell (a tight cluster, 40 exact duplicates) next to a sparse shell:
    emit_lbvh runs out of code bits and falls back to centroid medians (hlbvh.rs:102-157, :183-192)."""
    b = scenes.SceneBuilder()
    b.look_at((0, 0, -5), (0, 0, 0), (0, 1, 0)); b.camera_perspective(fov=40.0)
    b.film(xresolution=16, yresolution=16); b.pixel_filter_box(); b.sampler_sobol(1); b.integrator_path(maxdepth=1)
    b.accelerator_bvh("hlbvh", 4)
    b.material_matte((0.5, 0.5, 0.5))
    rng = np.random.default_rng(2)
    for k in range(60):
        c = np.array([0.3, 0.2, 0.1]) + rng.random(3) * 1e-5
        b.shape_trianglemesh([tuple(c), tuple(c + [1e-6, 0, 0]), tuple(c + [0, 1e-6, 0])], [0, 1, 2])
    for k in range(40):
        b.shape_trianglemesh([(-0.5, -0.5, 0.5), (-0.4, -0.5, 0.5), (-0.5, -0.4, 0.5)], [0, 1, 2])
    for k in range(200):
        c = rng.random(3) * 4 - 2
        b.shape_trianglemesh([tuple(c), tuple(c + [0.05, 0, 0]), tuple(c + [0, 0.05, 0.02])], [0, 1, 2])
    return b.build()


def scene_ao(sampler="sobol", cossample=True, nsamples=16, spp=4, res=40, kind="boxes"):
    """Integrator "ao": an enclosure open at the top (escaping occlusion rays) with random matte clutter; kind "spheres" adds an
    analytic sphere with a partial sweep, "instances" the instanced object of scene_instances."""
    if kind == "instances":
        sd = scene_instances(split="sah", res=res, spp=spp, sampler=sampler)
        sd.desc.integrator, sd.desc.ao_samples, sd.desc.ao_cos_sample = pkg.capi.PT_INTEGRATOR_AO, nsamples, int(cossample)
        return sd
    b = scenes.SceneBuilder()
    b.look_at((0, 0.4, -3.4), (0, -0.2, 0), (0, 1, 0))
    b.camera_perspective(fov=42.0)
    b.film(xresolution=res, yresolution=res - 8)
    b.pixel_filter_box()
    b.sampler_sobol(spp) if sampler == "sobol" else b.sampler_halton(spp)
    b.integrator_ao(nsamples=nsamples, cossample=cossample)
    b.accelerator_bvh("sah", 4)
    b.material_matte((0.5, 0.5, 0.5))
    b.shape_trianglemesh([(1, -1, -1), (-1, -1, -1), (-1, -1, 1), (1, -1, 1)], [0, 1, 2, 0, 2, 3])       # floor
    b.shape_trianglemesh([(1, -1, 1), (-1, -1, 1), (-1, 1, 1), (1, 1, 1)], [0, 1, 2, 0, 2, 3])           # back wall
    b.shape_trianglemesh([(-1, -1, 1), (-1, -1, -1), (-1, 1, -1), (-1, 1, 1)], [0, 1, 2, 0, 2, 3],
                         N=[(1, 0, 0)] * 4, uv=[(0, 0), (1, 0), (1, 1), (0, 1)])                            # side wall with normals / uv
    rng = np.random.default_rng(17)
    c = rng.uniform(-0.8, 0.8, (300, 3)).astype(np.float32)
    c[:, 1] = rng.uniform(-1.0, -0.2, 300)
    off = rng.uniform(-0.12, 0.12, (300, 3, 3)).astype(np.float32)
    b.material_plastic(Kd=(0.3, 0.3, 0.3), Ks=(0.2, 0.2, 0.2), roughness=0.1)
    b.shape_trianglemesh_fast((c[:, None, :] + off).reshape(-1, 3), np.arange(900), twosided=True)
    if kind == "spheres":
        T = scenes
        t = T.transform_mul(T.transform_translate(0.3, -0.5, 0.1), T.transform_rotate_x(30.0))
        b.shape_sphere(radius=0.4, zmin=-0.3, zmax=0.35, phimax=300.0, object_to_world=t[0], world_to_object=t[1])
    return b.build()


# ---- committed golden fixtures of the other SamplerIntegrators (tools/make_golden.py writes them from the oracle; tests/test_oracle_kat.py
# holds the oracle to them, tests/test_gpu_features.py the device): name -> (scene, tile of per-sample radiance)
def _golden_integrator(kind):
    import importlib
    capi = importlib.import_module("pbrt-r3_amd").capi
    if kind == "directlighting":         # strategy "all", three samples per light: the 2-D sample arrays (and quirk Q23) are in play
        sd = scene_materials_render(["glass", "mirror", "plastic"], spp=4)
        sd.desc.integrator, sd.desc.direct_strategy, sd.desc.max_depth = capi.PT_INTEGRATOR_DIRECTLIGHTING, capi.PT_DIRECT_ALL, 4
        for i in range(sd.desc.n_area_lights):
            sd.desc.area_lights[i].n_samples = 3
    elif kind == "whitted":              # glass + mirror trees to depth 4
        sd = scene_materials_render(["glass", "mirror", "metal"], spp=4)
        sd.desc.integrator, sd.desc.max_depth = capi.PT_INTEGRATOR_WHITTED, 4
    else:                                # ao: 16 cosine-distributed occlusion rays per camera sample
        from helpers import scenes
        sd = scenes.cornell_box(res=32, spp=4)
        sd.desc.integrator, sd.desc.ao_samples, sd.desc.ao_cos_sample = capi.PT_INTEGRATOR_AO, 16, 1
    return sd


GOLDEN_INTEGRATORS = {
    "directlighting_all_ns3_40x40_4spp": lambda: _golden_integrator("directlighting"),
    "whitted_depth4_40x40_4spp": lambda: _golden_integrator("whitted"),
    "ao_16cos_cornell_32x32_4spp": lambda: _golden_integrator("ao"),
}


def golden_tile(info):
    """The 12x12 tile whose per-sample radiance a fixture holds: the middle of the film (objects, their shadows and reflections)."""
    sb = list(info.sample_bounds)
    cx, cy = (sb[0] + sb[2]) // 2, (sb[1] + sb[3]) // 2
    return (cx - 6, cy - 6, cx + 6, cy + 6)


def scene_instance_swarm(split="sah", maxnodeprims=4, n_inst=36, res=48, spp=8, depth=6):
    """What the fixed instancing scene does not reach: world leaves that hold SEVERAL instances, with triangles before, between and behind them (a ray that
    enters an instance leaves the rest of its leaf on its stack and comes back to it), overlapping instances of a tree deep enough to matter
    (3 000 triangles, some of them glass), one-triangle objects among them (wrapped without an accelerator: tested on the spot), any-hit rays
    that end inside an object."""
    b = base(res=res, spp=spp, depth=depth)
    b.accelerator_bvh(splitmethod=split, maxnodeprims=maxnodeprims)
    T = scenes
    rng = np.random.default_rng(41)
    n = 3000
    c = rng.uniform(-0.5, 0.5, (n, 1, 3)).astype(np.float32)
    verts = (c + rng.uniform(-0.06, 0.06, (n, 3, 3)).astype(np.float32)).reshape(-1, 3)
    b.object_begin("cloud")
    b.material_matte((0.6, 0.45, 0.3))
    b.shape_trianglemesh(verts[:6000], np.arange(6000))
    b.material_glass()
    b.shape_trianglemesh(verts[6000:], np.arange(3 * n - 6000))
    b.object_end()
    b.object_begin("shard")
    b.material_mirror()
    b.shape_trianglemesh([(-0.3, 0.0, 0.0), (0.3, 0.0, 0.1), (0.0, 0.5, 0.05)], [0, 1, 2])
    b.object_end()
    room(b)
    b.material_matte((0.4, 0.4, 0.7))
    for k in range(n_inst):
        p = rng.uniform(-1.2, 1.2, 3)
        sc = float(rng.uniform(0.4, 1.1))
        m = T.transform_mul(T.transform_translate(float(p[0]), float(p[1]), float(p[2])), T.transform_mul(T.transform_rotate_x(float(rng.uniform(-60, 60))), T.transform_scale(sc, sc * (-1.0 if k % 7 == 3 else 1.0), sc)))
        b.object_instance("shard" if k % 5 == 4 else "cloud", m)
        if k % 3 == 0:          # a world triangle between the instances (primitive order = creation order)
            q = rng.uniform(-1.0, 1.0, 3).astype(np.float32)
            b.shape_trianglemesh([tuple(q), tuple(q + np.float32([0.3, 0.0, 0.05])), tuple(q + np.float32([0.0, 0.3, 0.1]))], [0, 1, 2])
    return b.build()


# ---- LightSource "infinite" scenes (lights/infinite.rs) for the device-against-oracle parity tests and the env golden fixture
ENV_MAPS = ("constant", "image", "wide", "tall", "row", "column", "holes")


def env_map_image(kind, seed=5):
    """The environment maps of the parity matrix: None (constant), 2:1, 8:1 (make_distribution's lookup lands on level 1), 1:4, 1 x N,
    N x 1, and a 2:1 map with all-black rows and columns (zero-probability cells of the Distribution2D, pdf_li 0 there)."""
    if kind == "constant":
        return None
    if kind == "holes":
        img = 0.2 + test_image(32, 16, 3, seed=seed)
        img[:, 4:9] = 0.0
        img[6:9] = 0.0
        img[0] = 0.0
        return img
    w, h = {"image": (32, 16), "wide": (64, 8), "tall": (8, 32), "row": (16, 1), "column": (1, 16)}[kind]
    return 0.2 + test_image(w, h, 3, seed=seed)


def env_transform(kind):
    """light_to_world of the map: identity, rotated, mirrored (swaps handedness), non-uniformly scaled (sample_li and pdf_li do not
    normalise their directions, le does)."""
    T = scenes
    rot = T.transform_mul(T.transform_rotate_x(-70.0), T.transform_mul(T.transform_rotate_x(20.0), T.transform_scale(1.0, 1.0, 1.0)))
    if kind == "identity":
        return None
    if kind == "rotated":
        return rot
    if kind == "mirrored":
        return T.transform_mul(T.transform_scale(-1.0, 1.0, 1.0), rot)
    return T.transform_mul(T.transform_scale(2.0, 0.5, 1.25), rot)


def scene_env(integrator="path", strategy="spatial", materials=("matte",), env_map="image", transform="identity", order="after", n_env=1,
              sampler="sobol", nsamples=1, far=False, area_light=True, res=24, spp=8, depth=4, L=(1.0, 0.9, 0.8)):
    """A floor with objects of the given materials under an environment.  order: the environment read "before" or "after" the area lights;
    n_env = 2 adds a second (constant) environment at the other end of the list.  far: an instance and a sphere far from the origin set the
    world bound (the radius r of the shadow target p + wi * 2r).  integrator "directlighting" takes strategy "all" / "one"."""
    T = scenes
    b = scenes.SceneBuilder()
    b.look_at((0.0, -4.0, 1.6), (0.0, 0.0, 0.4), (0.0, 0.0, 1.0))
    b.camera_perspective(fov=62.0)
    b.film(xresolution=res, yresolution=res)
    b.pixel_filter_box()
    b.sampler_sobol(spp) if sampler == "sobol" else b.sampler_halton(spp)
    if integrator == "path":
        b.integrator_path(maxdepth=depth, lightsamplestrategy=strategy)
    elif integrator == "directlighting":
        b.integrator_directlighting(maxdepth=depth, strategy=strategy)
    else:
        b.integrator_whitted(maxdepth=depth)
    img = env_map_image(env_map)
    l2w = env_transform(transform)

    def env(second=False):
        if second:
            b.light_infinite(L=(0.3, 0.35, 0.5), nsamples=2)
        else:
            b.light_infinite(L=L, image=img, light_to_world=None if l2w is None else l2w[0].reshape(4, 4),
                             world_to_light=None if l2w is None else l2w[1].reshape(4, 4), nsamples=nsamples)
    if order == "before":
        env()
        if n_env == 2:
            env(second=True)
    if area_light:
        b.area_light_source_diffuse(L=(4.0, 3.5, 3.0), nsamples=2)
        b.shape_trianglemesh([(-0.4, -0.3, 2.2), (0.4, -0.3, 2.2), (0.4, 0.5, 2.2), (-0.4, 0.5, 2.2)], [0, 2, 1, 0, 3, 2])
        b.no_area_light()
    if order == "after" and n_env == 2:
        env(second=True)
    b.material_matte((0.6, 0.55, 0.5))
    b.shape_trianglemesh([(-3, -3, 0), (3, -3, 0), (3, 3, 0), (-3, 3, 0)], [0, 1, 2, 0, 2, 3])
    xs = np.linspace(-1.3, 1.3, max(1, len(materials))) if len(materials) > 1 else [0.0]
    for k, (m, x) in enumerate(zip(materials, xs)):
        x = float(x)
        if m == "matte":
            b.material_matte((0.7, 0.4, 0.3))
        elif m == "plastic":
            b.material_plastic(Kd=(0.3, 0.4, 0.5), Ks=(0.4, 0.4, 0.4), roughness=0.15)
        elif m == "mirror":
            b.material_mirror(Kr=(0.9, 0.9, 0.85))
        elif m == "glass":
            b.material_glass(Kr=(1.0, 1.0, 1.0), Kt=(1.0, 1.0, 1.0), eta=1.5)
        elif m == "metal":
            b.material_metal(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), roughness=0.05)
        elif m == "textured":
            b.material_matte(Kd=b.texture_checkerboard(tex1=(0.8, 0.2, 0.2), tex2=(0.2, 0.8, 0.2), uscale=4, vscale=4))
        if m in ("glass", "sphere"):
            if m == "sphere":
                b.material_matte((0.7, 0.7, 0.7))
            t = T.transform_translate(x, 0.0, 0.45)
            b.shape_sphere(radius=0.42, object_to_world=t[0], world_to_object=t[1])
        elif m == "instanced":
            b.object_begin("env_q%d" % k)
            b.material_plastic(Kd=(0.5, 0.7, 0.3), Ks=(0.2, 0.2, 0.2), roughness=0.3)
            b.shape_trianglemesh([(-0.25, 0, 0), (0.25, 0, 0), (0.25, 0, 0.5), (-0.25, 0, 0.5)], [0, 1, 2, 0, 2, 3])
            b.object_end()
            for j in range(3):
                b.object_instance("env_q%d" % k, T.transform_mul(T.transform_translate(x + 0.3 * (j - 1), 0.25 * j, 0.05),
                                                                  T.transform_rotate_x(15.0 * j)))
        else:           # a quad tilted towards the camera: mirror and metal show the sky and the floor in it
            b.shape_trianglemesh([(x - 0.4, 0.2, 0.0), (x + 0.4, 0.2, 0.0), (x + 0.4, 0.6, 0.9), (x - 0.4, 0.6, 0.9)], [0, 1, 2, 0, 2, 3])
    if far:
        b.object_begin("env_far")
        b.material_matte((0.5, 0.5, 0.5))
        b.shape_trianglemesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [0, 1, 2])
        b.object_end()
        b.object_instance("env_far", T.transform_translate(60.0, 90.0, 25.0))
        t = T.transform_translate(-40.0, 120.0, -8.0)
        b.material_matte((0.4, 0.4, 0.6))
        b.shape_sphere(radius=2.0, object_to_world=t[0], world_to_object=t[1])
    if order == "after":
        env()
    elif order == "middle" and n_env == 1:
        env()
    return b.build()


def scene_env_golden():
    """The environment-lit fixture (tools/make_golden.py): an image-mapped sky under a rotation, a mirror and a glass sphere next to a
    plastic quad, directlighting "all" with samples 3, Halton."""
    return scene_env("directlighting", "all", ("mirror", "glass", "plastic"), env_map="image", transform="rotated", order="before",
                     sampler="halton", nsamples=3, res=32, spp=4, depth=4)


# ---- alpha masks that vary inside their triangles (shapes/alphamask.rs) for the device-against-oracle parity tests and the masked fixture
ALPHA_MASKS = ("image16_repeat", "image16_black", "image64_clamp_trilinear", "checker_closedform", "checker_none", "bilerp", "scale", "mix",
               "fbm", "wrinkled", "windy", "checker3d", "planar", "spherical", "cylindrical")


def alpha_mask_texture(b, kind):
    """A float texture that crosses zero inside the triangles it masks.  The names of alpha_mask_ref.cases() (uv-mapped image maps,
    checkerboards, bilerp, scale, mix), the noise textures (their octave count comes from log2 of a zero footprint), a 3-D checkerboard,
    and image / bilerp / checkerboard textures under the planar, spherical and cylindrical mappings."""
    import alpha_mask_ref as am
    T = scenes
    tw = T.transform_mul(T.transform_translate(0.3, -0.2, 0.1), T.transform_mul(T.transform_rotate_x(35.0), T.transform_scale(0.8, 1.3, 0.6)))
    if kind == "fbm":
        return b.texture_fbm(octaves=6, roughness=0.6, to_world=tw)
    if kind == "wrinkled":
        return b.texture_mix(-0.4, 0.6, amount=b.texture_wrinkled(octaves=5, roughness=0.5))
    if kind == "windy":
        return b.texture_windy(to_world=tw)
    if kind == "checker3d":
        return b.texture_checkerboard(0.5, -0.5, dimension=3, to_world=T.transform_mul(T.transform_rotate_x(20.0), T.transform_scale(0.45, 0.6, 0.35)))
    if kind == "planar":
        return b.texture_imagemap(b.image_pyramid(am.noise_image(16)), wrap="repeat", mapping="planar", v1=(0.31, 0.1, -0.05), v2=(-0.08, 0.27, 0.12), udelta=0.2, vdelta=-0.1)
    if kind == "spherical":
        return b.texture_bilerp(-1.0, 0.8, 0.6, -0.7, mapping="spherical", to_world=T.transform_translate(4.0, 4.0, 0.0))
    if kind == "cylindrical":
        return b.texture_checkerboard(0.5, -0.5, mapping="cylindrical", to_world=T.transform_mul(T.transform_translate(4.0, 4.0, 0.0), T.transform_scale(8.0, 8.0, 0.7)))
    return am.cases()[kind].tex(b)


def _alpha_material(b, m):
    if m == "matte":
        b.material_matte((0.25, 0.6, 0.3))
    elif m == "mirror":
        b.material_mirror(Kr=(0.9, 0.9, 0.85))
    elif m == "glass":
        b.material_glass(Kr=(1.0, 1.0, 1.0), Kt=(1.0, 1.0, 1.0), eta=1.5)
    else:
        b.material_plastic(Kd=(0.3, 0.4, 0.5), Ks=(0.4, 0.4, 0.4), roughness=0.15)


def leaf_quads(n=6, z=2.0, size=0.55, seed=9):
    """n x n small tilted quads over [0.5, 7.5]^2, each carrying the whole [0, 1]^2 of its mask: P, indices, uv."""
    rng = np.random.default_rng(seed)
    P, idx, uv = [], [], []
    for j in range(n):
        for i in range(n):
            c = np.array([0.5 + 7.0 * (i + 0.5) / n, 0.5 + 7.0 * (j + 0.5) / n, z]) + rng.uniform(-0.15, 0.15, 3)
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            u = np.cross(ax, [0.0, 0.0, 1.0]); u /= np.linalg.norm(u)
            v = np.cross(ax, u) * 0.7 + np.array([0.0, 0.0, 0.3])
            k = len(P)
            P += [c - size * u - size * v, c + size * u - size * v, c + size * u + size * v, c - size * u + size * v]
            uv += [(0, 0), (1, 0), (1, 1), (0, 1)]
            idx += [k, k + 1, k + 2, k, k + 2, k + 3]
    return np.array(P, np.float32), np.array(idx), np.array(uv, np.float32)


def scene_alpha(integrator="path", strategy="spatial", on="matte", under="matte", sampler="sobol", extra=None, mask="image16_repeat", shadow=None,
                emitter=None, split="sah", maxnodeprims=4, res=24, spp=4, depth=4):
    """A room (floor, two walls, an emitter above) around a masked canopy -- one large quad whose mask varies across it, uv running past
    [0, 1] -- and masked foliage above it: small tilted quads each carrying the whole mask.  on / under: the material of the masked
    meshes and of the floor beneath them.  shadow: a second mask as "shadowalpha".  emitter: the mask of a masked area light
    (sampled everywhere, seen only where it passes).  extra: "sphere", "instance" (the foliage as an object under a rotated, non-uniformly
    scaled and mirrored instance: the masks see object space), "env"."""
    T = scenes
    b = scenes.SceneBuilder()
    b.look_at((4, -3, 7), (4, 4, 0.5), (0, 0, 1))
    b.camera_perspective(fov=60)
    b.film(xresolution=res, yresolution=res)
    b.pixel_filter_box()
    (b.sampler_sobol if sampler == "sobol" else b.sampler_halton)(pixelsamples=spp)
    if integrator == "path":
        b.integrator_path(maxdepth=depth, lightsamplestrategy=strategy)
    elif integrator == "directlighting":
        b.integrator_directlighting(maxdepth=depth, strategy=strategy)
    elif integrator == "whitted":
        b.integrator_whitted(maxdepth=depth)
    else:
        b.integrator_ao(nsamples=4)
    b.accelerator_bvh(splitmethod=split, maxnodeprims=maxnodeprims)
    a_tex = alpha_mask_texture(b, mask)
    kw = {"alpha": a_tex}
    if shadow is not None:
        kw["shadowalpha"] = alpha_mask_texture(b, shadow)
    _alpha_material(b, under)
    b.shape_trianglemesh([-1, -1, 0, 9, -1, 0, 9, 9, 0, -1, 9, 0], [0, 1, 2, 0, 2, 3])
    b.material_matte(Kd=(0.5, 0.45, 0.4))
    b.shape_trianglemesh([-1, 9, 0, 9, 9, 0, 9, 9, 4, -1, 9, 4], [0, 1, 2, 0, 2, 3])
    b.shape_trianglemesh([9, -1, 0, 9, 9, 0, 9, 9, 4, 9, -1, 4], [0, 1, 2, 0, 2, 3])
    if integrator != "ao":
        b.area_light_source_diffuse(L=(6, 6, 5))
        b.shape_trianglemesh([2, 2, 3.9, 6, 2, 3.9, 6, 6, 3.9, 2, 6, 3.9], [0, 2, 1, 0, 3, 2])
        b.no_area_light()
        if emitter is not None:
            b.area_light_source_diffuse(L=(3, 2, 1), twosided=True, nsamples=2)
            b.shape_trianglemesh([0.5, 7.5, 0.4, 3.5, 7.5, 0.4, 3.5, 8.2, 2.6, 0.5, 8.2, 2.6], [0, 1, 2, 0, 2, 3], uv=[(0, 0), (1, 0), (1, 1), (0, 1)],
                                 alpha=alpha_mask_texture(b, emitter))
            b.no_area_light()
    _alpha_material(b, on)
    b.shape_trianglemesh([0.5, 0.5, 1.2, 7.5, 0.5, 1.0, 7.5, 7.5, 1.2, 0.5, 7.5, 1.4], [0, 1, 2, 0, 2, 3], uv=[(-0.25, -0.25), (1.25, -0.25), (1.25, 1.25), (-0.25, 1.25)], **kw)
    P, idx, uv = leaf_quads()
    if extra == "instance":
        m = T.transform_mul(T.transform_translate(4.0, 4.2, 2.1), T.transform_mul(T.transform_rotate_x(25.0), T.transform_scale(0.8, -1.1, 0.6)))
        Po = (np.concatenate([P, np.ones((len(P), 1), np.float32)], 1) @ np.asarray(m[1], np.float64).reshape(4, 4).T)[:, :3].astype(np.float32)
        b.object_begin("foliage")
        b.shape_trianglemesh(Po, idx, uv=uv, **kw)
        b.shape_trianglemesh(Po[:12] + np.float32([0.0, 0.0, 0.4]), idx[:18])            # unmasked triangles in the same object tree
        b.object_end()
        b.object_instance("foliage", m)
    else:
        b.shape_trianglemesh(P, idx, uv=uv, **kw)
        b.shape_trianglemesh(P[:24] + np.float32([0.1, 0.1, 0.5]), idx[:36])                # a mesh without uv: the default (0,0), (1,0), (1,1)
        b.shape_trianglemesh(P[24:48] + np.float32([0.1, 0.1, 0.5]), idx[:36], **kw)
    if extra == "sphere":
        _alpha_material(b, "glass" if on != "glass" else "matte")
        t = T.transform_translate(6.5, 2.5, 2.0)
        b.shape_sphere(radius=0.6, object_to_world=t[0], world_to_object=t[1])
    if extra == "env":
        b.light_infinite(L=(0.3, 0.35, 0.4))
    return b.build()


def scene_alpha_golden():
    """The masked fixture (tools/make_golden.py): image-masked canopy and foliage with a checkerboard "shadowalpha", a masked emitter,
    a mirror floor, path tracing with Halton."""
    return scene_alpha("path", "spatial", on="plastic", under="mirror", sampler="halton", mask="image16_repeat", shadow="checker_closedform",
                       emitter="bilerp", res=32, spp=4, depth=4)


# The render matrix of tests/test_gpu_alpha_mask_parity.py: (integrator, strategy, on, under, sampler, extra, mask, shadowalpha, emitter).
# The first five columns -- integrator with its strategy (7 values), the material on the masked meshes and the one under them (4 each),
# sampler (2), extra (4) -- are pairwise: every pair of values of any two of them is in some row (28 rows, the least that 7 x 4 allows;
# tests/test_alpha_mask_oracle.py::test_render_matrix_is_pairwise counts them).  The 15 mask kinds appear as "alpha" at least once each,
# not paired with the other columns; "shadowalpha" and the masked emitter's mask (none under ao, which has no lights) vary freely.
ALPHA_RENDERS = [
    ("path", "uniform", "matte", "plastic", "sobol", None, "image16_repeat", None, "bilerp"),
    ("path", "uniform", "mirror", "mirror", "halton", "sphere", "image16_black", "checker3d", None),
    ("path", "uniform", "glass", "glass", "halton", "instance", "image64_clamp_trilinear", "image16_repeat", "wrinkled"),
    ("path", "uniform", "plastic", "matte", "sobol", "env", "checker_closedform", None, "checker3d"),
    ("path", "power", "matte", "glass", "sobol", None, "checker_none", "fbm", "spherical"),
    ("path", "power", "mirror", "plastic", "halton", "sphere", "bilerp", "planar", None),
    ("path", "power", "glass", "matte", "halton", "env", "scale", None, "image64_clamp_trilinear"),
    ("path", "power", "plastic", "mirror", "halton", "instance", "mix", "bilerp", "checker_none"),
    ("path", "spatial", "matte", "mirror", "halton", "env", "fbm", "wrinkled", "scale"),
    ("path", "spatial", "mirror", "matte", "sobol", "instance", "wrinkled", None, None),
    ("path", "spatial", "glass", "glass", "sobol", None, "windy", "image64_clamp_trilinear", "windy"),
    ("path", "spatial", "plastic", "plastic", "halton", "sphere", "checker3d", "scale", "planar"),
    ("directlighting", "all", "matte", "mirror", "sobol", "env", "planar", None, "cylindrical"),
    ("directlighting", "all", "mirror", "glass", "halton", "sphere", "spherical", "cylindrical", None),
    ("directlighting", "all", "glass", "plastic", "halton", None, "cylindrical", "checker_closedform", "checker_closedform"),
    ("directlighting", "all", "plastic", "matte", "halton", "instance", "image16_repeat", None, "bilerp"),
    ("directlighting", "one", "matte", "glass", "halton", "env", "image16_black", "checker3d", "mix"),
    ("directlighting", "one", "mirror", "plastic", "halton", "instance", "image64_clamp_trilinear", "image16_repeat", None),
    ("directlighting", "one", "glass", "mirror", "sobol", "sphere", "checker_closedform", None, "checker3d"),
    ("directlighting", "one", "plastic", "matte", "halton", None, "checker_none", "fbm", "spherical"),
    ("whitted", None, "matte", "matte", "sobol", "sphere", "bilerp", "planar", "image16_repeat"),
    ("whitted", None, "mirror", "mirror", "halton", None, "scale", None, None),
    ("whitted", None, "glass", "plastic", "halton", "instance", "mix", "bilerp", "checker_none"),
    ("whitted", None, "plastic", "glass", "sobol", "env", "fbm", "wrinkled", "scale"),
    ("ao", None, "matte", "mirror", "halton", "instance", "wrinkled", None, None),
    ("ao", None, "mirror", "plastic", "sobol", "env", "windy", "image64_clamp_trilinear", None),
    ("ao", None, "glass", "glass", "halton", None, "checker3d", "scale", None),
    ("ao", None, "plastic", "matte", "halton", "sphere", "planar", None, None),
]


def alpha_render_name(row):
    integ, strat, on, under, sampler, extra = row[:6]
    return "%s_%s_on_%s_%s_%s" % (integ if strat is None else integ + "_" + strat, on, under, sampler, extra or "plain")


def alpha_render_scene(row):
    integ, strat, on, under, sampler, extra, mask, shadow, emitter = row
    return scene_alpha(integ, strat, on=on, under=under, sampler=sampler, extra=extra, mask=mask, shadow=shadow, emitter=emitter,
                       spp=8 if sampler == "sobol" else 6)


# ---- textures held to float64 (tests/texture_ref.py): one description drives the scene builder and the float64 evaluator.
# A spec is a dict {"type": ..., parameters under the scene file's names}; children ("tex1", "tex2", "amount") are specs, numbers or RGB
# triples; an imagemap carries its level-0 image under "image"; "to_world" is a (m, m_inv) pair as the transform_* helpers return.
_SPEC_2D = ("mapping", "uscale", "vscale", "udelta", "vdelta", "v1", "v2", "to_world")


def texture_from_spec(b, spec):
    """The builder's texture for a spec (recursively): a Tex handle, or the constant itself."""
    if not isinstance(spec, dict):
        return tuple(spec) if isinstance(spec, (tuple, list)) else float(spec)
    ch = lambda k, d: texture_from_spec(b, spec.get(k, d))
    kw = {k: spec[k] for k in _SPEC_2D if k in spec}
    kind = spec["type"]
    if kind == "scale":
        return b.texture_scale(ch("tex1", 1.0), ch("tex2", 1.0))
    if kind == "mix":
        return b.texture_mix(ch("tex1", 1.0), ch("tex2", 1.0), ch("amount", 0.5))
    if kind == "checkerboard":
        if spec.get("dimension", 2) == 3:
            return b.texture_checkerboard(ch("tex1", 1.0), ch("tex2", 0.0), dimension=3, to_world=spec.get("to_world"))
        return b.texture_checkerboard(ch("tex1", 1.0), ch("tex2", 0.0), aamode=spec.get("aamode", "closedform"), **kw)
    if kind == "dots":
        return b.texture_dots(ch("tex1", 1.0), ch("tex2", 0.0), **kw)
    if kind == "imagemap":
        names = {0: "repeat", 1: "black", 2: "clamp"}
        return b.texture_imagemap(b.image_pyramid(spec["image"]), trilinear=spec.get("trilinear", False), maxanisotropy=spec.get("maxanisotropy", 8.0),
                                  swrap=names[spec.get("swrap", spec.get("wrap", 0))], twrap=names[spec.get("twrap", spec.get("wrap", 0))], **kw)
    if kind == "uv":
        return b.texture_uv(**kw)
    if kind == "bilerp":
        return b.texture_bilerp(spec["v00"], spec["v01"], spec["v10"], spec["v11"], **kw)
    if kind in ("fbm", "wrinkled"):
        return getattr(b, "texture_" + kind)(octaves=spec.get("octaves", 8), roughness=spec.get("roughness", 0.5), to_world=spec.get("to_world"))
    if kind == "windy":
        return b.texture_windy(to_world=spec.get("to_world"))
    if kind == "marble":
        return b.texture_marble(octaves=spec.get("octaves", 8), roughness=spec.get("roughness", 0.5), scale=spec.get("scale", 1.0),
                                variation=spec.get("variation", 0.2), to_world=spec.get("to_world"))
    raise ValueError(kind)


def texture_ref_spec(spec, pyramid):
    """The same spec as texture_ref.evaluate reads it: the image replaced by its pyramid (`pyramid`: texture_ref.pyramid), to_world by
    the matrix the texture maps points with -- the inverse for the 2-D mappings (mapping2d.rs:190-198), tex2world itself for the 3-D
    ones (IdentityMapping3D::new(tex2world): fbm.rs:42, wrinkled.rs:42, windy.rs:38, marble.rs:87, checkerboard.rs:152)."""
    if not isinstance(spec, dict):
        return spec
    out = {k: (texture_ref_spec(v, pyramid) if k in ("tex1", "tex2", "amount") else v) for k, v in spec.items() if k not in ("image", "to_world")}
    if "image" in spec:
        out["levels"] = pyramid(spec["image"])
    if spec.get("to_world") is not None:
        three_d = spec["type"] in ("fbm", "wrinkled", "windy", "marble") or (spec["type"] == "checkerboard" and spec.get("dimension", 2) == 3)
        out["world_to_texture"] = np.asarray(spec["to_world"][0 if three_d else 1], np.float32).astype(np.float64).reshape(4, 4)
    return out


# ---- the observable of the filtered texture value (tests/test_gpu_texture_truth.py, test_texture_oracle.py): one planar quad with
# explicit uv, tilted against the view so that the footprint runs from mildly to strongly anisotropic across the tile, a Mirror whose
# Kr is the texture under test, and one light of radiance 1 in every direction: a constant infinite light ("env" rows; the reflected ray
# escapes) or a closed box of two-sided diffuse emitters around camera and quad ("box" rows; the reflected ray ends on an emitter,
# whose matte Kd is 0).  Either way the radiance of a sample is Kr (clamped at zero, mirror.rs:32) as filtered with that camera ray's
# differentials.  The two lights select different shading kernels on the device: with an infinite light the wavefront shades every
# material in k_shade_env / k_shade_env_inst (ptk_shade returns before the material sort and the textured split), which call the
# __noinline__ instantiation of the texture code; without one, and without instances, the textured hits of `path` go through
# k_tex_resolve -- the __forceinline__ instantiation with its value buffer in LDS -- and k_shade_general_res, and an instanced scene
# through k_shade_general_inst.
TRUTH_RES, TRUTH_TILE = 20, (2, 2, 18, 18)
TRUTH_EYE, TRUTH_LOOK, TRUTH_UP, TRUTH_FOV = (0.0, 2.4, -1.6), (0.0, 0.0, 0.6), (0.0, 1.0, 0.0), 80.0
TRUTH_QUAD = [(-4.0, -0.3, -2.5), (4.0, -0.3, -2.5), (4.0, 0.6, 6.5), (-4.0, 0.6, 6.5)]
TRUTH_UV = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
TRUTH_LENS = (0.05, 3.5)          # lensradius, focaldistance of the thin-lens rows


_TRUTH_IMAGES = {}


def truth_image(channels):
    """1024 x 512 texels in [0.1, 0.9]: one or two periods of a sine across the image.  The quad shows a fraction of a period (the uv
    scales below are < 1), so the texels under one footprint differ by a few hundredths of the range: what a texel that takes the
    neighbouring entry of the EWA weight table can change is proportional to that difference, and so is what a wrong filter changes,
    while the line below which a derived bound counts (1e-3 of the range) is not."""
    if channels not in _TRUTH_IMAGES:
        y, x = np.mgrid[0:512, 0:1024]
        out = np.empty((512, 1024, channels), np.float32)
        for k in range(channels):
            out[:, :, k] = 0.5 + 0.4 * np.sin(2 * np.pi * ((1 + k % 2) * x / 1024.0 + (1 + (k + 1) % 2) * y / 512.0) + k)
        _TRUTH_IMAGES[channels] = out
    return _TRUTH_IMAGES[channels]


def truth_texture_spec(name):
    rgb, mono = truth_image(3), truth_image(1)
    dense = dict(uscale=0.25, vscale=0.4)                               # a footprint of a few texels at the tile's centre
    edge = dict(uscale=0.5, vscale=0.8, udelta=-0.2, vdelta=-0.2)       # st runs from -0.05 to 0.43: the image's corner is in view
    tw = scenes.transform_mul(scenes.transform_translate(0.3, 0.1, -0.2), scenes.transform_mul(scenes.transform_rotate_x(-40.0), scenes.transform_scale(2.0, 3.5, 0.6)))
    checker = dict(type="checkerboard", tex1=(0.9, 0.8, 0.1), tex2=(0.1, 0.2, 0.7), uscale=15.0, vscale=13.0)
    return {
        "ewa1": dict(type="imagemap", image=rgb, maxanisotropy=1.0, wrap=0, **dense),
        "ewa8": dict(type="imagemap", image=rgb, maxanisotropy=8.0, wrap=0, **dense),
        "ewa16": dict(type="imagemap", image=rgb, maxanisotropy=16.0, wrap=0, uscale=0.25, vscale=1.2),
        "trilinear": dict(type="imagemap", image=rgb, trilinear=True, wrap=0, **dense),
        "mono_ewa": dict(type="scale", tex1=dict(type="imagemap", image=mono, maxanisotropy=8.0, wrap=0, **dense), tex2=(0.9, 0.5, 0.7)),
        "mono_trilinear": dict(type="scale", tex1=dict(type="imagemap", image=mono, trilinear=True, wrap=2, **dense), tex2=(0.4, 0.8, 0.6)),
        "ewa_black": dict(type="imagemap", image=rgb, maxanisotropy=8.0, wrap=1, **edge),
        "ewa_clamp": dict(type="imagemap", image=rgb, maxanisotropy=8.0, wrap=2, **edge),
        "ewa_deltas": dict(type="imagemap", image=rgb, maxanisotropy=8.0, wrap=0, uscale=1.5, vscale=0.3, udelta=0.25, vdelta=-0.5),
        "planar": dict(type="imagemap", image=rgb, trilinear=True, wrap=0, mapping="planar", v1=(0.5, 0.1, 0.0), v2=(0.1, 0.2, 0.6), udelta=0.2, vdelta=0.1),
        "spherical": dict(type="imagemap", image=rgb, trilinear=True, wrap=0, mapping="spherical", to_world=scenes.transform_translate(0.3, 1.5, 0.2)),
        "checker": checker,
        "checker_none": dict(checker, aamode="none"),
        "fbm": dict(type="fbm", octaves=6, roughness=0.6, to_world=tw),
        "wrinkled": dict(type="wrinkled", octaves=5, roughness=0.5, to_world=tw),
        "windy": dict(type="windy", to_world=tw),
        "marble": dict(type="marble", octaves=6, roughness=0.5, scale=2.0, variation=0.4),
        "dots": dict(type="dots", tex1=(0.9, 0.1, 0.1), tex2=(0.1, 0.9, 0.9), uscale=8.0, vscale=8.0),
        "mix": dict(type="mix", tex1=dict(type="imagemap", image=rgb, maxanisotropy=8.0, wrap=0, **dense), tex2=checker, amount=dict(type="fbm", octaves=3, roughness=0.5, to_world=tw)),
    }[name]


TRUTH_TEXTURES = ["ewa1", "ewa8", "ewa16", "trilinear", "mono_ewa", "mono_trilinear", "ewa_black", "ewa_clamp", "ewa_deltas", "planar", "spherical",
                  "checker", "checker_none", "fbm", "wrinkled", "windy", "marble", "dots", "mix"]


def _truth_rows():
    """(texture, camera, sampler, spp, placement, light).  Every texture twice under the infinite light, the second time with the four
    middle columns flipped, the first time with the bits of a counter; then once more in world space inside the emitting box -- the
    only rows `path` shades through k_tex_resolve, see scene_texture_truth -- and every fourth texture inside the box as an instance.
    Every pair of values of any two columns occurs (test_texture_oracle.py counts them)."""
    cols = (("pinhole", "lens"), ("sobol", "halton"), (4, 1), ("world", "instance"))
    rows = []
    for i, t in enumerate(TRUTH_TEXTURES):
        bits = [(i >> k) & 1 for k in range(4)]
        rows.append((t,) + tuple(c[b] for c, b in zip(cols, bits)) + ("env",))
        rows.append((t,) + tuple(c[1 - b] for c, b in zip(cols, bits)) + ("env",))
    for i, t in enumerate(TRUTH_TEXTURES):
        bits = [((5 * i + 3) >> k) & 1 for k in range(3)]
        rows.append((t,) + tuple(c[b] for c, b in zip(cols, bits)) + ("world", "box"))
        if i % 4 == 0:
            rows.append((t,) + tuple(c[1 - b] for c, b in zip(cols, bits)) + ("instance", "box"))
    return rows


TEXTURE_TRUTH = _truth_rows()
TRUTH_INTEGRATORS = ("path", "whitted")
TRUTH_DIRECTLIGHTING_ROWS = (2, 23)                                      # "directlighting" renders these two rows as well


def truth_instance_transform():
    T = scenes
    return T.transform_mul(T.transform_translate(0.2, -0.1, 0.3), T.transform_mul(T.transform_rotate_x(12.0), T.transform_scale(1.3, 0.8, 1.1)))


def truth_quad(placement):
    """The quad's vertices as the scene file gives them (float32) and in world space (float64, through the float32 matrix)."""
    P = np.asarray(TRUTH_QUAD, np.float32)
    if placement == "world":
        return P, P.astype(np.float64), None
    xf = truth_instance_transform()                                     # the object-space quad is the world one carried back, so both rows see one picture
    m, mi = (np.asarray(x, np.float32).astype(np.float64).reshape(4, 4) for x in xf)
    P = (P.astype(np.float64) @ mi[:3, :3].T + mi[:3, 3]).astype(np.float32)
    return P, P.astype(np.float64) @ m[:3, :3].T + m[:3, 3], xf


def scene_texture_truth(row, integrator):
    texture, camera, sampler, spp, placement, light = row
    b = scenes.SceneBuilder()
    b.look_at(TRUTH_EYE, TRUTH_LOOK, TRUTH_UP)
    lens = TRUTH_LENS if camera == "lens" else (0.0, 1e6)
    b.camera_perspective(fov=TRUTH_FOV, lensradius=lens[0], focaldistance=lens[1])
    b.film(xresolution=TRUTH_RES, yresolution=TRUTH_RES)
    b.pixel_filter_box()
    (b.sampler_halton if sampler == "halton" else b.sampler_sobol)(spp)
    {"path": b.integrator_path, "whitted": b.integrator_whitted, "directlighting": b.integrator_directlighting}[integrator](maxdepth=3)
    if light == "env":
        b.light_infinite(L=(1.0, 1.0, 1.0))
    else:                                                               # a closed box of two-sided emitters of radiance 1 around camera and quad
        b.material_matte(Kd=(0.0, 0.0, 0.0))
        b.area_light_source_diffuse(L=(1.0, 1.0, 1.0), twosided=True)
        c = [(x, y, z) for x in (-16.0, 16.0) for y in (-16.0, 16.0) for z in (-16.0, 16.0)]
        for f in ((0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)):
            scenes._quad(b, *[c[k] for k in f])
        b.no_area_light()
    P, _, xf = truth_quad(placement)
    if xf is not None:
        b.object_begin("quad")
    b.material_mirror(Kr=texture_from_spec(b, truth_texture_spec(texture)))
    b.shape_trianglemesh(P, [0, 1, 2, 0, 2, 3], uv=TRUTH_UV)
    if xf is not None:
        b.object_end()
        b.object_instance("quad", xf)
    return b.build()
