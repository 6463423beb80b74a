"""The two build paths of the scene upload (pt_scene_upload.cpp: build_world_on_device, and the host's three stages) make their triangle
flags, shading records and light records with the same helpers.  One small scene that feeds those helpers every input they branch on,
uploaded under each path: same tree, same lights, same film, bit for bit."""
import numpy as np
import pytest

import feature_scenes as fs
from helpers import bits, pkg, scenes

pytestmark = pytest.mark.gpu
HOST, DEVICE = pkg.capi.BVH_BUILD_HOST, pkg.capi.BVH_BUILD_DEVICE


def scene():
    """About 300 triangles and two spheres, 32 x 32 at 4 spp: matte walls, a one-sided and a reversed plastic quad, a smooth ball with N and
    uv, a two-sided emissive quad with normals, an emissive and a plain sphere, a ball cut away by a constant-0 alpha mask."""
    b = fs.base(res=32, spp=4, depth=5)
    fs.room(b)
    b.material_plastic(Kd=(0.3, 0.4, 0.6), Ks=(0.3, 0.3, 0.3), roughness=0.15)
    scenes._quad(b, (1.6, -1.9, 0.4), (0.2, -1.9, 0.4), (0.2, -1.9, 1.6), (1.6, -1.9, 1.6), twosided=False)
    b.reverse_orientation = True
    scenes._quad(b, (-1.9, -1.0, 0.2), (-1.9, -1.0, 1.4), (-1.9, 0.6, 1.4), (-1.9, 0.6, 0.2), twosided=False)
    b.reverse_orientation = False
    P, N, UV, idx = fs.uv_sphere((-0.8, -1.2, 0.3), 0.8, 8, 12)
    b.shape_trianglemesh(P, idx, N=N, uv=UV)
    b.material_matte((0.6, 0.5, 0.4))
    b.area_light_source_diffuse(L=(4.0, 5.0, 6.0), twosided=True)
    quad = [(1.2, -0.2, 1.0), (1.9, -0.2, 0.3), (1.9, 0.9, 0.3), (1.2, 0.9, 1.0)]
    tilt = np.array([[-0.7, 0.1, -0.7], [-0.6, -0.1, -0.8], [-0.8, 0.1, -0.6], [-0.7, -0.1, -0.7]])
    b.shape_trianglemesh(quad, [0, 1, 2, 0, 2, 3], N=tilt / np.linalg.norm(tilt, axis=1, keepdims=True))
    b.area_light_source_diffuse(L=(6.0, 3.0, 2.0))
    t = scenes.transform_translate(0.7, -1.5, -0.6)
    b.shape_sphere(radius=0.35, object_to_world=t[0], world_to_object=t[1])
    b.no_area_light()
    t = scenes.transform_translate(-0.2, 0.9, 0.8)
    b.shape_sphere(radius=0.5, object_to_world=t[0], world_to_object=t[1])
    P, N, UV, idx = fs.uv_sphere((0.9, 0.2, -0.4), 0.6, 6, 10)
    b.shape_trianglemesh(P, idx, N=N, uv=UV, alpha=0.0)
    return b.build()


def test_host_and_device_paths_upload_the_same_scene():
    sd = scene()
    d = sd.desc
    assert 250 <= d.n_triangles <= 350 and d.n_spheres == 2 and len(sd.alpha_masks) == 1
    ctx = pkg.Context(0)
    try:
        got = []
        for where, on_device in ((HOST, 0), (DEVICE, 1)):
            ctx.set_bvh_build(where)
            info = ctx.upload(sd)
            assert info.bvh_on_device == on_device
            ctx.film_clear()
            ctx.render()
            got.append((ctx.bvh_digest(), info.n_lights, info.n_nodes, info.n_leaves, bits(ctx.film_xyzw())))
    finally:
        ctx.close()
    host, dev = got
    assert host[:4] == dev[:4]
    assert host[1] == 5          # the ceiling light's and the tilted quad's two triangles each, and the sphere
    assert np.array_equal(host[4], dev[4])
    assert np.isfinite(host[4].view(np.float32)).all() and host[4].view(np.float32)[..., :3].max() > 0.0
