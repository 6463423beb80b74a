"""The random scene generator of tests/test_gpu_fuzz.py on the CPU: the same seed gives the same scene, and the oracle renders what it
draws (so the generator cannot rot between GPU runs)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_fuzz as fz
from helpers import pkg


def _digest(sd):
    d = sd.desc
    parts = [np.ctypeslib.as_array(d.P, shape=(3 * d.n_vertices,)).tobytes() if d.n_vertices else b"",
             np.ctypeslib.as_array(d.indices, shape=(3 * d.n_triangles,)).tobytes() if d.n_triangles else b"",
             bytes([d.integrator & 255, d.sampler & 255, d.split_method & 255, d.max_node_prims & 255]),
             np.int64([d.n_spheres, d.n_instances, d.n_materials, d.n_textures, d.spp, d.max_depth]).tobytes()]
    for il in getattr(sd, "infinite_lights", []):
        h, w = d.images[il.image].height, d.images[il.image].width
        parts += [bytes(il), np.ctypeslib.as_array(d.images[il.image].texels, shape=(3 * w * h,)).tobytes()]
    for m in getattr(sd, "alpha_masks", []):
        parts.append(bytes(m))
    if getattr(sd, "alpha_masks", []):
        parts.append(bytes(memoryview((pkg.capi.pt_texture * d.n_textures).from_address(C.addressof(d.textures.contents))).cast("B")))
    return b"".join(parts)


@pytest.mark.parametrize("seed", [0, 1, 5, 7, 970])
def test_random_scene_is_deterministic_and_renders(oracle, seed, env=False):
    a, exact_a = fz.random_scene(seed, env)
    b, exact_b = fz.random_scene(seed, env)
    assert exact_a == exact_b and _digest(a) == _digest(b)
    if env:         # the environment adds its lights and leaves every other draw alone
        plain, _ = fz.random_scene(seed)
        assert len(a.infinite_lights) in (1, 2) and a.desc.n_images >= plain.desc.n_images
        assert a.desc.integrator == plain.desc.integrator and a.desc.spp == plain.desc.spp and a.desc.n_spheres == plain.desc.n_spheres
    osc = oracle.scene(a)
    oracle.reference_panics()
    try:
        x, cnt, _ = osc.render(threads=4)
        assert np.isfinite(x).all() and cnt["camera_rays"] > 0 and cnt["regular_rays"] >= cnt["camera_rays"]
        assert (oracle.reference_panics() & 1) == (1 if seed == 970 else 0)        # seed 970: the scene that found quirk Q24
    finally:
        osc.close()


@pytest.mark.parametrize("seed", [0, 3, 11, 970])
def test_random_env_scene_is_deterministic_and_renders(oracle, seed):
    """The same seeds with one or two infinite lights drawn in (test_gpu_fuzz.random_scene(seed, env=True)), rendered by the oracle."""
    test_random_scene_is_deterministic_and_renders(oracle, seed, env=True)


def _geometry(sd):
    d = sd.desc
    mats = []                   # the materials with their texture numbers reduced to "has one": the masks' textures shift the numbering
    for i in range(d.n_materials):
        m = pkg.capi.pt_material.from_buffer_copy(d.materials[i])
        for name, _ in pkg.capi.pt_material._fields_:
            if name.startswith("tex_"):
                setattr(m, name, 1 if getattr(m, name) else 0)
        mats.append(bytes(m))
    return (np.ctypeslib.as_array(d.P, shape=(3 * d.n_vertices,)).tobytes(), np.ctypeslib.as_array(d.indices, shape=(3 * d.n_triangles,)).tobytes(),
            b"".join(mats),
            d.n_spheres, d.n_instances, d.n_meshes, d.integrator, d.sampler, d.spp, d.max_depth, d.split_method, d.max_node_prims)


@pytest.mark.parametrize("seed", [0, 1, 3, 5, 7, 11, 970])
def test_random_masked_scene_is_deterministic_and_renders(oracle, seed):
    """random_scene(seed, masks=True): the same scene twice; every draw of the main generator as without masks (same geometry, every material
    parameter up to the numbers of its textures, camera, sampler, integrator, accelerator); at least one mesh masked by a texture; and the oracle
    renders it, masks honoured, with finite output."""
    a, exact_a = fz.random_scene(seed, masks=True)
    b, exact_b = fz.random_scene(seed, masks=True)
    plain, exact_p = fz.random_scene(seed)
    assert exact_a == exact_b == exact_p and _digest(a) == _digest(b)
    ga, gp = _geometry(a), _geometry(plain)
    assert ga == gp
    assert not plain.alpha_masks and any(m.alpha_kind == pkg.capi.PT_ALPHA_TEXTURE for m in a.alpha_masks)
    assert all(m.mesh < a.desc.n_meshes for m in a.alpha_masks) and len({m.mesh for m in a.alpha_masks}) == len(a.alpha_masks)
    assert a.desc.n_textures > plain.desc.n_textures
    both, _ = fz.random_scene(seed, env=True, masks=True)              # the two extra generators do not disturb each other
    env_only, _ = fz.random_scene(seed, env=True)
    assert [bytes(m)[4:] for m in both.alpha_masks] == [bytes(m)[4:] for m in a.alpha_masks]       # (an open-topped room shifts the mesh numbers)
    assert [bytes(x)[:64] for x in both.infinite_lights] == [bytes(x)[:64] for x in env_only.infinite_lights]
    osc, osp = oracle.scene(a), oracle.scene(plain)
    oracle.reference_panics()
    try:
        x, cnt, _ = osc.render(threads=4)
        xp, cntp, _ = osp.render(threads=4)
        assert np.isfinite(x).all() and cnt["camera_rays"] == cntp["camera_rays"] > 0 and cnt["regular_rays"] >= cnt["camera_rays"]
        assert not np.array_equal(x, xp)                               # the masks are seen
    finally:
        oracle.reference_panics()
        osc.close(); osp.close()


def test_instanced_bench_scene_is_the_plain_one_copied(oracle):
    """bench.py --instances K (scenes.rt1m(instances=K)): the filler triangles become one object, instanced on a g x g x g grid.  With K = 1 the one
    instance sits under the identity (g = 1: scale 1, centre 0), so the oracle must see exactly the plain scene's image -- through TransformedPrimitive
    instead of through the world's own tree -- and with K = 8 eight scaled copies: more geometry in the same triangle arrays."""
    from helpers import pkg
    plain = pkg.scenes.rt1m(2012, res=24, spp=2, max_depth=4)
    one = pkg.scenes.rt1m(2012, res=24, spp=2, max_depth=4, instances=1)
    eight = pkg.scenes.rt1m(2012, res=24, spp=2, max_depth=4, instances=8)
    assert (plain.desc.n_instances, one.desc.n_instances, eight.desc.n_instances) == (0, 1, 8)
    assert plain.desc.n_triangles == one.desc.n_triangles == eight.desc.n_triangles
    m = list(one.desc.instances[0].instance_to_world)
    assert m == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    centres = sorted((round(eight.desc.instances[i].instance_to_world[3], 3), round(eight.desc.instances[i].instance_to_world[7], 3), round(eight.desc.instances[i].instance_to_world[11], 3))
                     for i in range(8))
    assert centres == sorted((x, y, z) for x in (-0.45, 0.45) for y in (-0.45, 0.45) for z in (-0.45, 0.45))
    imgs = []
    for sd in (plain, one, eight):
        osc = oracle.scene(sd)
        x, cnt, _ = osc.render(threads=4)
        imgs.append((x, cnt))
        osc.close()
    # identity instance: the same picture, sample for sample wherever the origin nudge of Transform::transform_ray (the error bound it adds along the
    # direction) does not send a later bounce to a neighbouring 5 mm triangle: most pixels agree to rounding, the image means closely
    a, b = imgs[0][0], imgs[1][0]
    same = np.isclose(a[..., :3], b[..., :3], rtol=1e-3, atol=1e-5).all(axis=-1).mean()
    assert same > 0.5, same
    assert abs(a[..., 1].mean() - b[..., 1].mean()) < 0.1 * a[..., 1].mean()
    assert np.array_equal(a[..., 3], b[..., 3])
    assert imgs[2][1]["nodes_visited"] > imgs[0][1]["nodes_visited"]
