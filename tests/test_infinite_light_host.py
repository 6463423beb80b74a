"""LightSource "infinite" in the .pbrt front end (no device needed): parameters, defaults, the alias, the CTM, the light's place in the
light list, the environment map's pyramid (lights/infinite.rs:44-67, 273-293), the kinds that stay refused, and the new kernels' budgets."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from helpers import pkg

capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = 'Sampler "sobol"\nWorldBegin\n'
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 0 0 1 0 0 1 1 0 0 1 0]\n'


def parse(body, work_dir=None):
    return capi.ParsedScene(text=HEAD + body + "WorldEnd\n", work_dir=work_dir)


def level0(ps, image):
    im = ps.desc.images[image]
    n = im.width * im.height * im.channels
    return np.ctypeslib.as_array(C.cast(im.texels, C.POINTER(C.c_float)), shape=(n,)).reshape(im.height, im.width, im.channels).copy()


def write_pfm(path, rgb_top_first):
    """Portable float map: rows stored bottom to top, little-endian."""
    a = np.asarray(rgb_top_first, np.float32)
    h, w, _ = a.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(a[::-1]).astype("<f4").tobytes())


def test_constant_light_parameters_and_defaults():
    ps = parse('LightSource "infinite"\n' + TRI)
    assert len(ps.infinite_lights) == 1
    il = ps.infinite_lights[0]
    assert il.n_samples == 1 and il.light_index == 0
    assert list(il.light_to_world) == list(np.eye(4, dtype=np.float32).reshape(-1))
    im = ps.desc.images[il.image]
    assert (im.width, im.height, im.channels, im.n_levels) == (1, 1, 3, 1)
    assert level0(ps, il.image).reshape(-1).tolist() == [1.0, 1.0, 1.0]
    ps = parse('LightSource "infinite" "rgb L" [1 2 3] "rgb scale" [2 0.5 4] "integer nsamples" [5]\n' + TRI)
    il = ps.infinite_lights[0]
    assert level0(ps, il.image).reshape(-1).tolist() == [2.0, 1.0, 12.0]
    assert il.n_samples == 5
    ps = parse('LightSource "infinite" "integer samples" [8] "integer nsamples" [5]\n' + TRI)
    assert ps.infinite_lights[0].n_samples == 8            # "samples" first, "nsamples" the fallback


def test_quick_quarters_the_sample_count(tmp_path):
    """--quick (bin/pbrt.rs:360-366): n_samples -> max(n / 4, 1)."""
    lib = capi.load_library()

    class Opts(C.Structure):
        _fields_ = [("quick", C.c_int32), ("quick_full_resolution", C.c_int32), ("pixelsamples", C.c_int32), ("reserved", C.c_int32)]
    lib.pth_parse_file_opts.argtypes = [C.c_char_p, C.POINTER(Opts), C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    lib.pth_scene_get_infinite_lights.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    lib.pth_scene_get_infinite_lights.restype = C.POINTER(capi.pt_infinite_light)
    lib.pth_scene_free.argtypes = [C.c_void_p]
    got = []
    for n, quick in ((9, 1), (3, 1), (9, 0), (0, 0)):
        f = tmp_path / ("s%d%d.pbrt" % (n, quick))
        f.write_text(HEAD + 'LightSource "infinite" "integer samples" [%d]\n' % n + TRI + "WorldEnd\n")
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        assert lib.pth_parse_file_opts(str(f).encode(), C.byref(Opts(quick, 0, 0, 0)), C.byref(h), err, 1024) == 0, err.value
        cnt = C.c_uint32()
        arr = lib.pth_scene_get_infinite_lights(h, C.byref(cnt))
        assert cnt.value == 1
        got.append(arr[0].n_samples)
        lib.pth_scene_free(h)
    assert got == [2, 1, 9, 0]             # 0 is taken as given (the library reads it as 1)


def test_alias_and_ctm():
    ps = parse('AttributeBegin\nRotate 90 0 0 1\nTranslate 1 2 3\nLightSource "exinfinite" "rgb L" [0.5 0.5 0.5]\nAttributeEnd\n' + TRI)
    assert len(ps.infinite_lights) == 1
    il = ps.infinite_lights[0]
    m = np.array(il.light_to_world, np.float64).reshape(4, 4)
    minv = np.array(il.world_to_light, np.float64).reshape(4, 4)
    c, s = np.cos(np.pi / 2), np.sin(np.pi / 2)
    rot = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    tr = np.eye(4)
    tr[:3, 3] = [1, 2, 3]
    np.testing.assert_allclose(m, rot @ tr, atol=1e-6)
    np.testing.assert_allclose(m @ minv, np.eye(4), atol=1e-6)


def test_light_list_index_follows_creation_order():
    body = ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 1 1]\n' + TRI + 'AttributeEnd\n'      # two emissive triangles
            'LightSource "infinite"\n'
            'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 1 1]\nShape "sphere" "float radius" [0.5]\nAttributeEnd\n'
            'LightSource "infinite" "rgb L" [2 2 2]\n' + TRI)
    ps = parse(body)
    assert [il.light_index for il in ps.infinite_lights] == [2, 4]
    # inside an object an area light is dropped (scene_context.rs:1302-1304): it takes no place in the list
    body = ('ObjectBegin "o"\nAreaLightSource "diffuse" "rgb L" [1 1 1]\n' + TRI + 'ObjectEnd\n'
            'LightSource "infinite"\n' + TRI)
    assert parse(body).infinite_lights[0].light_index == 0


def test_map_pyramid_top_row_at_t0_ungammad_scaled_clamped(tmp_path):
    rng = np.random.default_rng(3)
    img = rng.uniform(0.0, 2.0, (4, 8, 3)).astype(np.float32)
    img[0, 1, 2] = -1.5                                    # negative values are clamped to zero
    write_pfm(str(tmp_path / "env.pfm"), img)
    ps = parse('LightSource "infinite" "string mapname" "env.pfm" "rgb L" [2 1 0.5]\n' + TRI, work_dir=str(tmp_path))
    il = ps.infinite_lights[0]
    im = ps.desc.images[il.image]
    assert (im.width, im.height, im.channels, im.n_levels) == (8, 4, 3, 4)
    lv = level0(ps, il.image)
    want = np.maximum(img, 0.0) * np.array([2, 1, 0.5], np.float32)
    assert np.array_equal(lv, want.astype(np.float32))     # row 0 = the file's top row (no flip), no inverse gamma


def test_png_map_is_not_gamma_decoded(tmp_path):
    import struct
    import zlib
    h, w = 2, 4
    px = np.arange(h * w * 3, dtype=np.uint8).reshape(h, w, 3) * 10
    raw = b"".join(b"\x00" + px[y].tobytes() for y in range(h))

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")
    (tmp_path / "env.png").write_bytes(png)
    ps = parse('LightSource "infinite" "string mapname" "env.png"\n' + TRI, work_dir=str(tmp_path))
    lv = level0(ps, ps.infinite_lights[0].image)
    np.testing.assert_allclose(lv, px.astype(np.float32) / 255.0, rtol=1e-6)


def test_missing_map_fails_like_image_textures(tmp_path):
    with pytest.raises(capi.PtError) as e:
        parse('LightSource "infinite" "string mapname" "nope.exr"\n' + TRI, work_dir=str(tmp_path))
    assert "LightSource" in str(e.value)


@pytest.mark.parametrize("kind", ["point", "spot", "distant", "goniometric", "projection"])
def test_other_light_sources_still_refused(kind):
    with pytest.raises(capi.PtError) as e:
        parse('LightSource "%s"\n' % kind + TRI)
    assert e.value.status == 4              # PT_ERR_UNSUPPORTED
    assert "LightSource" in str(e.value)


def test_scene_builder_light_index():
    sb = pkg.scenes.SceneBuilder()
    sb.area_light_source_diffuse((1, 1, 1))
    sb.shape_trianglemesh([0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0], [0, 1, 2, 0, 2, 3])
    sb.no_area_light()
    assert sb.light_infinite(L=(1, 2, 3)) == 2
    sd = sb.build()
    assert len(sd.infinite_lights) == 1 and sd.infinite_lights[0].light_index == 2


def test_new_kernel_budgets():
    """Registers / spills of the infinite-light kernels, read from the library (tools/kernel_resources.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(capi.LIB_PATH)
    # The whole-vertex env kernels carry the texture interpreter, spheres and the map lookups and spill; the recursion kernels spill as their
    # plain-scene forms do.  The budgets are what they take now: a change may lower them, never raise them.
    budgets = {"k_shade_env": (256, 256), "k_shade_env_inst": (256, 258), "k_rec_enter_env": (256, 204), "k_rec_next_env": (256, 106),
               "k_nee_resolve_env": (32, 0), "k_light_grid_env": (256, 0), "k_light_hooks": (128, 0), "k_light_renumber": (32, 0)}
    for name, (vgpr, spill) in budgets.items():
        k = ks[name]
        assert k[".vgpr_count"] <= vgpr, (name, "registers", k[".vgpr_count"])
        assert k.get(".vgpr_spill_count", 0) <= spill, (name, "spilled registers", k.get(".vgpr_spill_count", 0))
        assert k[".group_segment_fixed_size"] <= 65536, (name, "LDS")
    for name, scratch in (("k_shade_env", 3264), ("k_shade_env_inst", 3312), ("k_rec_enter_env", 3584), ("k_rec_next_env", 3504)):
        assert ks[name][".private_segment_fixed_size"] <= scratch, (name, "scratch")
