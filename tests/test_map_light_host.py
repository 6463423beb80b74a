"""LightSource "goniometric" / "projection" / "point" through the .pbrt front end and SceneBuilder (no GPU): the pt_map_light and
pt_delta_light records of both against each other bit for bit, the light list order, the defaults, the refusals that stay, the maps
(resized, both aspects), and the float64 restatement (tests/map_light_ref.py) alone on the scenes the GPU tests render: every region
occurs and the share of samples near a discontinuity stays under the cap."""
import ctypes as C

import numpy as np
import pytest

import delta_light_ref as dref
import map_light_cases as cases
import map_light_ref as ref
from helpers import pkg, scenes

capi = pkg.capi
f32 = np.float32
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0]\n'
NAMES = ["goniometric", "projection", "point"]


def parse(world, work_dir=None, head='Sampler "sobol"\n', **kw):
    kw.setdefault("point_lights", True)
    return capi.ParsedScene(text=head + "WorldBegin\n" + world + "WorldEnd\n", work_dir=work_dir, **kw)


def mat(a):
    return np.array(list(a), np.float64).reshape(4, 4)


def bits(a):
    return np.array(list(a), np.float32).view(np.uint32)


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


# ---------------------------------------------------------------- records
def test_front_end_and_scene_builder_give_the_same_records(tmp_path):
    """The three directives under CTM = Translate * Scale through .pbrt text and through SceneBuilder: every field bit for bit, and the
    maps' level 0 texel for texel (negatives clamped, not multiplied by the intensity)."""
    img = cases.MAP_4x2.copy()
    img[1, 2, 0] = -0.75
    write_pfm(str(tmp_path / "m.pfm"), img)
    ps = parse('Translate 1 -2 0.5\nScale 2 0.5 -1.5\n'
               'LightSource "goniometric" "rgb L" [5 4 3] "rgb scale" [0.1 0.2 0.3] "string mapname" "m.pfm"\n' + TRI +
               'LightSource "projection" "rgb I" [7 8 9] "rgb scale" [2 0.5 1] "float fov" 33 "string mapname" "m.pfm"\n'
               'LightSource "point" "rgb I" [1 2 3] "rgb scale" [3 2 1] "point from" [0.25 0.5 -1]\n', work_dir=str(tmp_path))
    sb = scenes.SceneBuilder()
    ctm = scenes.transform_mul(scenes.transform_translate(1, -2, 0.5), scenes.transform_scale(2, 0.5, -1.5))
    sb.light_goniometric(L=(5, 4, 3), scale=(0.1, 0.2, 0.3), image=img, ctm=ctm)
    sb.shape_trianglemesh([-1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0], [0, 1, 2, 0, 2, 3])
    sb.light_projection(I=(7, 8, 9), scale=(2, 0.5, 1), fov=33, image=img, ctm=ctm)
    sb.light_point(I=(1, 2, 3), scale=(3, 2, 1), frm=(0.25, 0.5, -1), ctm=ctm)
    assert len(ps.map_lights) == len(sb.map_lights) == 2 and len(ps.delta_lights) == len(sb.delta_lights) == 1
    for a, b in zip(sb.map_lights, ps.map_lights):
        assert (a.kind, a.light_index, tuple(a.resolution)) == (b.kind, b.light_index, tuple(b.resolution))
        for field in ("light_to_world", "world_to_light", "spectrum"):
            assert np.array_equal(bits(getattr(a, field)), bits(getattr(b, field))), field
        assert bits([a.fov]).tolist() == bits([b.fov]).tolist()
        mine, theirs = cases.level0(sb.images, a.image), level0(ps, b.image)
        assert ps.desc.images[b.image].channels == 3 and np.array_equal(mine.astype(f32), theirs)
        assert np.array_equal(theirs, np.maximum(img, 0))
    assert [(m.kind, m.light_index) for m in ps.map_lights] == [(capi.PT_DELTA_GONIOMETRIC, 0), (capi.PT_DELTA_PROJECTION, 1)]
    assert tuple(ps.map_lights[1].resolution) == (4, 2) and ps.map_lights[1].fov == f32(33)
    a, b = sb.delta_lights[0], ps.delta_lights[0]
    assert (a.kind, a.light_index) == (b.kind, b.light_index) == (capi.PT_DELTA_POINT, 2)
    for field in ("light_to_world", "world_to_light", "spectrum"):
        assert np.array_equal(bits(getattr(a, field)), bits(getattr(b, field))), field
    # create_point_light: Translate(from) * CTM -- the light sits at from + the CTM's translation, whatever the CTM's scale
    assert np.array_equal(mat(b.light_to_world)[:3, 3], np.array([1.25, -1.5, -0.5]))
    assert np.array_equal(mat(b.light_to_world), dref.point_light_to_world(mat(ctm[0]), (0.25, 0.5, -1)))


def test_light_list_order_among_area_infinite_spot_and_the_new_lights():
    area = 'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 1 1]\n' + TRI + 'AttributeEnd\n'
    ps = parse(area + 'LightSource "goniometric"\n' + 'LightSource "infinite" "rgb L" [0.1 0.1 0.1]\n' + 'LightSource "spot"\n' + area +
               'LightSource "projection"\n' + 'LightSource "point"\n' + 'LightSource "goniometric"\n' + TRI, delta_lights=True)
    assert [(m.kind, m.light_index) for m in ps.map_lights] == [(capi.PT_DELTA_GONIOMETRIC, 2), (capi.PT_DELTA_PROJECTION, 7), (capi.PT_DELTA_GONIOMETRIC, 9)]
    assert [il.light_index for il in ps.infinite_lights] == [3]
    assert [(d.kind, d.light_index) for d in ps.delta_lights] == [(capi.PT_DELTA_SPOT, 4), (capi.PT_DELTA_POINT, 8)]
    # SceneBuilder counts the same way
    sb = scenes.SceneBuilder()
    sb.area_light_source_diffuse()
    sb.shape_trianglemesh([-1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0], [0, 1, 2, 0, 2, 3])
    sb.no_area_light()
    assert sb.light_goniometric() == 2 and sb.light_infinite() == 3 and sb.light_spot() == 4 and sb.light_projection() == 5 and sb.light_point() == 6


def test_defaults():
    """No parameters: spectrum 1, the CTM, a 1 x 1 map of ones (three channels), fov 45, resolution 1 x 1 (make_mipmap without a path)."""
    ps = parse('LightSource "goniometric"\nLightSource "projection"\nLightSource "point"\n' + TRI)
    g, p = ps.map_lights
    for ml in (g, p):
        assert list(ml.spectrum) == [1.0, 1.0, 1.0] and np.array_equal(mat(ml.light_to_world), np.eye(4)) and np.array_equal(mat(ml.world_to_light), np.eye(4))
        im = ps.desc.images[ml.image]
        assert (im.width, im.height, im.channels, im.n_levels) == (1, 1, 3, 1) and level0(ps, ml.image).tolist() == [[[1.0, 1.0, 1.0]]]
    assert g.image != p.image
    assert p.fov == 45.0 and tuple(p.resolution) == (1, 1)
    d, = ps.delta_lights
    assert d.kind == capi.PT_DELTA_POINT and list(d.spectrum) == [1.0, 1.0, 1.0] and np.array_equal(mat(d.light_to_world), np.eye(4))
    sb = scenes.SceneBuilder()
    sb.light_projection()
    assert sb.map_lights[0].fov == 45.0 and tuple(sb.map_lights[0].resolution) == (1, 1) and cases.level0(sb.images, 0).tolist() == [[[1.0, 1.0, 1.0]]]


# ---------------------------------------------------------------- the refusals that stay
REFUSALS = {
    "goniometric": 'LightSource "goniometric": goniometric and projection lights (image lookups per sample) are not on the accelerated path',
    "projection": 'LightSource "projection": goniometric and projection lights (image lookups per sample) are not on the accelerated path',
    "point": 'LightSource "point": not enabled in the .pbrt front end yet (the C ABI and SceneBuilder.light_point take point lights); '
             'spot, distant and infinite lights and diffuse area lights are on the accelerated path',
}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("entry", ["plain", "delta_lights_option", "features_without_the_bit"])
def test_without_the_bit_the_three_names_are_refused_word_for_word(name, entry):
    kw = dict(plain={}, delta_lights_option=dict(delta_lights=True), features_without_the_bit=dict(mix_materials=True, delta_lights=True, quadric_shapes=True,
                                                                                                   disney_materials=True))[entry]
    with pytest.raises(capi.PtError) as e:
        parse('LightSource "%s"\n' % name + TRI, point_lights=False, **kw)
    assert e.value.status == 4 and REFUSALS[name] in str(e.value)
    assert len(parse('LightSource "%s"\n' % name + TRI).map_lights) == (0 if name == "point" else 1)


def test_bad_maps_and_transforms_are_refused_by_name(tmp_path):
    for name in ("goniometric", "projection"):
        with pytest.raises(capi.PtError) as e:
            parse('LightSource "%s" "string mapname" "nothing_here.pfm"\n' % name + TRI, work_dir=str(tmp_path))
        assert 'LightSource "%s"' % name in str(e.value)
    (tmp_path / "empty.pfm").write_bytes(b"PF\n0 2\n-1.0\n")
    with pytest.raises(capi.PtError) as e:
        parse('LightSource "projection" "string mapname" "empty.pfm"\n' + TRI, work_dir=str(tmp_path))
    assert 'LightSource "projection"' in str(e.value)
    for name in NAMES:               # a projective CTM (the matrix is given column by column: its last ROW gets the 0.5)
        with pytest.raises(capi.PtError) as e:
            parse('Transform [1 0 0 0.5  0 1 0 0  0 0 1 0  0 0 0 1]\nLightSource "%s"\n' % name + TRI)
        assert 'LightSource "%s"' % name in str(e.value) and "projective" in str(e.value)


# ---------------------------------------------------------------- maps: resize and both aspects
@pytest.mark.parametrize("w,h", [(4, 2), (3, 2), (2, 4)])
def test_map_resolution_is_the_file_s_and_the_pyramid_a_power_of_two(tmp_path, w, h):
    """The projection light's aspect comes from the map as read (3 x 2: aspect 1.5, though its pyramid is 4 x 2); aspect > 1 widens x,
    aspect < 1 heightens y (projection.rs:30-38)."""
    img = cases.make_map(w, h)
    write_pfm(str(tmp_path / "m.pfm"), img)
    ps = parse('LightSource "projection" "string mapname" "m.pfm"\nLightSource "goniometric" "string mapname" "m.pfm"\n' + TRI, work_dir=str(tmp_path))
    p, g = ps.map_lights
    assert tuple(p.resolution) == (w, h) and tuple(g.resolution) == (0, 0)
    im = ps.desc.images[p.image]
    pw, ph = 1 << (w - 1).bit_length(), 1 << (h - 1).bit_length()
    assert (im.width, im.height, im.channels) == (pw, ph, 3)
    if (pw, ph) == (w, h):
        assert np.array_equal(level0(ps, p.image), img)
    lt = ref.from_record(p, level0(ps, p.image))
    aspect = w / h
    assert lt.screen == ((-aspect, -1.0, aspect, 1.0) if aspect > 1 else (-1.0, -1.0 / aspect, 1.0, 1.0 / aspect))
    # cos_total_width: the corner of the screen bounds through the inverse projection, fov 45
    t = np.tan(np.radians(45.0) / 2)
    corner = np.array([lt.screen[2] * t, lt.screen[3] * t, 1.0])
    assert abs(lt.cos_total - 1.0 / np.linalg.norm(corner)) < 1e-6


# ---------------------------------------------------------------- the restatement alone
def test_restated_quirks():
    img = cases.MAP_4x2.astype(np.float64)
    # goniometric: transform_point, not transform_vector -- under a translated light the two disagree
    l2w = dref.translate((0.1, 0.2, 0.3))
    lt = ref.goniometric(l2w, (1, 1, 1), img)
    w = dref.normalize(np.array([[0.3, -0.5, -0.3]]))
    moved, _, _ = ref.gonio_scale(lt, w)
    still, _, _ = ref.gonio_scale(ref.goniometric(np.eye(4), (1, 1, 1), img), w)
    assert np.abs(moved - still).max() > 0.01
    wp = w[0] - np.array([0.1, 0.2, 0.3])
    phi = np.arctan2(wp[1], wp[0]) % (2 * np.pi)
    want, _ = ref.triangle(img, [[phi / (2 * np.pi), np.arccos(wp[2]) / np.pi]])
    assert np.allclose(moved, want, rtol=0, atol=1e-15)
    # z beyond the clamp: theta stops at pi
    far = ref.goniometric(dref.translate((0, 0, 5.0)), (1, 1, 1), img)
    v1, _, _ = ref.gonio_scale(far, [[0.0, 0.6, -0.8]])
    v2, _, _ = ref.gonio_scale(far, [[0.0, 0.8, -0.6]])
    assert np.array_equal(v1, v2)
    # projection: inclusive bounds, black behind the near plane, the divide
    pl = ref.projection(np.eye(4), (1, 1, 1), img, 90.0, (4, 2))
    assert pl.screen == (-2.0, -1.0, 2.0, 1.0) and abs(pl.proj[0, 0] - 1.0) < 1e-15
    pl.proj[0, 0] = pl.proj[1, 1] = 1.0                      # (1 / tan(pi / 4) is one ulp above 1 in float64: the corner below is meant to sit ON the edge)
    val, _, near, region = ref.projection_scale(pl, [[2.0, 1.0, 1.0], [2.0001, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.0005], [0.5, 0.25, 1.0], [1.0, 0.5, 2.0]])
    assert region.tolist() == [0, 1, 2, 2, 0, 0] and near[0] and not near[4]
    assert (val[1] == 0).all() and (val[2] == 0).all() and np.array_equal(val[4], val[5])
    # the bilinear lookup is continuous across the s wrap and across cells
    a, _ = ref.triangle(img, [[1.0 - 1e-9, 0.4]])
    b, _ = ref.triangle(img, [[1e-9, 0.4]])
    assert np.abs(a - b).max() < 1e-7
    # power: lookup((.5, .5), .5) reads the level below the top: for 4 x 2 the 2 x 1 level's mean
    c = ref.lookup_trilinear(ref.pyramid(img), (0.5, 0.5), 0.5)
    assert np.allclose(c, img.mean((0, 1)))
    assert np.allclose(ref.power(lt), 4 * np.pi * c) and np.allclose(ref.power(pl), c * 2 * np.pi * (1 - pl.cos_total))
    one = ref.goniometric(np.eye(4), (2, 3, 4), np.ones((1, 1, 3)))
    assert np.allclose(ref.power(one), 4 * np.pi * np.array([2.0, 3, 4])) and np.array_equal(ref.gonio_scale(one, w)[0], [[1.0, 1.0, 1.0]])


def test_restatement_regions_and_near_share_on_the_gpu_tests_scenes():
    """On the floor points the GPU tests' camera sees: the goniometric light is lit everywhere, the projector looking down is lit and
    black outside its image, the grazing one also black behind its plane -- and the share of samples within their bound of a
    discontinuity is under the 2 % cap for every pose, with bounds that stay useful."""
    o, d = cases.camera_rays(res=32)
    p, hit, edge = cases.plane_hit(o, d, 0.0, cases.FLOOR, cases.P_ERR)
    assert hit.sum() > 1500
    counts = {}
    for name, add in cases.LIGHTS.items():
        sb = cases.base()
        cases.floor(sb)
        add(sb)
        lt, = cases.restate_lights(sb)
        s = ref.sample_li(lt, p[hit], cases.P_ERR)
        counts[name] = np.bincount(s["region"], minlength=3)
        assert s["near"].mean() <= cases.NEAR_CAP / 4, (name, s["near"].mean())
        ok = ~s["near"] & (s["region"] == 0)
        assert (s["li"][ok] > 0).all() and s["li_rel"][ok].max() < 2e-3, (name, s["li_rel"][ok].max())
        assert (s["li"][s["region"] != 0] == 0).all()
        assert len(np.unique(np.round(s["scale"][ok], 6), axis=0)) > ok.sum() // 2           # the map varies over the floor
    assert counts["goniometric"][0] == hit.sum()
    assert counts["projection"][0] > 200 and counts["projection"][1] > 200
    assert (counts["projection_grazing"] > 100).all()
    # the hooks' points: around both lights under the translated, rotated, scaled transform
    for ctm in (None, cases.HOOK_CTM):
        m = np.eye(4) if ctm is None else mat(ctm[0])
        g = ref.goniometric(m, (1, 1, 1), cases.MAP_8x4)
        pr = ref.projection(m, (1, 1, 1), cases.MAP_8x4, 70.0, (8, 4))
        pts = cases.hook_points(m)
        sg, sp = ref.sample_li(g, pts), ref.sample_li(pr, pts)
        assert sg["near"].mean() <= cases.NEAR_CAP and sp["near"].mean() <= cases.NEAR_CAP
        assert (np.bincount(sp["region"], minlength=3) > 60).all(), np.bincount(sp["region"], minlength=3)
        assert (sg["li"][~sg["near"]] > 0).all()
