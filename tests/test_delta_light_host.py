"""LightSource "spot" / "distant" through the .pbrt front end and SceneBuilder (no GPU): the pt_delta_light records against the float64
restatement of create_spot_light / create_distant_light / create_point_light (tests/delta_light_ref.py), the light list order, the
lights that stay refused, and the restatement's own discontinuity shares on the inputs the GPU tests use."""
import numpy as np
import pytest

import delta_light_ref as ref
from helpers import pkg, scenes

capi = pkg.capi

f32 = np.float32
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0]\n'


def parse(world, head='Sampler "sobol"\n', delta_lights=True):
    return capi.ParsedScene(text=head + "WorldBegin\n" + world + "WorldEnd\n", delta_lights=delta_lights)


def mat(a):
    return np.array(list(a), np.float64).reshape(4, 4)


def bits(a):
    return np.array(list(a), np.float32).view(np.uint32)


def rot_z(deg):
    a = np.radians(deg)
    m = np.eye(4)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return m


def product_bound(*ms):
    """Entrywise bound on an f32 product of the given factors against the float64 product.  Every entry of a 4 x 4 product is four
    roundings of products and three of sums; a chain of k factors therefore carries at most 7 k roundings on terms whose sizes add up
    to the product of the factors' absolute values.  The factors themselves are f32-rounded (1 each; the rotation's sin / cos, the
    normalised spot direction and the Gauss-Jordan inverse of dir_to_z -- 4 pivots of 8 operations -- at most 40 more)."""
    p = np.eye(4)
    for m in ms:
        p = p @ np.abs(m)
    return (7 * len(ms) + len(ms) + 40) * ref.EPS * p + 1e-30


def test_spot_defaults():
    """No parameters: I = 1, coneangle 30, conedelta 5, from the origin towards +z (spot.rs:141-147).  dir = +z takes the second branch
    of coordinate_system (|x| > |y| is false): du = +y, dv = -x, so light_to_world is a quarter turn about z, not the identity."""
    ps = parse('LightSource "spot"\n' + TRI)
    assert len(ps.delta_lights) == 1 and len(ps.infinite_lights) == 0
    dl = ps.delta_lights[0]
    assert (dl.kind, dl.light_index) == (capi.PT_DELTA_SPOT, 0)
    assert list(dl.spectrum) == [1.0, 1.0, 1.0]
    assert (dl.cone_total_width, dl.cone_falloff_start) == (30.0, 25.0)
    want = ref.spot_light_to_world(np.eye(4), (0, 0, 0), (0, 0, 1))
    assert np.array_equal(want, [[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    assert np.array_equal(mat(dl.light_to_world), want) and np.array_equal(mat(dl.world_to_light), want.T)


def test_spot_scale_and_conedeltaangle():
    ps = parse('LightSource "spot" "rgb I" [2 3 4] "rgb scale" [0.5 2 0.25] "float coneangle" 40 "float conedelta" 7 "float conedeltaangle" 12\n' + TRI)
    dl = ps.delta_lights[0]
    assert list(dl.spectrum) == [1.0, 6.0, 1.0]
    assert (dl.cone_total_width, dl.cone_falloff_start) == (40.0, 28.0)            # "conedeltaangle" overrides "conedelta" (spot.rs:144-145)
    dl = parse('LightSource "spot" "float coneangle" 40 "float conedelta" 7\n' + TRI).delta_lights[0]
    assert (dl.cone_total_width, dl.cone_falloff_start) == (40.0, 33.0)


def test_spot_from_to_under_a_rotated_scaled_ctm():
    """light_to_world = CTM * Translate(from) * Inverse(dir_to_z), CTM = Translate * Rotate(z) * Scale(non-uniform), against the float64
    product within the f32 products' bound; the stored inverse against the float64 inverse likewise (its factors in the reverse order)."""
    frm, to = (0.3, -0.2, 2.5), (0.1, 0.4, -0.5)
    ps = parse('Translate 1 -2 0.5\nRotate 35 0 0 1\nScale 2 0.5 1.5\n'
               'LightSource "spot" "point from" [%g %g %g] "point to" [%g %g %g] "float coneangle" 25 "float conedelta" 8\n' % (frm + to) + TRI)
    dl = ps.delta_lights[0]
    t, r, s = ref.translate((1, -2, 0.5)), rot_z(35), np.diag([2, 0.5, 1.5, 1.0])
    ctm = t @ r @ s
    want = ref.spot_light_to_world(ctm, frm, to)
    d, du, dv = ref.coordinate_system(ref.normalize(np.array(to) - np.array(frm)))
    rz = np.eye(4)
    rz[0, :3], rz[1, :3], rz[2, :3] = du, dv, d
    bound = product_bound(t, r, s, ref.translate(frm), rz.T)
    err = np.abs(mat(dl.light_to_world) - want)
    assert (err <= bound).all(), (err / bound).max()
    inv_bound = product_bound(rz, ref.translate(-np.array(frm)), np.diag([0.5, 2, 1 / 1.5, 1.0]), r.T, ref.translate((-1, 2, -0.5)))
    err = np.abs(mat(dl.world_to_light) - np.linalg.inv(want))
    assert (err <= inv_bound).all(), (err / inv_bound).max()
    # the light's position is the CTM's image of `from`, the axis the image of to - from
    lt = ref.from_record(dl)
    p = ctm @ np.array(frm + (1.0,))
    assert np.abs(lt.v - p[:3]).max() <= 40 * ref.EPS * np.abs(p[:3]).max()
    axis = ref.normalize(ctm[:3, :3] @ (np.array(to) - np.array(frm)))
    f, _, _ = ref.falloff(lt, axis[None, :])
    assert f[0] == 1.0


def test_light_index_counts_every_light_in_directive_order():
    """scene.lights grows as directives are read: an emissive quad (2 lights), the spot (2), an infinite light (3), a second quad (4, 5),
    a distant light (6) inside an attribute block -- which keeps the block's CTM and outlives the block."""
    area = 'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 1 1]\n' + TRI + 'AttributeEnd\n'
    ps = parse(area + 'LightSource "spot" "point from" [0 0 3] "point to" [0 0 0]\n' + 'LightSource "infinite" "rgb L" [0.1 0.1 0.1]\n' + area +
               'AttributeBegin\nTranslate 5 0 0\nScale 1 2 4\nLightSource "distant" "point from" [1 1 1] "point to" [0 0 0] "rgb L" [3 2 1] "rgb scale" [2 2 2]\nAttributeEnd\n' + TRI)
    assert [(d.kind, d.light_index) for d in ps.delta_lights] == [(capi.PT_DELTA_SPOT, 2), (capi.PT_DELTA_DISTANT, 6)]
    assert [il.light_index for il in ps.infinite_lights] == [3]
    dd = ps.delta_lights[1]
    assert list(dd.spectrum) == [6.0, 4.0, 2.0] and list(dd.direction) == [1.0, 1.0, 1.0]
    assert np.array_equal(mat(dd.light_to_world), [[1, 0, 0, 5], [0, 2, 0, 0], [0, 0, 4, 0], [0, 0, 0, 1]])
    lt = ref.from_record(dd)
    assert np.allclose(lt.v, ref.distant_w_light(mat(dd.light_to_world), (1, 1, 1), (0, 0, 0)), rtol=0, atol=1e-15)
    assert np.allclose(lt.v, np.array([1, 2, 4]) / np.sqrt(21.0))


def test_distant_defaults():
    dl = parse('LightSource "distant"\n' + TRI).delta_lights[0]
    assert dl.kind == capi.PT_DELTA_DISTANT and list(dl.spectrum) == [1.0, 1.0, 1.0]
    assert list(dl.direction) == [0.0, 0.0, -1.0]                      # from (0 0 0) - to (0 0 1): the light shines along +z
    assert np.array_equal(mat(dl.light_to_world), np.eye(4))


@pytest.mark.parametrize("name", ["goniometric", "projection"])
def test_image_driven_lights_are_refused_by_name(name):
    with pytest.raises(capi.PtError) as e:
        parse('LightSource "%s"\n' % name + TRI)
    assert e.value.status == 4 and name in str(e.value) and "LightSource" in str(e.value)


@pytest.mark.parametrize("name", ["spot", "distant"])
def test_delta_lights_are_an_option_of_the_parse(name):
    """Without pth_options.delta_lights the front end goes on refusing the two directives, with a message that names the option; with it they load."""
    with pytest.raises(capi.PtError) as e:
        parse('LightSource "%s"\n' % name + TRI, delta_lights=False)
    assert e.value.status == 4 and "LightSource" in str(e.value) and "delta_lights" in str(e.value)
    assert len(parse('LightSource "%s"\n' % name + TRI).delta_lights) == 1
    with pytest.raises(capi.PtError):
        parse('LightSource "point"\n' + TRI)                    # the point directive stays refused either way


def test_scene_builder_and_front_end_give_the_same_records():
    """The same lights through SceneBuilder.light_spot / light_distant and through .pbrt text, under CTM = Translate * Scale: every field
    bit for bit (both sides form the products in f32 in the reference's order, and invert dir_to_z by the reference's Gauss-Jordan)."""
    ps = parse('Translate 1 -2 0.5\nScale 2 0.5 1.5\n'
               'LightSource "spot" "point from" [0.3 -0.2 2.5] "point to" [0.1 0.4 -0.5] "float coneangle" 25 "float conedelta" 8 "rgb I" [5 4 3] "rgb scale" [0.1 0.2 0.3]\n'
               + TRI + 'LightSource "distant" "point from" [0.5 1 2] "point to" [0 0.25 0] "rgb L" [1 2 3]\n')
    sb = scenes.SceneBuilder()
    ctm = scenes.transform_mul(scenes.transform_translate(1, -2, 0.5), scenes.transform_scale(2, 0.5, 1.5))
    sb.light_spot(I=(5, 4, 3), scale=(0.1, 0.2, 0.3), coneangle=25, conedelta=8, frm=(0.3, -0.2, 2.5), to=(0.1, 0.4, -0.5), ctm=ctm)
    sb.shape_trianglemesh([-1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0], [0, 1, 2, 0, 2, 3])
    sb.light_distant(L=(1, 2, 3), frm=(0.5, 1, 2), to=(0, 0.25, 0), ctm=ctm)
    assert len(sb.delta_lights) == len(ps.delta_lights) == 2
    for a, b in zip(sb.delta_lights, ps.delta_lights):
        assert (a.kind, a.light_index) == (b.kind, b.light_index)
        for field in ("light_to_world", "world_to_light", "spectrum", "direction"):
            assert np.array_equal(bits(getattr(a, field)), bits(getattr(b, field))), field
        assert bits([a.cone_total_width, a.cone_falloff_start]).tolist() == bits([b.cone_total_width, b.cone_falloff_start]).tolist()


def test_scene_builder_point_light():
    """create_point_light multiplies Translate(from) on the LEFT of the CTM (point.rs:121): under a scaling CTM the light sits at `from`,
    not at the CTM's image of it."""
    sb = scenes.SceneBuilder()
    idx = sb.light_point(I=(2, 2, 2), scale=(3, 1, 0.5), frm=(1, 2, 3), ctm=scenes.transform_scale(2, 2, 2))
    dl = sb.delta_lights[0]
    assert idx == 0 and dl.kind == capi.PT_DELTA_POINT and list(dl.spectrum) == [6.0, 2.0, 1.0]
    assert np.array_equal(mat(dl.light_to_world), ref.point_light_to_world(np.diag([2.0, 2, 2, 1]), (1, 2, 3)))
    assert np.array_equal(ref.from_record(dl).v, [1.0, 2.0, 3.0])
    assert np.allclose(ref.power(ref.from_record(dl)), np.array([6.0, 2.0, 1.0]) * 4 * np.pi)


def test_restatement_bands_and_near_share():
    """The restatement alone on the floor the GPU tests light: all three bands of the spot occur, the share of points within their bound of
    a cone cosine stays far below the 2 % cap, and falloff is continuous across the inner cosine and jumps at the outer one."""
    lt = ref.spot(np.eye(4), (0.3, -0.2, 2.5), (0.1, 0.2, 0.0), (30, 20, 10), 25, 8)
    g = np.linspace(-2, 2, 201)
    p = np.stack([*np.meshgrid(g, g), np.zeros((201, 201))], -1).reshape(-1, 3)
    s = ref.sample_li(lt, p, 16 * ref.EPS * 4)
    f = s["falloff"]
    assert (f == 1).mean() > 0.02 and (f == 0).mean() > 0.3 and ((f > 0) & (f < 1)).mean() > 0.05
    assert s["near"].mean() <= 0.0005
    inner = (f < 1) & (f > 0)
    assert s["li_rel"][inner & ~s["near"] & (f > 1e-3)].max() < 1e-2            # the bound stays a useful one across the band
    # power: I * 2 pi (1 - .5 (cf - ct))
    ct, cs = ref.cone_cosines(25, 8)
    assert np.allclose(ref.power(lt), np.array([30, 20, 10]) * 2 * np.pi * (1 - 0.5 * (cs - ct)))
    assert ref.radical_inverse(2, 6) == 0.375 and abs(ref.radical_inverse(3, 5) - (2 / 3 + 1 / 9)) < 1e-15 and ref.PROBES.shape == (128, 5)
