"""The .pbrt front end with PTH_FEATURE_MOTION_BLUR (ParsedScene(motion_blur=True)): what an animated Shape, ObjectInstance and Camera
become, what is still refused, and that without the bit the three refusals read as they did.  No device."""
import numpy as np
import pytest

import motion_pbrt
from helpers import pkg

capi = pkg.capi


def _mesh_objects(ps):
    return [ps.desc.meshes[i].object for i in range(ps.desc.n_meshes)]


def test_animated_shape_instance_and_camera_become_records():
    ps = capi.ParsedScene(text=motion_pbrt.TEXT, motion_blur=True)
    sd = motion_pbrt.builder_scene()
    d, mo = ps.desc, ps.motion
    assert mo is not None and list(mo.transform_times) == [2.0, 5.0]                     # TransformTimes 2 5 arrives
    # the animated Shape: one implicit object (its mesh built under the identity), one instance, one motion record -- and no light
    assert _mesh_objects(ps) == [0, 1, 2, 2, 0] and d.n_instances == 2 and mo.n_instances == 2
    assert [d.meshes[i].area_light >= 0 for i in range(d.n_meshes)] == [True, False, False, False, False]
    assert "Ignoring currently set area light when creating animated shape" in ps.warnings
    P = np.ctypeslib.as_array(d.P, (d.n_vertices, 3))
    assert np.array_equal(P[4:8], np.array([(-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0)], np.float32))
    assert d.instances[0].object == 0 and d.instances[0].before_triangle == 4 and d.instances[1].object == 1 and d.instances[1].before_triangle == 6
    # ... and everything equals what SceneBuilder assembles, bit for bit
    bd, bm = sd.desc, sd.motion
    assert list(bm.transform_times) == [2.0, 5.0] and bm.n_instances == 2 and bm.camera_animated == 1 and mo.camera_animated == 1
    assert list(mo.camera_to_world_end) == list(bm.camera_to_world_end) and list(d.camera_to_world) == list(bd.camera_to_world)
    assert list(mo.camera_to_world_end) != list(d.camera_to_world)
    for k in range(2):
        a, b = mo.instances[k], bm.instances[k]
        assert a.instance == b.instance == k
        assert list(a.instance_to_world_end) == list(b.instance_to_world_end) and list(a.world_to_instance_end) == list(b.world_to_instance_end)
        assert list(d.instances[k].instance_to_world) == list(bd.instances[k].instance_to_world)
        assert list(d.instances[k].world_to_instance) == list(bd.instances[k].world_to_instance)
        assert d.instances[k].before_triangle == bd.instances[k].before_triangle and d.instances[k].object == bd.instances[k].object
    assert (d.shutter_open, d.shutter_close) == (2.5, 4.5)


def test_equal_slots_make_no_record():
    text = motion_pbrt.TEXT.replace("  Translate 0.25 -0.5 0\n", "  Translate 0 0 0\n")
    ps = capi.ParsedScene(text=text, motion_blur=True)
    assert ps.motion.n_instances == 1 and ps.desc.n_instances == 2          # the ObjectInstance's two slots are equal: a static instance
    static = "\n".join(ln for ln in motion_pbrt.TEXT.split("\n") if "ActiveTransform" not in ln and "LookAt 0.5" not in ln)
    assert capi.ParsedScene(text=static, motion_blur=True).motion is None


def test_still_refused_by_name():
    inside = motion_pbrt.TEXT.replace('ObjectBegin "thing"\n', 'ObjectBegin "thing"\n  ActiveTransform EndTime\n  Translate 0 1 0\n  ActiveTransform All\n')
    with pytest.raises(capi.PtError, match="animated Shape inside ObjectBegin .*two levels"):
        capi.ParsedScene(text=inside, motion_blur=True)
    proj = motion_pbrt.TEXT.replace("  Translate 0.25 -0.5 0\n", "  ConcatTransform [ 1 0 0 0  0 1 0 0  0 0 1 0.5  0 0 0 1 ]\n")
    with pytest.raises(capi.PtError, match="projective"):
        capi.ParsedScene(text=proj, motion_blur=True)


HEAD = 'LookAt 0 0 -5  0 0 0  0 1 0\n%sCamera "perspective"\nFilm "image" "integer xresolution" 8 "integer yresolution" 8\nSampler "sobol"\nWorldBegin\n'
TRI = 'Shape "trianglemesh" "integer indices" [ 0 1 2 ] "point P" [ 0 0 0  1 0 0  0 1 0 ]\n'
ANIM = "ActiveTransform EndTime\nTranslate 0 1 0\nActiveTransform All\n"
ONE_KIND = {
    "camera": (HEAD % ANIM + TRI + "WorldEnd\n", "animated camera transforms are outside the accelerated path"),
    "shape": (HEAD % "" + TRI + "AttributeBegin\n" + ANIM + TRI + "AttributeEnd\nWorldEnd\n", "animated transforms are outside the accelerated path"),
    "instance": (HEAD % "" + TRI + 'ObjectBegin "o"\n' + TRI + "ObjectEnd\nAttributeBegin\n" + ANIM + 'ObjectInstance "o"\nAttributeEnd\nWorldEnd\n',
                 "animated instance transforms are outside the accelerated path"),
}


@pytest.mark.parametrize("kind", list(ONE_KIND))
def test_without_the_bit_the_three_refusals_stand(kind):
    """Each kind alone in a scene: refused word for word through the plain entry point and through the features entry point without the
    bit, taken with it."""
    text, message = ONE_KIND[kind]
    for kw in ({}, {"mix_materials": True}):
        with pytest.raises(capi.PtError) as e:
            capi.ParsedScene(text=text, **kw)
        assert str(e.value) == "PT_ERR_UNSUPPORTED: " + message
    ps = capi.ParsedScene(text=text, motion_blur=True)
    assert ps.motion is not None and list(ps.motion.transform_times) == [0.0, 1.0]          # render_options.rs:65-66
    assert (ps.motion.camera_animated, ps.motion.n_instances) == ((1, 0) if kind == "camera" else (0, 1))
