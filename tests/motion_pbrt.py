"""A 20-line .pbrt scene that moves -- TransformTimes, ActiveTransform, an animated Shape, an animated ObjectInstance, an animated
camera -- and the same scene assembled with SceneBuilder (test_motion_frontend_host.py, test_gpu_motion_pbrt.py)."""
from helpers import scenes

TEXT = """
ActiveTransform StartTime
LookAt 0 0 -6.5  0 0 0  0 1 0
ActiveTransform EndTime
LookAt 0.5 0.25 -6  0 0 0  0 1 0
ActiveTransform All
Camera "perspective" "float fov" 40 "float shutteropen" 2.5 "float shutterclose" 4.5
TransformTimes 2 5
Film "image" "integer xresolution" 16 "integer yresolution" 16
PixelFilter "box"
Sampler "sobol" "integer pixelsamples" 4
Integrator "path" "integer maxdepth" 2
WorldBegin
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 30 30 30 ]
  Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ 1 3 -1  1 3 1  -1 3 1  -1 3 -1 ]
AttributeEnd
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 5 5 5 ]
  Translate -1 -0.5 0
  ActiveTransform EndTime
  Translate 0.5 0.75 0.25
  Scale 1 0.5 1.5
  ActiveTransform All
  Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ -0.5 -0.5 0  0.5 -0.5 0  0.5 0.5 0  -0.5 0.5 0 ]
AttributeEnd
ObjectBegin "thing"
  Shape "trianglemesh" "integer indices" [ 0 1 2 ] "point P" [ -0.5 0 0  0.5 0 0.125  0 0.75 0 ]
  Shape "trianglemesh" "integer indices" [ 0 1 2 ] "point P" [ -0.5 0 0.5  0.5 0 0.5  0 -0.75 0.25 ]
ObjectEnd
AttributeBegin
  Translate 1 0 0.5
  ActiveTransform EndTime
  Translate 0.25 -0.5 0
  ActiveTransform All
  ObjectInstance "thing"
AttributeEnd
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ 2.5 -2 -2  -2.5 -2 -2  -2.5 -2 2.5  2.5 -2 2.5 ]
WorldEnd
"""


def builder_scene():
    T, S, mul = scenes.transform_translate, scenes.transform_scale, scenes.transform_mul
    b = scenes.SceneBuilder()
    b.look_at((0, 0, -6.5), (0, 0, 0), (0, 1, 0))
    b.look_at_end((0.5, 0.25, -6), (0, 0, 0), (0, 1, 0))
    b.camera_perspective(fov=40.0, shutteropen=2.5, shutterclose=4.5)
    b.transform_times(2.0, 5.0)
    b.film(xresolution=16, yresolution=16)
    b.pixel_filter_box()
    b.sampler_sobol(4)
    b.integrator_path(maxdepth=2)
    b.area_light_source_diffuse(L=(30, 30, 30))
    b.shape_trianglemesh([(1, 3, -1), (1, 3, 1), (-1, 3, 1), (-1, 3, -1)], [0, 1, 2, 0, 2, 3])
    b.area_light_source_diffuse(L=(5, 5, 5))
    start = T(-1, -0.5, 0)
    b.animated_shape_begin(start, mul(mul(start, T(0.5, 0.75, 0.25)), S(1, 0.5, 1.5)))
    b.shape_trianglemesh([(-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0)], [0, 1, 2, 0, 2, 3])
    b.animated_shape_end()
    b.no_area_light()
    b.object_begin("thing")
    b.shape_trianglemesh([(-0.5, 0, 0), (0.5, 0, 0.125), (0, 0.75, 0)], [0, 1, 2])
    b.shape_trianglemesh([(-0.5, 0, 0.5), (0.5, 0, 0.5), (0, -0.75, 0.25)], [0, 1, 2])
    b.object_end()
    s2 = T(1, 0, 0.5)
    b.object_instance("thing", s2, mul(s2, T(0.25, -0.5, 0)))
    b.shape_trianglemesh([(2.5, -2, -2), (-2.5, -2, -2), (-2.5, -2, 2.5), (2.5, -2, 2.5)], [0, 1, 2, 0, 2, 3])
    return b.build()
