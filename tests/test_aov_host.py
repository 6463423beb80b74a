"""Integrator "aov" without a GPU: the front end's names and defaults, the side call's range check, the calibration of the truth
(tests/aov_ref.py in float32 held to itself in float64 on every case of test_gpu_aov.py) and the kernels' code-object metadata.

The calibration's figures are recorded in profiles/aov_truth.txt (rewritten when AOV_TRUTH_WRITE=1 is set, or when the file is missing);
test_gpu_aov.py reads the float32 medians from it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import aov_cases as AC
import aov_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENE = '''LookAt 0 0 1 0 0 0 0 1 0
Camera "perspective" "float fov" 40
Film "image" "integer xresolution" 8 "integer yresolution" 8
Sampler "sobol" "integer pixelsamples" 4
Integrator "aov" %s
WorldBegin
Shape "trianglemesh" "point P" [-1 -1 0 1 -1 0 0 1 0] "integer indices" [0 1 2]
WorldEnd
'''
# get_aov_target (integrators/aov.rs:27-56), name -> position in AOVTarget
NAMES = {"distance": 0, "depth": 1, "n": 2, "ng": 2, "ns": 3, "shading.n": 3, "uv": 4, "rdxc": 5, "rdyc": 6, "drodx": 7, "drddx": 8, "dpdx": 9,
         "dpdy": 10, "dpdu": 11, "dpdv": 12, "dstdx": 13, "duvdx": 13, "dstdy": 14, "dpdus": 15, "shading.dpdu": 15, "dpdvs": 16, "shading.dpdv": 16}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_target_names(pkg, name):
    s = pkg.capi.ParsedScene(text=SCENE % ('"string target" "%s" "float scale" 0.5' % name))
    assert s.desc.integrator == pkg.capi.PT_INTEGRATOR_AOV == 4
    assert s.aov == (NAMES[name], 0.5)
    assert pkg.capi.AOV_TARGETS[name] == NAMES[name]


def test_names_are_the_references(pkg):
    assert pkg.capi.AOV_TARGETS == NAMES
    assert [getattr(pkg.capi, "PT_AOV_" + t.upper()) for t in R.TARGETS] == list(range(17))


def test_defaults(pkg):
    s = pkg.capi.ParsedScene(text=SCENE % "")
    assert s.desc.integrator == 4 and s.aov == (pkg.capi.PT_AOV_UV, 1.0)
    other = pkg.capi.ParsedScene(text=SCENE.replace('Integrator "aov" %s', 'Integrator "path"'))
    assert other.desc.integrator == 0 and other.aov == (pkg.capi.PT_AOV_UV, 1.0)


@pytest.mark.parametrize("name", ["duvdy", "normal", "UV", ""])
def test_unknown_target(pkg, name):
    with pytest.raises(pkg.capi.PtError) as e:
        pkg.capi.ParsedScene(text=SCENE % ('"string target" "%s"' % name))
    assert 'AOV target "%s" unknown' % name in str(e.value)
    with pytest.raises(pkg.capi.PtError) as other:           # the status of the front end's other Integrator errors
        pkg.capi.ParsedScene(text=SCENE.replace('Integrator "aov" %s', 'Integrator "bdpt"'))
    assert e.value.args[0].split(":")[0] == other.value.args[0].split(":")[0] == "PT_ERR_UNSUPPORTED"


def test_builder_and_text_agree(pkg):
    for name, scale in (("uv", 1.0), ("shading.dpdu", 0.25), ("ng", 2.0)):
        b = pkg.scenes.SceneBuilder()
        b.integrator_aov(name, scale)
        b.shape_trianglemesh([(-1, -1, 0), (1, -1, 0), (0, 1, 0)], [0, 1, 2])
        sd = b.build()
        s = pkg.capi.ParsedScene(text=SCENE % ('"string target" "%s" "float scale" %r' % (name, scale)))
        assert sd.aov == s.aov and sd.desc.integrator == s.desc.integrator == 4
    b = pkg.scenes.SceneBuilder()
    assert b.build().aov == (pkg.capi.PT_AOV_UV, 1.0)
    with pytest.raises(ValueError):
        b.integrator_aov("duvdy")


def test_set_aov_symbol(pkg):
    """The side call is exported and refuses a missing context.  Its range check (17 and -1 refused, 16 accepted) needs a context, which
    needs a device: test_gpu_aov.py::test_set_aov_range_and_no_leak."""
    lib = pkg.capi.load_library()
    assert hasattr(lib, "pt_scene_set_aov") and "pt_scene_set_aov" in pkg.capi.SYMBOLS and "pth_scene_get_aov" in pkg.capi.HOST_SYMBOLS
    assert lib.pt_scene_set_aov(None, C.c_int32(17), C.c_float(1.0)) == 1       # PT_ERR_INVALID_ARGUMENT
    assert lib.pt_scene_set_aov(None, C.c_int32(-1), C.c_float(1.0)) == 1


def _calibrate(name):
    sd = AC.CASES[name]()
    cam = R.Camera(sd)
    rng = np.random.default_rng(3)
    px, _ = AC.pixel_samples(sd, cam.spp)
    pf = (px + rng.random(px.shape)).astype(np.float32)
    ul = rng.random(px.shape).astype(np.float32)
    o, d = R.main_ray(cam, pf, ul)
    hits, und = AC.truth_hits(name, sd, o, d)
    t64 = R.evaluate(sd, o, d, pf, ul, hits, np.float64)
    t32 = R.evaluate(sd, o, d, pf, ul, hits, np.float32, hits32=True)
    lines = []
    AC.check(name, t32["value"], t64, und | t64["und"], report=lines)
    return lines, t64


_lines = {}


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_calibration(name):
    """The float32 run of the restatement against its float64 run: err <= bound everywhere outside the left-out set, left-out share <= 3 %."""
    lines, t64 = _calibrate(name)
    _lines[name] = lines
    assert t64["hit"].mean() > 0.25 and (name != "reports" or (~t64["hit"]).mean() > 0.25)
    for k in ("depth", "distance"):             # the geometry keeps most of these inside (0, 1), where v2c does not clamp
        v = t64["value"][k][t64["hit"]]
        assert (v < 1.0).mean() >= 0.8 and v.min() > 0.0, (k, (v < 1.0).mean())


def test_profile_recorded():
    """profiles/aov_truth.txt holds this calibration (the medians the device is compared with)."""
    for name in sorted(AC.CASES):
        if name not in _lines:
            _lines[name] = _calibrate(name)[0]
    text = "# tests/test_aov_host.py: float32 run of tests/aov_ref.py against its float64 run, err / bound per case and target\n" + \
           "".join(l + "\n" for name in sorted(_lines) for l in _lines[name])
    if os.environ.get("AOV_TRUTH_WRITE") == "1" or not os.path.exists(AC.PROFILE):
        with open(AC.PROFILE, "w") as f:
            f.write(text)
    rec = AC.read_medians()
    for name in _lines:
        for l in _lines[name]:
            f = l.split()
            assert (f[0], f[1]) in rec, (f[0], f[1], "missing from profiles/aov_truth.txt")
            assert abs(rec[(f[0], f[1])] - float(f[5])) <= 1e-3 * max(float(f[5]), 1e-9), (l, rec[(f[0], f[1])])


def test_kernel_resources(pkg):
    """k_aov_plain (triangles only, no textures) spills nothing and has no scratch; k_aov's figures are its budget: a change may lower
    them, never raise them.  Its scratch is the frames of the calls it shares with the other everything-compiled-in kernels (the sphere
    test, the texture interpreter)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(pkg.capi.LIB_PATH)
    plain, full = ks["k_aov_plain"], ks["k_aov"]
    assert plain.get(".vgpr_spill_count", 0) == 0 and plain[".private_segment_fixed_size"] == 0 and plain[".vgpr_count"] <= 141
    assert full[".vgpr_count"] <= 223 and full.get(".vgpr_spill_count", 0) == 0 and full[".private_segment_fixed_size"] <= 416
    assert plain[".group_segment_fixed_size"] == 0 and full[".group_segment_fixed_size"] == 0
