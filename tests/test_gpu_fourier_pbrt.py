"""A .pbrt scene that names the rough-gold table, end to end: parsed with the fourier feature, uploaded, rendered by the build that knows
FourierBSDF -- and `pbrt_gpu -i` on the same file -- bit for bit what the same scene assembled with SceneBuilder renders."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fourier_cases as FC
from helpers import bits, pkg, scenes

pytestmark = pytest.mark.gpu
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TEXT = """LookAt 0 -4 3  0 0 0  0 0 1
Camera "perspective" "float fov" [50]
Film "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" "o.pfm"
PixelFilter "box"
Sampler "sobol" "integer pixelsamples" [4]
Integrator "path" "integer maxdepth" [3]
WorldBegin
LightSource "distant" "rgb L" [3 3 3] "point from" [0.2 3 2.5] "point to" [0 0 0]
Material "fourier" "string bsdffile" "bsdfs/gold.bsdf"
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -2 0 2 -2 0 2 2 0 -2 2 0] "float uv" [0 0 1 0 1 1 0 1]
MakeNamedMaterial "g" "string type" "fourier" "string bsdffile" "bsdfs/gold.bsdf"
NamedMaterial "g"
Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-1 -1 0.5 1 -1 0.5 0 1 1.2]
WorldEnd
"""


def builder_scene(path):
    sb = scenes.SceneBuilder()
    sb.look_at((0, -4, 3), (0, 0, 0), (0, 0, 1))
    sb.camera_perspective(fov=50.0)
    sb.film(xresolution=16, yresolution=16)
    sb.pixel_filter_box()
    sb.sampler_sobol(pixelsamples=4)
    sb.integrator_path(maxdepth=3)
    sb.light_distant(L=(3, 3, 3), frm=(0.2, 3, 2.5), to=(0, 0, 0))
    sb.material_fourier(bsdffile=path)
    sb.shape_trianglemesh([-2, -2, 0, 2, -2, 0, 2, 2, 0, -2, 2, 0], [0, 1, 2, 0, 2, 3], uv=[(0, 0), (1, 0), (1, 1), (0, 1)])
    sb.shape_trianglemesh([-1, -1, 0.5, 1, -1, 0.5, 0, 1, 1.2], [0, 1, 2])
    return sb.build()


def test_pbrt_text_and_the_command_line_render_what_the_builder_scene_renders(gpu_ctx, tmp_path):
    os.makedirs(tmp_path / "bsdfs")
    shutil.copy(FC.ROUGHGOLD, tmp_path / "bsdfs" / "gold.bsdf")
    (tmp_path / "s.pbrt").write_text(TEXT)
    ctx = gpu_ctx

    def render(scene):
        ctx.upload(scene)
        assert ctx.kernel_set() == capi.PT_KERNELS_FOURIER
        ctx.film_clear(); ctx.render()
        return ctx.film_rgb()
    want = render(builder_scene(str(tmp_path / "bsdfs" / "gold.bsdf")))
    ps = capi.ParsedScene(filename=str(tmp_path / "s.pbrt"), fourier_materials=True, delta_lights=True)
    assert len(ps.fourier_tables) == 1 and len(ps.fourier) == 1          # one file named twice: one table; the same material twice: one record
    parsed = render(ps)
    assert np.array_equal(bits(parsed), bits(want)) and (want > 0).any(-1).mean() > 0.3
    info = capi.pt_scene_info()
    assert ctx.lib.pt_scene_info_get(ctx.h, info) == 0 and info.fourier_capped == 0
    exe = os.path.join(ROOT, "pbrt-r3_amd", "csrc", "pbrt_gpu")
    out = tmp_path / "cli.pfm"
    r = subprocess.run([exe, "-i", str(tmp_path / "s.pbrt"), "--outfile", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer(out.read_bytes().split(b"\n", 3)[3], "<f4").reshape(16, 16, 3)[::-1]
    assert np.array_equal(bits(got), bits(want))
