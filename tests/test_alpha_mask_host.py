"""Alpha masks in the .pbrt front end and the scene builder (no device needed): "alpha" / "shadowalpha" on trianglemesh and plymesh, inside
ObjectBegin too, "texture" over "float" (shapes/triangle.rs:654-694), names that are no float texture, constants, spheres ignoring both
(shapes/sphere.rs:401-420), and the budgets of the alpha traversal kernels."""
import os
import sys

import pytest

from helpers import pkg, scenes

capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = 'Sampler "sobol"\nWorldBegin\n'
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 0 0 1 0 0 1 1 0 0 1 0]'
CHECKER = 'Texture "ck" "float" "checkerboard" "float uscale" [4] "float vscale" [4]\n'


def parse(body, work_dir=None):
    return capi.ParsedScene(text=HEAD + body + "WorldEnd\n", work_dir=work_dir)


def masks(ps):
    return [(m.mesh, m.alpha_kind, m.alpha_value, m.alpha_texture, m.shadow_kind, m.shadow_value, m.shadow_texture) for m in ps.alpha_masks]


N, C_, T = capi.PT_ALPHA_NONE, capi.PT_ALPHA_CONSTANT, capi.PT_ALPHA_TEXTURE


def test_trianglemesh_constants():
    ps = parse(TRI + ' "float alpha" [0]\n' + TRI + '\n' + TRI + ' "float shadowalpha" [-1] "float alpha" [0.5]\n')
    assert masks(ps) == [(0, C_, 0.0, -1, N, 0.0, -1), (2, C_, 0.5, -1, C_, -1.0, -1)]
    assert ps.desc.n_meshes == 3 and ps.desc.n_triangles == 6          # masked triangles stay in the scene (world bound)


def test_texture_before_float_and_unknown_names():
    ps = parse(CHECKER + 'Texture "sp" "spectrum" "checkerboard"\n' +
               TRI + ' "texture alpha" "ck" "float alpha" [0]\n' +          # the texture wins
               TRI + ' "texture alpha" "nope" "float alpha" [0]\n' +        # unknown name: no mask at all, the float is not read
               TRI + ' "texture shadowalpha" "sp"\n' +                      # a spectrum texture is no float texture: no mask
               TRI + ' "float alpha" [0] "texture shadowalpha" "ck"\n')
    ck = 0
    assert ps.desc.textures[ck].type == capi.PT_TEX_CHECKERBOARD_2D
    assert masks(ps) == [(0, T, 0.0, ck, N, 0.0, -1), (3, C_, 0.0, -1, T, 0.0, ck)]


def test_texture_that_folds_to_a_constant():
    ps = parse('Texture "z" "float" "constant" "float value" [0]\nTexture "h" "float" "scale" "float tex1" [0.5] "float tex2" [3]\n' +
               TRI + ' "texture alpha" "z"\n' + TRI + ' "texture shadowalpha" "h"\n')
    assert masks(ps) == [(0, C_, 0.0, -1, N, 0.0, -1), (1, N, 0.0, -1, C_, 1.5, -1)]


def test_plymesh_and_object_instances(tmp_path):
    ply = tmp_path / "q.ply"
    ply.write_text("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                   "element face 2\nproperty list uchar int vertex_indices\nend_header\n"
                   "0 0 0\n1 0 0\n1 1 0\n0 1 0\n3 0 1 2\n3 0 2 3\n")
    ps = parse(CHECKER + 'Shape "plymesh" "string filename" "q.ply" "texture alpha" "ck" "float shadowalpha" [0]\n' +
               'ObjectBegin "o"\n' + TRI + ' "float alpha" [0]\n' + TRI + ' "texture shadowalpha" "ck"\nObjectEnd\n'
               'ObjectInstance "o"\n', work_dir=str(tmp_path))
    assert masks(ps) == [(0, T, 0.0, 0, C_, 0.0, -1), (1, C_, 0.0, -1, N, 0.0, -1), (2, N, 0.0, -1, T, 0.0, 0)]
    assert ps.desc.meshes[1].object == 1 and ps.desc.meshes[2].object == 1


def test_spheres_accept_and_ignore_the_parameters():
    ps = parse(CHECKER + 'Shape "sphere" "float alpha" [0] "texture shadowalpha" "ck"\n' + TRI + '\n')
    assert ps.desc.n_spheres == 1 and masks(ps) == []
    sb = scenes.SceneBuilder()
    sb.shape_sphere(alpha=0.0, shadowalpha=0.0)
    assert sb.build().alpha_masks == []


def test_builder_matches_the_parser():
    text = (CHECKER + TRI + ' "texture alpha" "ck"\n' + TRI + '\n' + TRI + ' "float alpha" [0] "float shadowalpha" [2]\n' +
            TRI + ' "texture shadowalpha" "ck"\n')
    ps = parse(text)
    sb = scenes.SceneBuilder()
    ck = sb.texture_checkerboard(uscale=4.0, vscale=4.0)
    P, idx = [0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0], [0, 1, 2, 0, 2, 3]
    sb.shape_trianglemesh(P, idx, alpha=ck)
    sb.shape_trianglemesh(P, idx)
    sb.shape_trianglemesh(P, idx, alpha=0.0, shadowalpha=2.0)
    sb.shape_trianglemesh(P, idx, shadowalpha=ck)
    sd = sb.build()
    assert [(m.mesh, m.alpha_kind, m.alpha_value, m.alpha_texture, m.shadow_kind, m.shadow_value, m.shadow_texture) for m in sd.alpha_masks] == masks(ps)
    assert ps.desc.textures[0].type == sd.desc.textures[0].type and ps.desc.textures[0].su == sd.desc.textures[0].su


def test_other_refusals_stay():
    with pytest.raises(capi.PtError, match="animated"):
        parse('ActiveTransform EndTime\nTranslate 1 0 0\nActiveTransform All\n' + TRI + ' "float alpha" [0]\n')


def test_abi_struct_layout():
    import ctypes as C
    assert C.sizeof(capi.pt_alpha_mask) == 48


def test_alpha_kernel_budgets():
    """Registers / spills / LDS of the alpha traversal kernels, read from the library (tools/kernel_resources.py).  k_trace_alpha is
    k_trace_inst's per-lane form plus a call of the out-of-line mask test: the call's saved registers spill.  The budgets are what the
    kernels take now: a change may lower them, never raise them."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(capi.LIB_PATH)
    budgets = {"k_trace_alpha": (168, 55, 2224), "k_trace_batch_alpha": (248, 0, 2352)}
    for name, (vgpr, spill, scratch) in budgets.items():
        k = ks[name]
        assert k[".vgpr_count"] <= vgpr, (name, "registers", k[".vgpr_count"])
        assert k.get(".vgpr_spill_count", 0) <= spill, (name, "spilled registers", k.get(".vgpr_spill_count", 0))
        assert k[".private_segment_fixed_size"] <= scratch, (name, "scratch")
        assert k[".group_segment_fixed_size"] <= 32800, (name, "LDS")
