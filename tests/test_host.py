"""Host-side logic and the C-ABI boundary, without a GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from helpers import pkg, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ABI = 9      # include/pbrtgpu.h PT_ABI_VERSION; bump together with the header, capi.py and INTEGRATION.md (generated)


def pkg_symbols():
    return pkg.capi.SYMBOLS


def test_library_exports_every_declared_symbol():
    """libpbrtgpu.so loads (no device needed) and exports exactly what include/pbrtgpu.h declares."""
    header = open(os.path.join(ROOT, "include", "pbrtgpu.h")).read()
    declared = set(re.findall(r"\b(pt_[a-z0-9_]+)\s*\(", header))
    declared -= {"pt_status"}
    lib = pkg.capi.load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), "missing export: " + name
    assert declared == set(pkg.capi.SYMBOLS), declared ^ set(pkg.capi.SYMBOLS)
    assert lib.pt_abi_version() == PT_ABI


def test_struct_layouts_match_header():
    """ctypes mirrors of the ABI structs have the C sizes (checked against a tiny C program)."""
    import subprocess, tempfile
    src = '#include <stdio.h>\n#include "pbrtgpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pt_scene_desc), sizeof(pt_material), sizeof(pt_area_light), sizeof(pt_mesh), sizeof(pt_tile), sizeof(pt_hit), sizeof(pt_counters), sizeof(pt_scene_info));return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")])
        sizes = [int(x) for x in subprocess.check_output([os.path.join(td, "s")]).split()]
    c = pkg.capi
    mine = [C.sizeof(t) for t in (c.pt_scene_desc, c.pt_material, c.pt_area_light, c.pt_mesh, c.pt_tile, c.pt_hit, c.pt_counters, c.pt_scene_info)]
    assert mine == sizes
    assert c.HIT_DTYPE.itemsize == C.sizeof(c.pt_hit)


def test_no_device_fails_loudly():
    """There is no CPU fallback: without a HIP device the context cannot be created."""
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.PtError) as e:
        pkg.Context(0)
    assert e.value.status == 2          # PT_ERR_NO_DEVICE


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(OSError):
        pkg.capi.load_library(str(tmp_path / "libpbrtgpu.so"))


@pytest.mark.parametrize("method", ["sah", "middle", "equal", "hlbvh"])
def test_host_bvh_matches_reference_topology(oracle, method):
    """The product's BVH builder (pt_bvh.cpp, in-place partition, threaded) yields the oracle's
    (= reference's recursive_build) leaf order and node counts."""
    for sd_fn in (lambda: scenes.cornell_box(res=16, spp=1), lambda: scenes.rt1m(30000, res=16, spp=1)):
        b = sd_fn
        sd = b()
        sd.desc.split_method = {"sah": 0, "hlbvh": 1, "middle": 2, "equal": 3}[method]
        order, n_nodes, n_leaves, max_stack = pkg.capi.bvh_leaf_order(sd)
        sc = oracle.scene(sd)
        assert np.array_equal(order, sc.ordered_prims())
        assert (n_nodes, n_leaves) == (sc.info.n_nodes, sc.info.n_leaves)
        assert max_stack >= 1
        sc.close()


def test_hlbvh_morton_fallback_and_duplicates(oracle):
    """hlbvh.rs:102-157, :183-192: more than maxnodeprims primitives in one Morton cell fall back to
    centroid-median splits (start axis z, then y, x); coincident triangles stay in input order."""
    b = scenes.SceneBuilder()
    b.look_at((0, 0, -5), (0, 0, 0), (0, 1, 0)); b.camera_perspective(fov=40.0)
    b.film(xresolution=16, yresolution=16); b.pixel_filter_box(); b.sampler_sobol(1); b.integrator_path(maxdepth=1)
    b.material_matte((0.5, 0.5, 0.5))
    rng = np.random.default_rng(2)
    # a tight cluster (all in one 1/1024 cell of the scene box), 40 exact duplicates, and a sparse shell
    for k in range(60):
        c = np.array([0.3, 0.2, 0.1]) + rng.random(3) * 1e-5
        b.shape_trianglemesh([tuple(c), tuple(c + [1e-6, 0, 0]), tuple(c + [0, 1e-6, 0])], [0, 1, 2])
    for k in range(40):
        b.shape_trianglemesh([(-0.5, -0.5, 0.5), (-0.4, -0.5, 0.5), (-0.5, -0.4, 0.5)], [0, 1, 2])
    for k in range(200):
        c = rng.random(3) * 4 - 2
        b.shape_trianglemesh([tuple(c), tuple(c + [0.05, 0, 0]), tuple(c + [0, 0.05, 0.02])], [0, 1, 2])
    sd = b.build()
    sd.desc.split_method = 1
    for leaf in (1, 4, 16):
        sd.desc.max_node_prims = leaf
        order, n_nodes, n_leaves, max_stack = pkg.capi.bvh_leaf_order(sd)
        sc = oracle.scene(sd)
        assert np.array_equal(order, sc.ordered_prims())
        assert (n_nodes, n_leaves) == (sc.info.n_nodes, sc.info.n_leaves)
        assert sorted(order) == list(range(300))
        sc.close()


def test_scene_builder_mirrors_reference_rules():
    """pbrt_shape-side rules restated in scenes.py: degenerate triangles dropped (triangle.rs:726),
    uv auto-fill only for 'fillable' index patterns (triangle.rs:733-821), one light per emissive triangle."""
    b = scenes.SceneBuilder()
    b.shape_trianglemesh([(0, 0, 0), (1, 0, 0), (0, 1, 0), (5, 5, 5), (5, 5, 5), (5, 5, 5)], [0, 1, 2, 3, 4, 5])   # second triangle degenerate
    b.area_light_source_diffuse(L=(2, 2, 2), scale=(0.5, 1, 1))
    b.shape_trianglemesh([(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], [0, 1, 2, 0, 2, 3])
    sd = b.build()
    assert sd.desc.n_triangles == 3
    assert sd.desc.n_meshes == 2
    m0, m1 = sd.desc.meshes[0], sd.desc.meshes[1]
    assert m0.flags & pkg.capi.PT_MESH_HAS_UV          # one triangle: fillable
    assert not (m1.flags & pkg.capi.PT_MESH_HAS_UV)    # quad as 2 triangles sharing vertices in different slots
    assert m1.area_light == 0 and m0.area_light == -1
    assert list(sd.desc.area_lights[0].L) == [1.0, 2.0, 2.0]
    uv = sd.buffers["UV"]
    assert np.array_equal(uv[:3], np.array([[0, 0], [1, 0], [1, 1]], np.float32))
    # a vertex reused in a different corner slot makes the mesh non-fillable (the rule runs before the degenerate filter)
    assert not scenes._is_fillable_uv(np.array([[0, 1, 2], [3, 3, 3]]), 4)


def test_rt1m_generator_is_deterministic():
    a, b = scenes.rt1m(5000, res=16, spp=1), scenes.rt1m(5000, res=16, spp=1)
    assert np.array_equal(a.buffers["P"], b.buffers["P"])
    assert a.desc.n_triangles == 5000
    p = a.buffers["P"]
    assert p.min() >= -1.0 and p.max() <= 1.0


def test_all_tiles_cover_sample_bounds():
    class I:
        sample_bounds = [-1, -1, 1025, 1025]
    t = scenes.all_tiles(I())
    assert len(t) == 65 * 65                   # 4225 tiles
    area = sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in t)
    assert area == 1026 * 1026


def test_rust_ffi_block_matches_header(tmp_path):
    """INTEGRATION.md's Rust `#[repr(C)]` / `extern "C"` block is generated from include/pbrtgpu.h (tools/gen_rust_ffi.py): the document must
    be the generator's current output, and the sizes, alignments and field offsets the generator computed (and printed into the block)
    must be the C compiler's for every ABI struct -- an ABI change that forgets the document fails here."""
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as g
    h = g.Header()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    a, b = doc.index(g.BEGIN), doc.index(g.END) + len(g.END)
    assert doc[a:b] == g.generated_block(h), "INTEGRATION.md is stale: run tools/gen_rust_ffi.py --update"
    src = tmp_path / "layout.c"
    src.write_text(h.layout_c_program())
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    from_c = subprocess.check_output([exe], text=True).split("\n")
    assert [ln for ln in from_c if ln] == h.layout_lines()
    # every struct, every exported function and the ABI number are in the block
    names = {n for n, _ in h.structs}
    assert {"pt_scene_desc", "pt_material", "pt_counters", "pt_hit", "pt_scene_info", "pt_texture", "pt_sphere", "pt_instance", "pt_image"} <= names
    block = doc[a:b]
    for n in names:
        assert "pub struct %s " % n in block
    assert {f[0] for f in h.functions} == set(pkg_symbols())
    assert "(ABI %d)" % PT_ABI in block and "pub struct pt_material {      // 164 bytes" in block


def test_kernel_register_budgets():
    """The occupancy steps the measured numbers rest on, read from the built library's own code-object metadata (tools/kernel_resources.py):
    a change elsewhere in pt_kernels.hip that costs a hot kernel a wave per SIMD or makes it spill shows here, on the CPU, instead of as a
    few per cent in the next bench run.  (Waves per SIMD by allocated registers: <= 128 -> 4, <= 168 -> 3, <= 256 -> 2.)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(pkg.capi.LIB_PATH)
    budgets = {                      # kernel: (registers at most, spilled registers at most, LDS bytes at most)
        "k_trace": (128, 0, 163840),             # four waves per SIMD; ONE 1024-thread block per CU (PT_TRACE_WIDE): its stacks + the shared copy of the tree's top five levels
        "k_trace_inst": (168, 48, 32800),        # scenes with object instances: three waves per SIMD (rays enter instances; the blocking form took 212)
        "k_trace_far": (128, 0, 163840),         # the same with nodes fetched by lane pairs (scenes whose rays miss the caches)
        "k_trace_seq": (128, 0, 40960),
        "k_trace_sph_dist": (128, 0, 163840),    # scenes with spheres (config 4's class): the same occupancy step
        "k_shade": (256, 0, 40960),              # two waves per SIMD, nothing in scratch
        "k_shade_matte_sorted": (256, 0, 40960),
        "k_shade_general": (256, 0, 40960),
        "k_shade_general_inst_plain": (256, 0, 40960),   # scenes with instances and neither textures nor spheres: the lobe-list kernel + the instance-space reconstruction, nothing spilled
        "k_shade_all": (256, 0, 40960),              # the locally sorted queue's one kernel (the default for constant lobe-list materials): k_shade_general's figures
        "k_shade_general_res": (256, 0, 40960),      # the textured segment's shading half: nothing spilled
        "k_tex_resolve": (256, 32, 40960),           # ... and its texture half, the texture code inlined, the interpreter's node values in LDS: 28 registers spilled, 116 B of scratch
        "k_tex_resolve_sph": (256, 56, 40960),
        # The sphere-capable whole-vertex kernels (killeroo-class scenes) DO spill -- Sphere::sample_from and the EFloat quadratic are calls in the
        # middle of next-event estimation.  Round 4 built the spill-free form (the vertex in two kernels, since retired: tools/patches/README.md) and
        # measured it 6 % SLOWER on the killeroo-class line, so these are the only form; the budgets hold them where they are.
        "k_shade_matte_sorted_sph": (256, 90, 40960),
        "k_shade_general_sph": (256, 64, 40960),
        "k_shade_all_sph": (256, 64, 40960),         # k_shade_general_sph over the locally sorted queue
        "k_shade_general_res_sph": (256, 104, 40960),
        "k_shade_general_inst": (256, 150, 40960),   # scenes with object instances: one kernel shades everything (a breadth feature)
        # the recursive integrators: the instantiation BASELINE's scenes run (no spheres, instances or textured materials) spills nothing;
        # the everything-compiled-in one keeps its per-hit lobe list in scratch
        "k_rec_enter_plain": (256, 0, 64), "k_rec_next_plain": (256, 0, 8192),
        "k_rec_enter": (256, 180, 64), "k_rec_next": (256, 110, 8192),
        "k_nee_resolve": (64, 0, 0),
        "k_gen": (128, 0, 0),
        "k_grid_mark": (128, 0, 0),
    }
    for name, (vgpr, spill, lds) in budgets.items():
        k = ks[name]
        assert k[".vgpr_count"] <= vgpr, (name, "registers", k[".vgpr_count"])
        assert k.get(".vgpr_spill_count", 0) <= spill, (name, "spilled registers", k.get(".vgpr_spill_count", 0))
        assert k[".group_segment_fixed_size"] <= lds, (name, "LDS", k[".group_segment_fixed_size"])
    assert ks["k_tex_resolve"][".private_segment_fixed_size"] <= 1024       # as calls its frames took 2.4 KB per lane: more scratch in flight than L2 holds
