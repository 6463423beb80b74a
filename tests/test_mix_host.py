"""Material "mix" without a device: the descriptor SceneBuilder.material_mix writes, the restatement tests/mix_ref.py held to the text of
materials/mix.rs and core/reflection/scaled.rs, and its float32 run calibrated against its float64 run on the inputs of the GPU hook test
(tests/test_gpu_mix.py).  Uploads (and so the upload's refusals) need a device: they are in the GPU file."""
import ctypes as C_

import numpy as np
import pytest

import bsdf_cases as C
import bsdf_ref as R
import mix_cases as MC
import mix_ref as M
from helpers import pkg, scenes

capi = pkg.capi
f32 = np.float32


# ---------------------------------------------------------------- the descriptor
def test_abi_constant_and_struct_size():
    assert capi.PT_MATERIAL_MIX == 9
    assert C_.sizeof(capi.pt_material) == 164          # a mix rides in fields the struct already has
    assert capi.PT_MIX_MAX_LEAVES >= 4 and capi.PT_MIX_MAX_LOBES >= 16


def test_builder_writes_children_and_amount():
    b = scenes.SceneBuilder()
    b.material_plastic(Kd=(0.3, 0.2, 0.1))
    p = b.cur_material
    b.material_matte(Kd=(0.6, 0.5, 0.4))
    m = b.cur_material
    b.material_mix(p, m, (0.3, 0.4, 0.5))
    x = b.cur_material
    assert p < x and m < x                             # children precede the mix
    mm = b.materials[x]
    assert mm.type == capi.PT_MATERIAL_MIX
    assert (mm.tex_kr, mm.tex_kt, mm.tex_kd) == (p + 1, m + 1, 0)
    assert [f32(v) for v in mm.kd] == [f32(0.3), f32(0.4), f32(0.5)]
    b.material_mix(x, p)                               # nesting: a child may be a mix; "amount" defaults to 0.5
    y = b.cur_material
    assert b.materials[y].tex_kr == x + 1 and list(b.materials[y].kd) == [0.5, 0.5, 0.5]
    t = b.texture_checkerboard(0.2, 0.9, uscale=4.0, vscale=4.0, aamode="none")
    b.material_mix(p, m, t)
    assert b.materials[b.cur_material].tex_kd == t.index + 1 and list(b.materials[b.cur_material].kd) == [0.5, 0.5, 0.5]
    with pytest.raises(ValueError):
        b.material_mix(p, len(b.materials))            # not defined yet: no forward references, so no cycles


# ---------------------------------------------------------------- the restatement itself
def _dirs(n, seed):
    rng = np.random.default_rng(seed)
    return C.sphere_dirs(rng, n), C.sphere_dirs(rng, n), rng.random((n, 2)).astype(np.float32)


@pytest.mark.parametrize("case,setting", [("plastic", "remap"), ("uber", "five"), ("glass", "smooth"), ("translucent", "four")])
def test_mix_with_a_lobeless_sibling_at_amount_one_is_the_child(case, setting):
    """mix(A, matte(Kd 0), 1): s1 = 1, the sibling adds nothing -- 1 * f is f, in value and (float32 run) bit for bit."""
    p = C.params(case, setting)
    wo, wi, u = _dirs(2000, 5)
    for dt in (np.float64, np.float32):
        a, x = R.BSDF(p, dt), M.BSDF(MC.mix(p, MC.BLACK, 1.0), dt)
        assert len(x.lobes) == len(a.lobes)
        for _, flags in C.FLAG_SETS:
            va, vx = a.eval(wo, wi, flags), x.eval(wo, wi, flags)
            assert np.array_equal(va.f, vx.f) and np.array_equal(va.pdf, vx.pdf)
            sa, sx = a.sample(wo, u, flags), x.sample(wo, u, flags)
            for k in ("f", "wi", "pdf", "type", "pick"):
                assert np.array_equal(sa[k], sx[k]), (case, setting, k)


def test_a_lobe_scaled_by_zero_still_counts():
    """mix(lambert A, lambert B, 1): B is scaled by s2 = 0 and stays in the list -- the pdf is averaged over two lobes, the component
    choice halves u.x, and f is A's alone."""
    a, bm = dict(type="matte", Kd=(0.6, 0.45, 0.3)), dict(type="matte", Kd=(0.2, 0.3, 0.9))
    x = M.BSDF(MC.mix(a, bm, 1.0), np.float64)
    assert len(x.lobes) == 2
    wo, wi, u = _dirs(500, 6)
    wi[:, 2] = np.abs(wi[:, 2]) * np.sign(wo[:, 2])             # the same hemisphere
    v, va = x.eval(wo, wi), R.BSDF(a, np.float64).eval(wo, wi)
    assert np.array_equal(v.f, va.f)                            # 1 * f_A + 0 * f_B
    assert np.allclose(v.pdf, va.pdf, rtol=1e-12) and (v.pdf > 0).all()          # (p_A + p_B) / 2 with p_B = p_A: two lobes were counted
    s = x.sample(wo, u)
    assert set(np.unique(s["pick"])) == {0, 1}                  # the zero-scaled lobe is chosen for u.x >= 1 / 2
    dec = ~s["und"]
    assert np.array_equal(s["pick"][dec], (u[dec, 0] >= 0.5).astype(int))


def test_nesting_multiplies_innermost_first_and_the_order_shows_in_float32():
    """f = s_outer * (s_inner * f): two roundings.  (s_outer * s_inner) * f is another float for suitable inputs; one is exhibited."""
    s_i, s_o, kd = f32(0.1), f32(0.7), f32(0.3)
    f = kd * f32(R.INV_PI)
    nested, folded = s_o * (s_i * f), (s_o * s_i) * f
    assert nested != folded, "choose other constants: the two orders agree for these"
    leaf = dict(type="matte", Kd=(float(kd),) * 3)
    tree = MC.mix(MC.mix(leaf, MC.BLACK, float(s_i)), MC.BLACK, float(s_o))
    wo, wi = np.array([[0.3, 0.2, 0.9]], np.float32), np.array([[-0.1, 0.4, 0.8]], np.float32)
    got = M.BSDF(tree, np.float32).eval(wo, wi).f[0, 0]
    assert f32(got) == nested and f32(got) != folded
    chains = M.BSDF(tree, np.float64).chains
    assert [float(c[0].v) for c in chains[0]] == [float(s_i), float(s_o)]          # innermost first


def test_amount_is_clamped_below_only_and_weights_child_one():
    s1, s2 = M._scales((1.5, -0.25, 0.3), np.float64)
    assert [float(s.v) for s in s1] == [1.5, 0.0, float(f32(0.3))]
    assert [float(s.v) for s in s2] == [0.0, 1.0, 1.0 - float(f32(0.3))]
    a, b = dict(type="matte", Kd=(1.0, 1.0, 1.0)), MC.BLACK
    wo, wi = np.array([[0.0, 0.0, 1.0]], np.float32), np.array([[0.0, 0.6, 0.8]], np.float32)
    assert M.BSDF(MC.mix(a, b, 0.25), np.float64).eval(wo, wi).f[0, 0] == 0.25 * R.INV_PI          # amount weights namedmaterial1


def test_a_child_without_bsdf_adds_no_lobes():
    glass0 = dict(type="glass", Kr=(0.0,) * 3, Kt=(0.0,) * 3)
    x = M.BSDF(MC.mix(glass0, C.params("plastic", "remap"), 0.5), np.float64)
    assert len(x.lobes) == 2 and x.has_bsdf


# ---------------------------------------------------------------- calibration: the float32 run against the float64 run
@pytest.mark.parametrize("name", list(MC.SETTINGS))
def test_float32_restatement_stays_within_bound_and_under_the_cap(name):
    """The inputs of the GPU hook test leave the reference's own arithmetic inside the cap of left-out evaluations."""
    for s in MC.calibration(name).values():
        print(s)
        assert s.left <= C.MAX_LEFT_OUT, (s.what, s.left)          # (within bound: check_eval / check_sample assert it)


# ---------------------------------------------------------------- the .pbrt front end (pth_parse_*_features, PTH_FEATURE_MIX_MATERIAL)
HEAD = """LookAt 0 -3 2.5  0 0 0.4  0 0 1
Camera "perspective" "float fov" [50]
Film "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" "o.pfm"
Sampler "sobol" "integer pixelsamples" [1]
Integrator "path" "integer maxdepth" [3]
WorldBegin
"""
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0] "float uv" [0 0 1 0 1 1 0 1]'
NAMED = """MakeNamedMaterial "a" "string type" "plastic" "rgb Kd" [0.3 0.2 0.1] "rgb Ks" [0.25 0.25 0.25] "float roughness" [0.1]
MakeNamedMaterial "b" "string type" "matte" "rgb Kd" [0.6 0.5 0.4]
"""


def parse(body, **kw):
    return capi.ParsedScene(text=HEAD + body + "\nWorldEnd\n", mix_materials=True, **kw)


def mats(ps):
    return [capi.pt_material.from_buffer_copy(ps.desc.materials[i]) for i in range(ps.desc.n_materials)]          # copies: they outlive the scene


def raw(m):
    return bytes(memoryview(m).cast("B")) if not isinstance(m, bytes) else m


def mix_of(ps):
    ms = mats(ps)
    mesh_mat = ps.desc.meshes[ps.desc.n_meshes - 1].material
    assert ms[mesh_mat].type == capi.PT_MATERIAL_MIX
    return ms, mesh_mat


def test_plain_entry_points_still_refuse_mix():
    with pytest.raises(capi.PtError) as e:
        capi.ParsedScene(text=HEAD + NAMED + 'Material "mix" "string namedmaterial1" "a" "string namedmaterial2" "b"\n' + QUAD + "\nWorldEnd\n")
    assert e.value.status == 4 and "mix" in str(e.value) and "translucent" in str(e.value)


@pytest.mark.parametrize("form", ["material", "named"])
def test_both_directive_forms_parse_to_the_builders_bytes(form):
    use = ('Material "mix" "string namedmaterial1" "a" "string namedmaterial2" "b" "rgb amount" [0.3 0.4 0.5]\n' if form == "material" else
           'MakeNamedMaterial "m" "string type" "mix" "string namedmaterial1" "a" "string namedmaterial2" "b" "rgb amount" [0.3 0.4 0.5]\nNamedMaterial "m"\n')
    ms, k = mix_of(parse(NAMED + use + QUAD))
    m = ms[k]
    c1, c2 = m.tex_kr - 1, m.tex_kt - 1
    assert 0 <= c1 < k and 0 <= c2 < k                                  # children precede the mix
    assert (ms[c1].type, ms[c2].type) == (capi.PT_MATERIAL_PLASTIC, capi.PT_MATERIAL_MATTE)
    b = scenes.SceneBuilder()
    b.material_plastic(Kd=(0.3, 0.2, 0.1), Ks=(0.25, 0.25, 0.25), roughness=0.1)
    p = b.cur_material
    b.material_matte(Kd=(0.6, 0.5, 0.4))
    q = b.cur_material
    b.material_mix(p, q, (0.3, 0.4, 0.5))
    want = capi.pt_material.from_buffer_copy(raw(b.materials[b.cur_material]))
    want.tex_kr, want.tex_kt = m.tex_kr, m.tex_kt                       # (the tables number their entries differently)
    assert raw(m) == raw(want)
    assert raw(ms[c1]) == raw(b.materials[p]) and raw(ms[c2]) == raw(b.materials[q])


def test_nesting_two_deep_parses():
    body = NAMED + """MakeNamedMaterial "c" "string type" "mirror"
MakeNamedMaterial "inner" "string type" "mix" "string namedmaterial1" "a" "string namedmaterial2" "b" "rgb amount" [0.25 0.25 0.25]
MakeNamedMaterial "outer" "string type" "mix" "string namedmaterial1" "inner" "string namedmaterial2" "c" "rgb amount" [0.6 0.6 0.6]
NamedMaterial "outer"
""" + QUAD
    ms, k = mix_of(parse(body))
    inner = ms[k].tex_kr - 1
    assert ms[inner].type == capi.PT_MATERIAL_MIX and inner < k and ms[ms[k].tex_kt - 1].type == capi.PT_MATERIAL_MIRROR
    assert ms[ms[inner].tex_kr - 1].type == capi.PT_MATERIAL_PLASTIC and [f32(v) for v in ms[inner].kd] == [f32(0.25)] * 3


def test_float_amount_is_not_found_and_texture_amount_binds_a_spectrum_node():
    ms, k = mix_of(parse(NAMED + 'Material "mix" "string namedmaterial1" "a" "string namedmaterial2" "b" "float amount" [0.9]\n' + QUAD))
    assert list(ms[k].kd) == [0.5, 0.5, 0.5] and ms[k].tex_kd == 0          # get_spectrum_texture("amount", 0.5) (Q72)
    body = NAMED + """Texture "mask" "spectrum" "checkerboard" "rgb tex1" [0.9 0.8 0.7] "rgb tex2" [0.1 0.2 0.3] "float uscale" [4] "float vscale" [4] "string aamode" "none"
Texture "fmask" "float" "checkerboard" "float uscale" [4] "float vscale" [4]
Material "mix" "string namedmaterial1" "a" "string namedmaterial2" "b" "texture amount" "mask"
""" + QUAD
    ps = parse(body)
    ms, k = mix_of(ps)
    assert ms[k].tex_kd >= 1 and ps.desc.textures[ms[k].tex_kd - 1].type == capi.PT_TEX_CHECKERBOARD_2D
    ms, k = mix_of(parse(body.replace('"texture amount" "mask"', '"texture amount" "fmask"')))
    assert ms[k].tex_kd == 0 and list(ms[k].kd) == [0.5, 0.5, 0.5]          # a float texture is not a spectrum texture: not found


def test_a_missing_child_becomes_a_matte_from_the_mixs_parameters():
    ms, k = mix_of(parse(NAMED + 'Material "mix" "string namedmaterial1" "a" "string namedmaterial2" "nobody" "rgb Kd" [0.1 0.7 0.2]\n' + QUAD))
    c2 = ms[ms[k].tex_kt - 1]
    assert c2.type == capi.PT_MATERIAL_MATTE and [f32(v) for v in c2.kd] == [f32(0.1), f32(0.7), f32(0.2)]


def test_children_are_looked_up_at_the_directive_and_again_at_a_shape_that_may_set_parameters():
    """"b" is redefined after the mix's MakeNamedMaterial.  A shape that may not set material parameters (arrays only) gets the mix as the
    directive made it, with the first "b"; one that may (a single float) gets the mix made again at the shape, with the second."""
    body = NAMED + """MakeNamedMaterial "m" "string type" "mix" "string namedmaterial1" "a" "string namedmaterial2" "b"
MakeNamedMaterial "b" "string type" "matte" "rgb Kd" [0.05 0.05 0.9]
NamedMaterial "m"
"""
    fixed = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-1 -1 0 1 -1 0 1 1 0]'
    ms, k = mix_of(parse(body + fixed))
    assert [f32(v) for v in ms[ms[k].tex_kt - 1].kd] == [f32(0.6), f32(0.5), f32(0.4)]
    ms, k = mix_of(parse(body + fixed + ' "float sigma" [0]'))
    assert [f32(v) for v in ms[ms[k].tex_kt - 1].kd] == [f32(0.05), f32(0.05), f32(0.9)]


def test_a_none_child_is_refused_by_name():
    with pytest.raises(capi.PtError) as e:
        parse(NAMED + 'MakeNamedMaterial "n" "string type" "none"\nMaterial "mix" "string namedmaterial1" "a" "string namedmaterial2" "n"\n' + QUAD)
    assert e.value.status == 4 and '"n"' in str(e.value) and "mix" in str(e.value)


def test_checkerboard_amount_leaves_few_samples_undecided():
    """The lit quad's cells (mix_cases.LIT_SCALE per uv unit) against the uv bound: the share of a uniform film within the bound of a
    cell edge stays under the cap, so the GPU test's left-out share is the BSDF's own."""
    from test_gpu_delta_light import P_ERR
    margin = MC.lit_uv_margin(P_ERR, 4.0)
    st = np.random.default_rng(9).random((200000, 2)) * MC.LIT_SCALE
    share = (np.abs(st - np.round(st)) <= margin).any(1).mean()
    assert share <= C.MAX_LEFT_OUT and 4 * margin <= C.MAX_LEFT_OUT          # (analytically: two edges per cell and axis)
