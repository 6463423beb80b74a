"""Material "translucent" (materials/translucent.rs) without a GPU: the front end into pt_material, SceneBuilder against the parsed text, the
materials that stay refused, and the numpy restatement the GPU tests lean on (tests/translucent_ref.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import translucent_ref as tr
from helpers import pkg

capi = pkg.capi
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]'
HEAD = 'Sampler "sobol" "integer pixelsamples" 1\nWorldBegin\n'
CHECKS = ('Texture "cc" "spectrum" "checkerboard" "rgb tex1" [0.9 0.1 0.1] "rgb tex2" [0.1 0.1 0.9]\n'
          'Texture "cf" "float" "checkerboard" "float tex1" 0.05 "float tex2" 0.4\n')


def parse_materials(body):
    ps = capi.ParsedScene(text=HEAD + body + "\nWorldEnd")
    d = ps.desc
    return ps, [d.materials[d.meshes[i].material] for i in range(d.n_meshes)]


def test_front_end_fills_pt_material():
    """create_translucent_material (translucent.rs:110-127): defaults, every parameter, "reflect" / "transmit" in kr / kt, constants from
    the material before the shape (Q18), MakeNamedMaterial, and no "eta" / "index"."""
    ps, mats = parse_materials('''
      Material "translucent"
      %(tri)s
      Material "translucent" "rgb Kd" [0.1 0.2 0.3] "rgb Ks" [0.4 0.5 0.6] "rgb reflect" [0.7 0.8 0.9] "rgb transmit" [0.15 0.25 0.35]
               "float roughness" 0.3 "bool remaproughness" "false"
      %(tri)s
      Material "translucent" "rgb Kd" [0.1 0.2 0.3] "float roughness" 0.3
      %(tri)s "rgb Kd" [0.9 0.9 0.9] "float roughness" 0.7 "rgb transmit" [0.6 0.6 0.6]
      MakeNamedMaterial "leaf" "string type" "translucent" "rgb reflect" [0.2 0.3 0.1] "rgb transmit" [0.3 0.5 0.2] "float roughness" 0.25
      NamedMaterial "leaf"
      %(tri)s
      Material "translucent" "float eta" 1.9 "float index" 1.2
      %(tri)s
    ''' % {"tri": TRI})
    m = mats[0]
    assert m.type == capi.PT_MATERIAL_TRANSLUCENT == 8
    assert list(m.kd) == [0.25] * 3 and list(m.ks) == [0.25] * 3 and list(m.kr) == [0.5] * 3 and list(m.kt) == [0.5] * 3
    assert m.roughness == np.float32(0.1) and m.remap_roughness == 1 and m.tex_bump == 0
    assert (m.tex_kd, m.tex_ks, m.tex_kr, m.tex_kt, m.tex_roughness) == (0, 0, 0, 0, 0)
    m = mats[1]
    f = lambda v: [float(np.float32(x)) for x in v]
    assert list(m.kd) == f([0.1, 0.2, 0.3]) and list(m.ks) == f([0.4, 0.5, 0.6])
    assert list(m.kr) == f([0.7, 0.8, 0.9]) and list(m.kt) == f([0.15, 0.25, 0.35])          # reflect -> kr, transmit -> kt
    assert m.roughness == np.float32(0.3) and m.remap_roughness == 0
    m = mats[2]         # Q18: the material's constants first, the shape's only for what the material leaves out
    assert list(m.kd) == f([0.1, 0.2, 0.3]) and m.roughness == np.float32(0.3) and list(m.kt) == f([0.6] * 3) and list(m.kr) == [0.5] * 3
    m = mats[3]
    assert m.type == capi.PT_MATERIAL_TRANSLUCENT and list(m.kr) == f([0.2, 0.3, 0.1]) and list(m.kt) == f([0.3, 0.5, 0.2])
    assert m.roughness == np.float32(0.25) and list(m.kd) == [0.25] * 3
    # "eta" / "index" are not parameters of this material: the descriptor is the default one
    assert bytes(mats[4]) == bytes(mats[0])


def test_front_end_texture_bindings():
    """A texture on each of the five parameters and on "bumpmap"; bindings are looked up shape first (texture_params.rs:85-105)."""
    ps, mats = parse_materials(CHECKS + '''
      Material "translucent" "texture Kd" "cc" "texture Ks" "cc" "texture reflect" "cc" "texture transmit" "cc" "texture roughness" "cf"
               "texture bumpmap" "cf"
      %(tri)s
      Material "translucent" "texture reflect" "cc"
      %(tri)s
      Material "translucent" "texture transmit" "cc"
      %(tri)s
      Material "translucent" "rgb reflect" [1 1 1]
      %(tri)s "texture reflect" "cc" "texture roughness" "cf"
    ''' % {"tri": TRI})
    m = mats[0]
    refs = (m.tex_kd, m.tex_ks, m.tex_kr, m.tex_kt, m.tex_roughness, m.tex_bump)
    assert all(r > 0 for r in refs)
    d = ps.desc
    assert all(d.textures[r - 1].type == capi.PT_TEX_CHECKERBOARD_2D for r in refs)
    assert refs[0] == refs[1] == refs[2] == refs[3] and refs[4] == refs[5] != refs[0]
    assert (m.tex_opacity, m.tex_sigma, m.tex_eta, m.tex_uroughness, m.tex_vroughness) == (0, 0, 0, 0, 0)
    assert mats[1].tex_kr == refs[0] and mats[1].tex_kt == 0
    assert mats[2].tex_kt == refs[0] and mats[2].tex_kr == 0
    assert mats[3].tex_kr == refs[0] and mats[3].tex_roughness == refs[4]            # the shape's binding wins over the material's constant


def test_scene_builder_equals_parsed_text():
    """SceneBuilder.material_translucent produces the descriptor the front end produces for the same text, byte for byte."""
    ps, mats = parse_materials(CHECKS + '''
      Material "translucent"
      %(tri)s
      Material "translucent" "rgb Kd" [0.1 0.2 0.3] "rgb Ks" [0.4 0.5 0.6] "rgb reflect" [0.7 0.8 0.9] "rgb transmit" [0.15 0.25 0.35]
               "float roughness" 0.3 "bool remaproughness" "false"
      %(tri)s
      Material "translucent" "texture Kd" "cc" "texture reflect" "cc" "texture roughness" "cf" "texture bumpmap" "cf"
      %(tri)s
    ''' % {"tri": TRI})
    b = pkg.scenes.SceneBuilder()
    cc = b.texture_checkerboard((0.9, 0.1, 0.1), (0.1, 0.1, 0.9))
    cf = b.texture_checkerboard(0.05, 0.4)
    built = []
    b.material_translucent()
    built.append(b.materials[b.cur_material])
    b.material_translucent(Kd=(0.1, 0.2, 0.3), Ks=(0.4, 0.5, 0.6), reflect=(0.7, 0.8, 0.9), transmit=(0.15, 0.25, 0.35), roughness=0.3, remaproughness=False)
    built.append(b.materials[b.cur_material])
    b.material_translucent(Kd=cc, reflect=cc, roughness=cf, bumpmap=cf)
    built.append(b.materials[b.cur_material])
    assert C.sizeof(capi.pt_material) == 164
    for k, (p, q) in enumerate(zip(mats, built)):
        assert bytes(p) == bytes(q), k
    # the texture nodes the handles name are the parsed ones
    assert ps.desc.textures[mats[2].tex_kd - 1].type == b.textures[built[2].tex_kd - 1].type == capi.PT_TEX_CHECKERBOARD_2D


@pytest.mark.parametrize("name", ["mix", "fourier", "hair", "subsurface", "kdsubsurface"])
def test_other_materials_still_refused(name):
    with pytest.raises(capi.PtError) as e:
        capi.ParsedScene(text=HEAD + 'Material "%s"\n' % name + TRI + "\nWorldEnd")
    assert e.value.status == 4              # PT_ERR_UNSUPPORTED
    assert name in str(e.value) and "translucent" in str(e.value)


# ------------------------------------------------------------------ the restatement itself
def test_transmission_pdf_integrates_to_pi():
    """lambertian.rs:80-86 returns |cos| without INV_PI: over the hemisphere opposite wo it integrates to pi (pbrt-v3's integrates to 1), over
    wo's own hemisphere to 0.  Midpoint rule in (cos theta, phi): the integrand is linear in cos theta, so the rule is exact up to rounding."""
    n = 256
    mu = (np.arange(n) + 0.5) / n
    phi = (np.arange(2 * n) + 0.5) * (np.pi / n)
    MU, PH = np.meshgrid(mu, phi, indexing="ij")
    s = np.sqrt(1 - MU * MU)
    up = np.stack([s * np.cos(PH), s * np.sin(PH), MU], -1).reshape(-1, 3)
    dw = (1.0 / n) * (np.pi / n)
    for wo in ([0.3, -0.2, 0.9], [0.1, 0.7, -0.4]):
        wo = np.tile(np.array(wo) / np.linalg.norm(wo), (len(up), 1))
        other = up * np.array([1, 1, -np.sign(wo[0, 2])])
        own = up * np.array([1, 1, np.sign(wo[0, 2])])
        assert abs(tr.lambert_t_pdf(wo, other).sum() * dw - np.pi) < 1e-9
        assert tr.lambert_t_pdf(wo, own).sum() == 0.0
        assert abs(tr.lambert_r_pdf(wo, own).sum() * dw - 1.0) < 1e-9 and tr.lambert_r_pdf(wo, other).sum() == 0.0
        # through the BSDF: one matching lobe, no averaging
        ls = tr.lobes(Kd=(0.5,) * 3, Ks=(0,) * 3, reflect=(0,) * 3, transmit=(1,) * 3)
        assert abs(tr.bsdf_pdf(ls, wo, other).sum() * dw - np.pi) < 1e-9


def test_diffuse_only_sample_leaves_on_the_far_side():
    rng = np.random.default_rng(3)
    wo = rng.standard_normal((4096, 3)); wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    u = rng.random((4096, 2))
    ls = tr.lobes(Kd=(0.6, 0.5, 0.4), Ks=(0,) * 3, reflect=(0,) * 3, transmit=(1,) * 3)
    assert [l["kind"] for l in ls] == ["lambert_t"]
    f, wi, pdf, t = tr.bsdf_sample_f(ls, wo, u)
    assert (t == (tr.TRANS | tr.DIFFUSE)).all()
    assert (wi[:, 2] * wo[:, 2] < 0).all()
    assert np.allclose(pdf, np.abs(wi[:, 2])) and np.allclose(f, np.array([0.6, 0.5, 0.4]) / np.pi)
    assert np.allclose(np.linalg.norm(wi, axis=1), 1.0)
    # the float32 restatement agrees with the float64 one to rounding
    f32l = tr.diffuse_f32_lobes((0.6, 0.5, 0.4), (0,) * 3, (1,) * 3)
    ff, pp = tr.diffuse_f32_eval(f32l, wo, wi)
    assert np.allclose(ff, tr.bsdf_f(ls, wo, wi), rtol=1e-6) and np.allclose(pp, tr.bsdf_pdf(ls, wo, wi), rtol=1e-6)
    # reflection-only flags leave nothing to sample
    assert (tr.bsdf_sample_f(ls, wo, u, tr.REFL | tr.DIFFUSE | tr.GLOSSY | tr.SPECULAR)[3] == 0).all()


def test_lobe_counts_and_order_for_all_black_combinations():
    """The 16 black / non-black combinations of (Kd, Ks, reflect, transmit): lobe order (translucent.rs:60-104), "no BSDF" (r and t black:
    the ray passes on) against "empty BSDF" (Kd and Ks black: the path ends)."""
    for kd, ks, r, t in itertools.product((0.0, 0.5), repeat=4):
        ls = tr.lobes(Kd=(kd,) * 3, Ks=(ks,) * 3, reflect=(r, 0.0, 0.0), transmit=(0.0, t, 0.0))
        if r == 0 and t == 0:
            assert ls is None
            continue
        assert ls is not None
        want = []
        if kd:
            want += ["lambert_r"] * bool(r) + ["lambert_t"] * bool(t)
        if ks:
            want += ["mf_r"] * bool(r) + ["mf_t"] * bool(t)
        assert [l["kind"] for l in ls] == want
        if not kd and not ks:
            assert ls == []
    # negative values clamp to zero before the tests for black
    assert tr.lobes(reflect=(-1,) * 3, transmit=(-0.5,) * 3) is None
    assert tr.lobes(Kd=(-1,) * 3, Ks=(-1,) * 3) == []
    # colours are products, the roughness is remapped once for both glossy lobes
    ls = tr.lobes(Kd=(0.2, 0.4, 0.6), Ks=(0.5,) * 3, reflect=(0.5, 1.0, 0.0), transmit=(0.25,) * 3, roughness=0.3)
    assert np.allclose(ls[0]["c"], [0.1, 0.4, 0.0]) and np.allclose(ls[1]["c"], [0.05, 0.1, 0.15])
    assert ls[2]["alpha"] == ls[3]["alpha"] == tr.roughness_to_alpha(0.3)
    assert tr.lobes(roughness=0.3, remaproughness=False)[2]["alpha"] == 0.3
