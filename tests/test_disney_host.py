"""Material "disney" without a device: the restatement tests/disney_ref.py held to the text of materials/disney.rs (lobe lists, the quirks),
its float32 run calibrated against its float64 run on the inputs of the GPU hook test (tests/test_gpu_disney.py), the host's
build_disney_lobes (pt_lobes.h, shared with the device) bit for bit against the float32 run, the .pbrt front end and
SceneBuilder.material_disney.  Uploads (and so the upload's refusals) need a device: they are in the GPU file."""
import ctypes as C_
import os
import shutil
import subprocess

import numpy as np
import pytest

import bsdf_cases as C
import bsdf_ref as R
import disney_cases as DC
import disney_ref as D
from helpers import pkg, scenes

capi = pkg.capi
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_SETTINGS = list(DC.SETTINGS) + list(DC.FLOOR_SETTINGS)


# ---------------------------------------------------------------- the descriptor
def test_abi_constants_and_struct_sizes():
    assert capi.PT_MATERIAL_DISNEY == 10
    assert C_.sizeof(capi.pt_material) == 164          # "color", "eta", "roughness" and "bumpmap" ride in fields the struct already has
    assert C_.sizeof(capi.pt_disney) == 128
    assert capi.PTH_FEATURE_DISNEY_MATERIAL == 8


# ---------------------------------------------------------------- calibration: the float32 run against the float64 run
@pytest.mark.parametrize("name", list(DC.SETTINGS))
def test_float32_restatement_stays_within_bound_and_under_the_cap(name):
    """The inputs of the GPU hook test leave the reference's own arithmetic inside the cap of left-out evaluations, for every flag set."""
    for s in DC.calibration(name).values():
        print(s)
        assert s.left <= C.MAX_LEFT_OUT, (s.what, s.left)          # (within bound: check_eval / check_sample assert it)


@pytest.mark.parametrize("name", list(DC.FLOOR_SETTINGS))
def test_float32_restatement_of_the_directed_settings_stays_within_bound(name):
    for s in DC.calibration(name).values():
        print(s)                                                   # uncapped: check_sample has asserted the bounds


# ---------------------------------------------------------------- the lobe list against the text
@pytest.mark.parametrize("name", ALL_SETTINGS)
def test_lobe_list_matches_the_hand_written_table(name):
    for dt in (np.float64, np.float32):
        b = D.BSDF(DC.params(name), dt)
        assert [(l.kind, l.type) for l in b.lobes] == DC.LOBE_TABLE[name]
    assert len(DC.LOBE_TABLE["thin_all"]) == 8 and len(DC.LOBE_TABLE["glass"]) == 2


def test_distribution_and_tint_values():
    b = D.BSDF(DC.params("aniso"), np.float64)
    aspect = np.sqrt(1.0 - R.c32(0.8) * R.c32(0.9))
    r2 = R.c32(0.3) ** 2
    assert np.isclose(float(b.info["ax"].v), r2 / aspect, rtol=1e-12) and np.isclose(float(b.info["ay"].v), r2 * aspect, rtol=1e-12)
    z = D.BSDF(DC.params("rough_zero"), np.float64)
    assert float(z.info["ax"].v) == R.c32(0.001) == float(z.info["ay"].v)                 # the floor
    assert [float(c.v) for c in D.BSDF(DC.params("black"), np.float64).info["c_tint"]] == [1.0, 1.0, 1.0]
    g = D.BSDF(DC.params("clearcoat"), np.float64).info["gloss"]                           # lerp(0.8, 0.1, 0.001)
    assert np.isclose(float(g.v), (1.0 - R.c32(0.8)) * R.c32(0.1) + R.c32(0.8) * R.c32(0.001), rtol=1e-12)
    t = D.BSDF(DC.params("thin_all"), np.float64)
    assert type(t.lobes[6].dist) is R.TR and type(t.lobes[4].dist) is D.DisneyTR           # thin: the transmission lobe's distribution is the plain one
    assert type(D.BSDF(DC.params("half_trans"), np.float64).lobes[3].dist) is D.DisneyTR
    with pytest.raises(ValueError):
        D.BSDF(DC.disney(scatterdistance=(0.1, 0.0, 0.0)), np.float64)                     # todo!() in the reference


# ---------------------------------------------------------------- the quirks
def _dirs(n, seed):
    rng = np.random.default_rng(seed)
    return C.sphere_dirs(rng, n), C.sphere_dirs(rng, n), rng.random((n, 2)).astype(np.float32)


def test_default_samples_nothing_below_one_third():
    """diffuse, retro, microfacet: u.x < 1/3 picks DisneyDiffuse, whose pdf is 0, and BSDF::sample_f returns None."""
    b = D.BSDF(DC.params("default"), np.float64)
    wo, _, u = _dirs(3000, 11)
    u[:, 0] = (np.arange(3000) % 1365 / 4096.0).astype(np.float32)          # a 2^-12 grid below 1/3
    s = b.sample(wo, u)
    assert not s["und"].any() and (s["type"] == 0).all() and (s["pick"] == 0).all()
    u[:, 0] = np.float32(0.5)
    s = b.sample(wo, u)
    assert (s["type"][~s["und"]] == (R.REFL | R.DIFFUSE)).all() and (s["pick"] == 1).all()          # Retro: the lobe's own type
    v = b.eval(wo, wo * np.array([-1, 1, 1], np.float32))
    r = D.BSDF(dict(DC.params("default")), np.float64)
    r.lobes = r.lobes[1:]                                                    # without DisneyDiffuse: the same pdf sum, divided by 2 instead of 3
    assert np.allclose(v.pdf * 3.0, r.eval(wo, wo * np.array([-1, 1, 1], np.float32)).pdf * 2.0, rtol=1e-12)


def test_clearcoat_pdf_is_the_sum():
    b = D.BSDF(DC.params("clearcoat"), np.float64)
    cc = [l for l in b.lobes if l.kind == "d_clearcoat"][0]
    wo = np.array([[0.3, 0.2, 0.9327379]], np.float32)
    wi = np.array([[-0.1, 0.4, 0.9110434]], np.float32)
    p = float(D.lobe_pdf(cc, R.vexact(wo, np.float64), R.vexact(wi, np.float64), np.zeros(1, bool)).v[0])
    wo64, wi64 = wo[0].astype(np.float64), wi[0].astype(np.float64)
    wh = (wo64 + wi64) / np.linalg.norm(wo64 + wi64)
    a2 = float(cc.gloss.v) ** 2
    dr = (a2 - 1.0) / (R.PI * np.log(a2) * (1.0 + (a2 - 1.0) * wh[2] ** 2))
    assert np.isclose(p, dr + abs(wh[2]) / (4.0 * abs(wo64[2])), rtol=1e-9)
    assert not np.isclose(p, dr * abs(wh[2]) / (4.0 * abs(wo64[2])), rtol=1e-3)          # not the product


def test_clearcoat_cos_theta_at_u0_zero():
    """cos_theta = sqrt(max(0, 1 - powf(alpha2, 1 - u0) / (1 - alpha2))): at u0 = 0 the power is alpha2 itself."""
    b = D.BSDF(DC.params("clearcoat"), np.float64)
    cc = [l for l in b.lobes if l.kind == "d_clearcoat"][0]
    a2 = float(cc.gloss.v) ** 2
    want = np.sqrt(max(0.0, 1.0 - a2 / (1.0 - a2)))
    wo = R.vexact(np.array([[0.0, 0.0, 1.0]], np.float32), np.float64)         # wi = reflect(wo, wh) = 2 cos wh - wo: wi.z = 2 cos^2 - 1
    s = D.lobe_sample(cc, wo, R.E(np.zeros(1)), R.E(np.full(1, 0.25)), np.zeros(1, bool))
    assert np.isclose(float(s["wi"][2].v[0]), 2.0 * want * want - 1.0, rtol=1e-12)


# ---------------------------------------------------------------- the host's build_disney_lobes, bit for bit
KIND = {"lambert_t": 0, "mf_r": 5, "mf_t": 6, "d_diffuse": 8, "d_fakess": 9, "d_retro": 10, "d_sheen": 11, "d_clearcoat": 12}
PROGRAM = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include "pt_lobes.h"
static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
int main() {
    static const float P[][16] = {
%s
    };
    for (unsigned s = 0; s < sizeof(P) / sizeof(P[0]); s++) {
        PtDisneyParams dp;
        std::memset(&dp, 0, sizeof(dp));
        for (int i = 0; i < 3; i++) dp.color[i] = P[s][i];
        for (int i = 0; i < PT_DP_COUNT; i++) dp.f[i] = P[s][3 + i];
        dp.thin = P[s][15] != 0.0f;
        PtLobe l[PT_DISNEY_MOST_LOBES];
        const unsigned n = build_disney_lobes(dp, l);
        std::printf("setting %%u %%u\n", s, n);
        for (unsigned i = 0; i < n; i++)
            std::printf("%%u %%u %%u %%08x %%08x %%08x %%08x %%08x %%08x %%08x %%08x %%08x %%08x %%08x %%08x %%08x\n", l[i].kind, l[i].type, l[i].fresnel, bits(l[i].r[0]),
                        bits(l[i].r[1]), bits(l[i].r[2]), bits(l[i].ax), bits(l[i].ay), bits(l[i].t[0]), bits(l[i].t[1]), bits(l[i].t[2]), bits(l[i].eta_b),
                        bits(l[i].fr_eta_i), bits(l[i].fr_eta_t), bits(l[i].oa), bits(l[i].ob));
    }
    return 0;
}
"""
ORDER = ("metallic", "eta", "roughness", "speculartint", "anisotropic", "sheen", "sheentint", "clearcoat", "clearcoatgloss", "spectrans", "flatness",
         "difftrans")          # PtDisneyParams::f


def test_host_build_lobes_is_bit_equal_to_the_float32_restatement(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # host code only (a .cpp file): pt_device.h names HIP's vector types
    cxx = [hipcc] if os.path.exists(hipcc) else [shutil.which("g++") or "c++", "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    rows = []
    for name in ALL_SETTINGS:
        q = dict(D.DEFAULTS, **{k: v for k, v in DC.params(name).items() if k != "type"})
        vals = list(q["color"]) + [q[k] for k in ORDER] + [1.0 if q["thin"] else 0.0]
        rows.append("        {" + ", ".join(float(f32(v)).hex() + "f" for v in vals) + "},")
    src = tmp_path / "disney_lobes.cpp"
    src.write_text(PROGRAM % "\n".join(rows))
    exe = tmp_path / "disney_lobes"
    subprocess.check_call(cxx + ["-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pbrt-r3_amd", "csrc"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")

    def b32(e):
        return "%08x" % int(np.asarray(e.v, np.float32).view(np.uint32))
    at = 0
    for k, name in enumerate(ALL_SETTINGS):
        lobes = D.BSDF(DC.params(name), np.float32).lobes
        assert lines[at] == "setting %d %d" % (k, len(lobes)), (name, lines[at])
        for i, l in enumerate(lobes):
            got = lines[at + 1 + i].split()
            assert (int(got[0]), int(got[1])) == (KIND[l.kind], l.type), (name, i, got)
            assert got[3:6] == [b32(c) for c in l.r], (name, i, "R / T / weights", got[3:6], [b32(c) for c in l.r])
            if l.kind in ("mf_r", "mf_t"):
                assert got[6:8] == [b32(l.dist.ax), b32(l.dist.ay)], (name, i, "ax ay")
                sep = 0x100 if isinstance(l.dist, D.DisneyTR) else 0
                assert int(got[2]) == (3 | sep if l.kind == "mf_r" else sep), (name, i, "fresnel / g switch", got[2])
            if l.kind == "mf_r":
                assert got[8:11] == [b32(c) for c in l.r0], (name, i, "cspec0")
                assert got[12:14] == [b32(l.metallic), b32(l.eta)], (name, i, "metallic eta")
            if l.kind == "mf_t":
                assert got[11] == b32(l.eta_b), (name, i, "eta")
            if l.kind in ("d_fakess", "d_retro"):
                assert got[14] == b32(l.roughness), (name, i, "roughness")
            if l.kind == "d_clearcoat":
                assert got[14:16] == [b32(l.weight), b32(l.gloss)], (name, i, "weight gloss")
        at += 1 + len(lobes)


# ---------------------------------------------------------------- the .pbrt front end (pth_parse_*_features, PTH_FEATURE_DISNEY_MATERIAL)
HEAD = """LookAt 0 -3 2.5  0 0 0.4  0 0 1
Camera "perspective" "float fov" [50]
Film "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" "o.pfm"
Sampler "sobol" "integer pixelsamples" [1]
Integrator "path" "integer maxdepth" [3]
WorldBegin
"""
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0] "float uv" [0 0 1 0 1 1 0 1]'
REFUSAL = 'Material "disney": outside the accelerated path (matte, plastic, mirror, glass, metal, uber, substrate, translucent are supported)'
FLOATS = ("metallic", "speculartint", "anisotropic", "sheen", "sheentint", "clearcoat", "clearcoatgloss", "spectrans", "flatness", "difftrans")          # PT_DISNEY_*


def parse(body, **kw):
    return capi.ParsedScene(text=HEAD + body + "\nWorldEnd\n", disney_materials=True, **kw)


def raw(m):
    return bytes(memoryview(m).cast("B")) if not isinstance(m, bytes) else m


def shape_material(ps):
    k = ps.desc.meshes[ps.desc.n_meshes - 1].material
    return k, capi.pt_material.from_buffer_copy(ps.desc.materials[k])


def record_of(ps, k):
    r = [r for r in ps.disney if r.material == k]
    assert len(r) == 1
    return r[0]


def test_plain_entry_points_still_refuse_disney_word_for_word():
    for kw in ({}, dict(mix_materials=True), dict(quadric_shapes=True)):
        with pytest.raises(capi.PtError) as e:
            capi.ParsedScene(text=HEAD + 'Material "disney"\n' + QUAD + "\nWorldEnd\n", **kw)
        assert e.value.status == 4 and str(e.value) == "PT_ERR_UNSUPPORTED: " + REFUSAL


def test_defaults_of_every_parameter():
    ps = parse('Material "disney"\n' + QUAD)
    k, m = shape_material(ps)
    assert m.type == capi.PT_MATERIAL_DISNEY
    assert list(m.kd) == [0.5, 0.5, 0.5] and m.eta == 1.5 and m.roughness == 0.5 and (m.tex_kd, m.tex_eta, m.tex_roughness, m.tex_bump) == (0, 0, 0, 0)
    r = record_of(ps, k)
    assert list(r.value) == [0.0, 0.0, 0.0, 0.0, 0.5, 0.0, 1.0, 0.0, 0.0, 1.0] and list(r.tex) == [0] * 10
    assert r.thin == 0 and list(r.scatterdistance) == [0.0, 0.0, 0.0] and r.tex_scatterdistance == 0
    assert [r.value[getattr(capi, "PT_DISNEY_" + n.upper())] for n in FLOATS] == [D.DEFAULTS[n] for n in FLOATS]


TEXT = ('"rgb color" [0.6 0.45 0.3] "float metallic" [0.2] "float eta" [1.4] "float roughness" [0.35] "float speculartint" [0.1] "float anisotropic" [0.4] '
        '"float sheen" [0.6] "float sheentint" [0.7] "float clearcoat" [0.5] "float clearcoatgloss" [0.25] "float spectrans" [0.3] "float flatness" [0.15] '
        '"float difftrans" [0.8] "bool thin" "true" "rgb scatterdistance" [0.5 0.2 0.1]')
BUILDER = dict(color=(0.6, 0.45, 0.3), metallic=0.2, eta=1.4, roughness=0.35, speculartint=0.1, anisotropic=0.4, sheen=0.6, sheentint=0.7, clearcoat=0.5,
               clearcoatgloss=0.25, spectrans=0.3, flatness=0.15, difftrans=0.8, thin=True, scatterdistance=(0.5, 0.2, 0.1))


@pytest.mark.parametrize("form", ["material", "named"])
def test_both_directive_forms_parse_to_the_builders_records(form):
    """SceneBuilder.material_disney writes the pt_material and the pt_disney record the parsed text gives, byte for byte."""
    use = 'Material "disney" ' + TEXT + "\n" if form == "material" else 'MakeNamedMaterial "d" "string type" "disney" ' + TEXT + '\nNamedMaterial "d"\n'
    ps = parse(use + QUAD)
    k, m = shape_material(ps)
    b = scenes.SceneBuilder()
    b.material_matte()                                   # (so that the builder's index is not 0 by accident)
    b.material_disney(**BUILDER)
    assert raw(m) == raw(b.materials[b.cur_material])
    want = capi.pt_disney.from_buffer_copy(raw(b.disney[-1]))
    assert want.material == b.cur_material
    want.material = k                                    # (the tables number their entries differently)
    assert raw(record_of(ps, k)) == raw(want)
    assert raw(b.build().disney[-1]) == raw(b.disney[-1])


def test_disney_under_a_mix():
    body = ('MakeNamedMaterial "d" "string type" "disney" "rgb color" [0.2 0.7 0.4] "float sheen" [1]\n'
            'MakeNamedMaterial "b" "string type" "matte" "rgb Kd" [0.6 0.5 0.4]\n'
            'Material "mix" "string namedmaterial1" "d" "string namedmaterial2" "b" "rgb amount" [0.3 0.4 0.5]\n')
    ps = parse(body + QUAD, mix_materials=True)
    k, m = shape_material(ps)
    assert m.type == capi.PT_MATERIAL_MIX
    c1, c2 = m.tex_kr - 1, m.tex_kt - 1
    assert 0 <= c1 < k and ps.desc.materials[c1].type == capi.PT_MATERIAL_DISNEY and ps.desc.materials[c2].type == capi.PT_MATERIAL_MATTE
    r = record_of(ps, c1)
    assert r.value[capi.PT_DISNEY_SHEEN] == 1.0 and [f32(v) for v in ps.desc.materials[c1].kd] == [f32(0.2), f32(0.7), f32(0.4)]
    b = scenes.SceneBuilder()
    b.material_disney(color=(0.2, 0.7, 0.4), sheen=1.0)
    d = b.cur_material
    b.material_matte(Kd=(0.6, 0.5, 0.4))
    b.material_mix(d, b.cur_material, (0.3, 0.4, 0.5))              # usable as a child of material_mix
    assert b.materials[b.cur_material].tex_kr == d + 1


TEXTURES = """Texture "fc" "float" "checkerboard" "float tex1" [0.9] "float tex2" [0.1] "float uscale" [4] "float vscale" [4] "string aamode" "none"
Texture "cc" "spectrum" "checkerboard" "rgb tex1" [0.9 0.8 0.7] "rgb tex2" [0.1 0.2 0.3] "float uscale" [4] "float vscale" [4] "string aamode" "none"
"""


def test_float_and_colour_textures_and_bumpmap_on_parameters():
    ps = parse(TEXTURES + 'Material "disney" "texture color" "cc" "texture metallic" "fc" "texture roughness" "fc" "texture clearcoat" "fc" "texture bumpmap" "fc"\n' + QUAD)
    k, m = shape_material(ps)
    r = record_of(ps, k)
    assert m.tex_kd >= 1 and m.tex_roughness >= 1 and m.tex_bump == m.tex_roughness and m.tex_kd != m.tex_roughness
    assert r.tex[capi.PT_DISNEY_METALLIC] == m.tex_roughness and r.tex[capi.PT_DISNEY_CLEARCOAT] == m.tex_roughness
    assert [r.tex[i] for i in range(10) if i not in (capi.PT_DISNEY_METALLIC, capi.PT_DISNEY_CLEARCOAT)] == [0] * 8
    assert list(m.kd) == [0.5, 0.5, 0.5] and m.roughness == 0.5 and r.value[capi.PT_DISNEY_METALLIC] == 0.0          # the (unused) constants stay the defaults
    b = scenes.SceneBuilder()
    fc = b.texture_checkerboard(0.9, 0.1, uscale=4.0, vscale=4.0, aamode="none")
    cc = b.texture_checkerboard((0.9, 0.8, 0.7), (0.1, 0.2, 0.3), uscale=4.0, vscale=4.0, aamode="none")
    b.material_disney(color=cc, metallic=fc, roughness=fc, clearcoat=fc, bumpmap=fc)
    bm, br = b.materials[b.cur_material], b.disney[-1]
    assert (bm.tex_kd, bm.tex_roughness, bm.tex_bump) == (cc.index + 1, fc.index + 1, fc.index + 1)
    assert list(br.tex) == [fc.index + 1 if i in (capi.PT_DISNEY_METALLIC, capi.PT_DISNEY_CLEARCOAT) else 0 for i in range(10)]
    assert list(br.value) == list(r.value) and list(bm.kd) == list(m.kd) and bm.roughness == m.roughness


def test_a_colour_texture_on_metallic_is_refused():
    with pytest.raises(capi.PtError) as e:
        parse(TEXTURES + 'Material "disney" "texture metallic" "cc"\n' + QUAD)
    assert e.value.status == 4 and "metallic" in str(e.value) and "float texture" in str(e.value)


def test_scatterdistance_is_refused_unless_thin():
    with pytest.raises(capi.PtError) as e:
        parse('Material "disney" "rgb scatterdistance" [0.1 0 0]\n' + QUAD)
    assert e.value.status == 4 and "scatterdistance" in str(e.value) and "thin" in str(e.value)
    ps = parse('Material "disney" "rgb scatterdistance" [0.1 0 0] "bool thin" "true"\n' + QUAD)
    k, _ = shape_material(ps)
    r = record_of(ps, k)
    assert r.thin == 1 and [f32(v) for v in r.scatterdistance] == [f32(0.1), 0.0, 0.0]
    parse('Material "disney" "rgb scatterdistance" [0 0 0]\n' + QUAD)          # black: the regular diffuse lobe


def test_the_same_material_twice_is_one_record_and_another_parameter_is_another():
    ps = parse('Material "disney" "float sheen" [0.5]\n' + QUAD + '\nMaterial "disney" "float sheen" [0.5]\n' + QUAD + '\nMaterial "disney" "float sheen" [0.6]\n' + QUAD)
    ks = [ps.desc.meshes[i].material for i in range(ps.desc.n_meshes)]
    assert ks[0] == ks[1] != ks[2] and len(ps.disney) == 2


# ---------------------------------------------------------------- the MIS quadrature of the GPU test, held to the restatement's own sampler
@pytest.mark.parametrize("name", ["sheen", "clearcoat"])
def test_mis_quadrature_meets_the_restatements_sampler(name):
    """disney_cases._mis_at takes the expectation of the BSDF half over densities written down per lobe (cosine, visible normals, the
    clearcoat's gtr1 cos_h / (4 wo . wh)), not over what the lobes report.  Here the same half is drawn: disney_ref's sample_f on random
    u at one wo, its returned f and pdf into B = f cos sp / (sp^2 + lp^2).  The drawn mean must lie within five standard errors of the
    quadrature's, and the share of samples that return None must be one minus the densities' mass."""
    theta_o, n = 0.12, 60000
    b = DC.truth(name)
    ea, eb, var, mass = DC._mis_at(b, theta_o, 480, 160, False)
    rng = np.random.default_rng(71)
    u = rng.random((n, 2)).astype(np.float32)
    wo = np.tile(np.array([np.sin(theta_o), 0.0, np.cos(theta_o)]), (n, 1))
    s = b.sample(wo.astype(np.float32), u)          # (float32 wo: 6e-8 off the quadrature's)
    some = (s["type"] != 0) & (s["pdf"] > 0)
    cos = np.abs(s["wi"][:, 2])
    lp = 1.0 / (2.0 * np.pi * np.pi * np.sqrt(np.maximum(1.0 - cos * cos, 1e-24)))
    sp = s["pdf"]
    with np.errstate(all="ignore"):
        B = np.where(some[:, None], s["f"] * (cos * sp / (sp * sp + lp * lp))[:, None], 0.0)
    se = B.std(0) / np.sqrt(n)
    print(name, "drawn", B.mean(0), "quadrature", eb, "5 se", 5 * se, "None share", 1 - some.mean(), "1 - mass", 1 - mass)
    assert (np.abs(B.mean(0) - eb) <= 5.0 * se).all()
    assert abs((1 - some.mean()) - (1 - mass)) <= 5.0 * np.sqrt(mass * (1 - mass) / n)
    assert 0.25 <= 1 - mass < 0.35                   # a quarter of the picks is DisneyDiffuse (Q84); the rest leave through the horizon


def test_mis_moments_can_tell_the_reported_pdfs():
    """With DisneyDiffuse's pdf repaired to cos / pi in the averaged pdf, the frame mean moves by far more than the GPU test's bound."""
    n = 64 * 64 * 16
    for name in ("sheen", "clearcoat"):
        mean, var = DC.mis_moments(name)
        other, _ = DC.mis_moments(name, True)
        assert (np.abs(other - mean) > 5.0 * np.sqrt(var / n)).all(), name
