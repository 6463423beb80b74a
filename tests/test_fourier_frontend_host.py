"""Material "fourier" in the .pbrt front end (pth_parse_*_features, PTH_FEATURE_FOURIER_MATERIAL) and SceneBuilder.material_fourier,
without a device: both directive forms, the file-name resolution, one table per file, a material under a mix, the bump map, the failures
that carry the file's name, and the refusal of the plain entry points, word for word."""
import os
import shutil

import numpy as np
import pytest

import fourier_cases as FC
import fourier_tables as FT
from helpers import pkg, scenes

capi = pkg.capi

HEAD = """LookAt 0 -3 2.5  0 0 0.4  0 0 1
Camera "perspective" "float fov" [50]
Film "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" "o.pfm"
Sampler "sobol" "integer pixelsamples" [1]
Integrator "path" "integer maxdepth" [3]
WorldBegin
"""
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0] "float uv" [0 0 1 0 1 1 0 1]'
REFUSAL = 'Material "fourier": outside the accelerated path (matte, plastic, mirror, glass, metal, uber, substrate, translucent are supported)'
ARRAYS = ("mu", "cdf", "offset_and_length", "a")


def parse(body, work_dir, **kw):
    return capi.ParsedScene(text=HEAD + body + "\nWorldEnd\n", work_dir=str(work_dir), fourier_materials=True, **kw)


def raw(m):
    return bytes(memoryview(m).cast("B")) if not isinstance(m, bytes) else m


def shape_material(ps, mesh=-1):
    k = ps.desc.meshes[ps.desc.n_meshes + mesh if mesh < 0 else mesh].material
    return k, capi.pt_material.from_buffer_copy(ps.desc.materials[k])


def record_of(ps, k):
    r = [r for r in ps.fourier if r.material == k]
    assert len(r) == 1
    return r[0]


@pytest.fixture
def files(tmp_path):
    """two.bsdf and sub/rgb.bsdf beside the scene, and the fixture under its own name."""
    FT.write_bsdf(tmp_path / "two.bsdf", FC.table("two_sided"))
    os.makedirs(tmp_path / "sub")
    FT.write_bsdf(tmp_path / "sub" / "rgb.bsdf", FC.table("rgb_long"))
    shutil.copy(FC.ROUGHGOLD, tmp_path / "gold.bsdf")
    return tmp_path


def same_table(got, want):
    assert (got.n_mu, got.n_channels, got.m_max, got.n_coeffs) == (want.n_mu, want.n_channels, want.m_max, want.n_coeffs)
    assert got.eta == float(np.float32(want.eta))
    for k in ARRAYS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), k


def test_plain_entry_points_still_refuse_fourier_word_for_word(files):
    for kw in ({}, dict(mix_materials=True), dict(disney_materials=True), dict(delta_lights=True)):
        with pytest.raises(capi.PtError) as e:
            capi.ParsedScene(text=HEAD + 'Material "fourier" "string bsdffile" "two.bsdf"\n' + QUAD + "\nWorldEnd\n", work_dir=str(files), **kw)
        assert e.value.status == 4 and str(e.value) == "PT_ERR_UNSUPPORTED: " + REFUSAL


@pytest.mark.parametrize("form", ["material", "named"])
def test_both_directive_forms_parse_to_the_builders_records(files, form):
    """SceneBuilder.material_fourier writes the pt_material and the pt_fourier record the parsed text gives, byte for byte, and reads the
    same table."""
    text = '"string bsdffile" "two.bsdf"'
    use = 'Material "fourier" ' + text + "\n" if form == "material" else 'MakeNamedMaterial "f" "string type" "fourier" ' + text + '\nNamedMaterial "f"\n'
    ps = parse(use + QUAD, files)
    k, m = shape_material(ps)
    assert m.type == capi.PT_MATERIAL_FOURIER and m.tex_bump == 0
    b = scenes.SceneBuilder()
    b.material_matte()                                   # (so that the builder's index is not 0 by accident)
    b.material_fourier(bsdffile=str(files / "two.bsdf"))
    assert raw(m) == raw(b.materials[b.cur_material])
    want = capi.pt_fourier.from_buffer_copy(raw(b.fourier[-1]))
    assert want.material == b.cur_material and want.table == 0
    want.material = k                                    # (the tables number their entries differently)
    assert raw(record_of(ps, k)) == raw(want)
    assert len(ps.fourier_tables) == 1 and len(b.fourier_tables) == 1
    same_table(ps.fourier_tables[0], FC.table("two_sided"))
    same_table(b.fourier_tables[0], FC.table("two_sided"))
    sd = b.build()
    assert raw(sd.fourier[-1]) == raw(b.fourier[-1]) and sd.fourier_tables[0] is b.fourier_tables[0]


def test_the_fixture_parses_and_paths_resolve_like_image_maps(files):
    """A relative name is taken from the scene's directory, a subdirectory and an absolute name work as they do for "filename"."""
    body = ('Material "fourier" "string bsdffile" "gold.bsdf"\n' + QUAD + "\n" +
            'Material "fourier" "string bsdffile" "sub/rgb.bsdf"\n' + QUAD + "\n" +
            'Material "fourier" "string bsdffile" "%s"\n' % (files / "two.bsdf") + QUAD)
    ps = parse(body, files)
    assert len(ps.fourier_tables) == 3 and len(ps.fourier) == 3
    for mesh, name in enumerate(("roughgold", "rgb_long", "two_sided")):
        k, m = shape_material(ps, mesh)
        assert m.type == capi.PT_MATERIAL_FOURIER
        same_table(ps.fourier_tables[record_of(ps, k).table], FC.table(name))
    scene = files / "scene.pbrt"                       # ... and from a file, relative to the file
    scene.write_text(HEAD + 'Material "fourier" "string bsdffile" "sub/rgb.bsdf"\n' + QUAD + "\nWorldEnd\n")
    pf = capi.ParsedScene(filename=str(scene), fourier_materials=True)
    same_table(pf.fourier_tables[0], FC.table("rgb_long"))


def test_one_file_named_twice_is_one_table(files):
    body = ('Texture "b" "float" "checkerboard" "float tex1" [0.02] "float tex2" [0] "float uscale" [4] "float vscale" [4]\n'
            'Material "fourier" "string bsdffile" "two.bsdf"\n' + QUAD + "\n" +
            'Material "fourier" "string bsdffile" "two.bsdf" "texture bumpmap" "b"\n' + QUAD + "\n" +
            'Material "fourier" "string bsdffile" "two.bsdf"\n' + QUAD)
    ps = parse(body, files)
    assert len(ps.fourier_tables) == 1
    ks = [shape_material(ps, mesh)[0] for mesh in range(3)]
    assert ks[0] == ks[2] != ks[1]                       # the same material twice is one record, another bump map is another
    assert len(ps.fourier) == 2 and all(r.table == 0 for r in ps.fourier)
    m1 = shape_material(ps, 1)[1]
    assert m1.tex_bump != 0 and ps.desc.textures[m1.tex_bump - 1].type == capi.PT_TEX_CHECKERBOARD_2D
    b = scenes.SceneBuilder()                            # the builder: one file, or one table object, is one table however many materials name it
    t = FC.table("rgb_long")
    b.material_fourier(bsdffile=str(files / "two.bsdf"))
    b.material_fourier(table=t, bumpmap=0.25)
    b.material_fourier(bsdffile=str(files / "two.bsdf"))
    b.material_fourier(table=t)
    assert len(b.fourier_tables) == 2 and [r.table for r in b.fourier] == [0, 1, 0, 1]
    assert b.materials[b.fourier[1].material].tex_bump != 0
    with pytest.raises(ValueError):
        b.material_fourier()
    with pytest.raises(ValueError):
        b.material_fourier(bsdffile="x", table=t)


def test_a_number_as_bumpmap_is_a_constant_texture(files):
    ps = parse('Material "fourier" "string bsdffile" "two.bsdf" "float bumpmap" [0.25]\n' + QUAD, files)
    k, m = shape_material(ps)
    t = ps.desc.textures[m.tex_bump - 1]
    assert t.type == capi.PT_TEX_CONSTANT and t.value[0][0] == 0.25


def test_fourier_under_a_mix(files):
    body = ('MakeNamedMaterial "f" "string type" "fourier" "string bsdffile" "gold.bsdf"\n'
            'MakeNamedMaterial "b" "string type" "matte" "rgb Kd" [0.6 0.5 0.4]\n'
            'Material "mix" "string namedmaterial1" "f" "string namedmaterial2" "b" "rgb amount" [0.3 0.4 0.5]\n')
    ps = parse(body + QUAD, files, mix_materials=True)
    k, m = shape_material(ps)
    assert m.type == capi.PT_MATERIAL_MIX
    c1, c2 = m.tex_kr - 1, m.tex_kt - 1
    assert 0 <= c1 < k and ps.desc.materials[c1].type == capi.PT_MATERIAL_FOURIER and ps.desc.materials[c2].type == capi.PT_MATERIAL_MATTE
    same_table(ps.fourier_tables[record_of(ps, c1).table], FC.table("roughgold"))
    b = scenes.SceneBuilder()
    b.material_fourier(table=FC.table("roughgold"))
    f = b.cur_material
    b.material_matte(Kd=(0.6, 0.5, 0.4))
    b.material_mix(f, b.cur_material, (0.3, 0.4, 0.5))              # usable as a child of material_mix
    assert b.materials[b.cur_material].tex_kr == f + 1


def test_a_missing_or_malformed_file_fails_the_parse_with_its_name(files):
    """create_fourier_material returns the reader's error (materials/fourier.rs:46-52): no lobeless material is rendered."""
    for text, phrase in (('"string bsdffile" "absent.bsdf"', "cannot be opened"), ("", "cannot be opened")):
        with pytest.raises(capi.PtError) as e:
            parse('Material "fourier" ' + text + "\n" + QUAD, files)
        assert 'Material "fourier"' in str(e.value) and phrase in str(e.value)
        assert "absent.bsdf" in str(e.value) or not text
    raw_bytes = bytearray(open(files / "two.bsdf", "rb").read())
    open(files / "short.bsdf", "wb").write(bytes(raw_bytes[:200]))
    raw_bytes[8:12] = (2).to_bytes(4, "little")
    open(files / "flags.bsdf", "wb").write(bytes(raw_bytes))
    for name, phrase in (("short.bsdf", "truncated"), ("flags.bsdf", "flags is 2")):
        with pytest.raises(capi.PtError) as e:
            parse('Material "fourier" "string bsdffile" "%s"\n' % name + QUAD, files)
        assert e.value.status == 4 and name in str(e.value) and phrase in str(e.value), str(e.value)          # (the status every failure of the scene assembly has)
    # a material that no shape uses is never created (get_material_for_shape makes materials at shapes), so its file is never opened
    parse('MakeNamedMaterial "unused" "string type" "fourier" "string bsdffile" "absent.bsdf"\nMaterial "matte"\n' + QUAD, files)


def test_the_other_refused_materials_stay_refused_with_the_bit(files):
    for name in ("hair", "subsurface", "kdsubsurface"):
        with pytest.raises(capi.PtError) as e:
            parse('Material "%s"\n' % name + QUAD, files)
        assert e.value.status == 4 and str(e.value) == "PT_ERR_UNSUPPORTED: " + REFUSAL.replace("fourier", name)
