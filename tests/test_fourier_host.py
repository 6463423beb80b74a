"""Material "fourier" without a device: the restatement tests/fourier_ref.py held to the reference's own known-answer test
(tests/fourierbsdf.rs, its eight recorded numbers as values), its float32 run calibrated against its float64 run on the inputs of the
GPU hook test (tests/test_gpu_fourier.py), the measured iteration maxima against the device's loop caps, the library's reader
(pth_fourier_read) against an independent numpy parse and against corrupted copies, the ABI's constants and sizes.  Uploads (and so the
upload's refusals) need a device: they are in the GPU file."""
import ctypes as C_
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bsdf_cases as C
import bsdf_ref as R
import fourier_cases as FC
import fourier_ref as FR
import fourier_tables as FT
from helpers import pkg

capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrt-r3_amd", "csrc")


def rel(a, b):
    return abs(a - b) / abs(b)


# ---------------------------------------------------------------- the reference's own known answers
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_meets_the_eight_recorded_numbers(dtype):
    rec = FC.RECORDED
    b = FR.BSDF(FC.table("roughgold"), dtype)
    wo, wi = FC.normalize32(rec["wo"])[None], FC.normalize32(rec["wi"])[None]
    e = b.eval(wo, wi, R.ALL)
    assert rel(FC.luminance(e.f)[0], rec["f_y"]) < FC.RECORDED_REL
    assert rel(e.pdf[0], rec["pdf"]) < FC.RECORDED_REL
    assert rel(b.eval(wi, wo, R.ALL).pdf[0], rec["pdf_swapped"]) < FC.RECORDED_REL
    s = b.sample(wo, np.array([rec["u"]], np.float32), R.ALL)
    assert s["type"][0] == FR.TYPE
    assert rel(FC.luminance(s["f"])[0], rec["sample_f_y"]) < FC.RECORDED_REL
    assert rel(s["pdf"][0], rec["sample_pdf"]) < FC.RECORDED_REL
    for k in range(3):
        assert rel(s["wi"][0, k], rec["sample_wi"][k]) < FC.RECORDED_REL


# ---------------------------------------------------------------- calibration: the float32 run against the float64 run
@pytest.mark.parametrize("name", FC.TABLES)
def test_float32_restatement_stays_within_bound_and_under_the_cap(name):
    """Every comparison of run_table asserts err <= bound; here the shares left out stay under bsdf_cases.MAX_LEFT_OUT as well."""
    stats = list(FC.calibration(name).values())
    print(FC.summary("f32", name, stats))
    for s in stats:
        assert s.left <= C.MAX_LEFT_OUT, (s.what, s.left)
    if name != "dark":
        held = {s.what.split(" all ")[1]: s.n for s in stats if " all " in s.what}
        assert held["eval f"] > 1800 and held["sample mu"] > 800, held


def test_dark_table_gives_nothing():
    wo, wi, u = FC.inputs("dark")
    for dtype in (np.float64, np.float32):
        b = FR.BSDF(FC.table("dark"), dtype)
        e = b.eval(wo, wi, R.ALL)
        assert not e.f.any() and not e.pdf.any()
        assert not b.sample(wo, u, R.ALL)["type"].any()


def test_a_row_without_energy_samples_nothing():
    """Rough gold has no energy for wo below the surface: maximum == 0, pdf = NaN, max(0, NaN) = 0, None -- half of all drawn wo."""
    wo, _, u = FC.inputs("roughgold")
    s = FC.truth_sample("roughgold", R.ALL)
    below = wo[:FC.N_BULK, 2] < 0
    assert 0.4 < below.mean() < 0.6
    assert not s["type"][:FC.N_BULK][below].any() and s["type"][:FC.N_BULK][~below].all()
    assert not s["maximum"][:FC.N_BULK][below].any()


def test_the_lobe_matches_no_specular_request():
    """reflection | transmission | glossy: inside ALL and NOSPEC, outside REFL_ONLY (and outside both of whitted's specular requests)."""
    b = FC.truth("two_sided")
    assert b.matches(R.ALL) and b.matches(R.NOSPEC) and not b.matches(R.REFL_ONLY)
    assert not b.matches(R.REFL | R.SPECULAR) and not b.matches(R.TRANS | R.SPECULAR)


def test_iteration_maxima_against_the_device_caps():
    """pt_fourier.h: each cap is at least four times the most iterations the float32 restatement takes over every sampling input."""
    text = open(os.path.join(CSRC, "pt_fourier.h")).read()
    cap_mu = int(re.search(r"#define PT_FOURIER_MU_ITERS (\d+)", text).group(1))
    cap_phi = int(re.search(r"#define PT_FOURIER_PHI_ITERS (\d+)", text).group(1))
    it_mu, it_phi = FC.iteration_maxima()
    print("iterations: sample_catmull_rom_2d", it_mu, "sample_fourier", it_phi, "caps", cap_mu, cap_phi)
    assert it_mu >= 2 and it_phi >= 2
    assert cap_mu >= 4 * it_mu and cap_phi >= 4 * it_phi
    assert "at most %d iterations in the first loop and %d in the" % (it_mu, it_phi) in " ".join(text.replace("//", " ").split())          # the numbers written beside the caps


# ---------------------------------------------------------------- the reader
ARRAYS = ("mu", "cdf", "offset_and_length", "a")


def test_reader_equals_an_independent_parse_of_the_fixture():
    d = FR.parse_file(FC.ROUGHGOLD)
    assert os.path.getsize(FC.ROUGHGOLD) == 207354 and d["trailing"] == 682          # the bytes after the coefficients are ignored
    t = capi.read_fourier_table(FC.ROUGHGOLD)
    assert (t.n_mu, t.n_channels, t.m_max, t.n_coeffs) == (d["n_mu"], d["n_channels"], d["m_max"], d["n_coeffs"]) == (58, 3, 172, 41502)
    assert t.eta == d["eta"]
    for k in ARRAYS:
        assert np.array_equal(getattr(t, k).view(np.uint32), d[k].view(np.uint32)), k
    assert t.mu[28] == 0 and t.mu[29] == 0 and (np.diff(t.mu) >= 0).all()          # the node 0 twice: "strictly increasing" would refuse the reference's own file
    T = FR.Table(t)
    assert np.isinf(T.recip[0]) and T.recip[5] == np.float32(0.2)
    assert T.a0[T.m == 0].sum() == 0 and np.array_equal(T.a0[T.m > 0], T.a[T.off[T.m > 0]])


@pytest.mark.parametrize("name", ["two_sided", "rgb_long", "dark"])
def test_reader_round_trips_the_synthetic_tables(tmp_path, name):
    t = FC.table(name)
    got = capi.read_fourier_table(FT.write_bsdf(tmp_path / (name + ".bsdf"), t, trailing=b"trailing bytes"))
    assert (got.n_mu, got.n_channels, got.m_max, got.n_coeffs, got.eta) == (t.n_mu, t.n_channels, t.m_max, t.n_coeffs, float(np.float32(t.eta)))
    for k in ARRAYS:
        assert np.array_equal(getattr(got, k), getattr(t, k)), k


def test_synthetic_tables_are_what_their_docstring_says():
    t = FC.table("two_sided")
    L = t.offset_and_length.reshape(-1, 2)
    assert list(t.mu) == [-1.0, np.float32(-0.6), 0.0, np.float32(0.3), np.float32(0.8), 1.0] and t.n_channels == 1
    assert sorted(set(L[:, 1].tolist())) == [0, 1, 2, 3, 4, 5]
    t = FC.table("rgb_long")
    L = t.offset_and_length.reshape(-1, 2)
    assert t.n_channels == 3 and t.n_mu == 8 and L[:, 1].max() == 70 and (L[:, 1] == 0).any()
    assert (L[:, 0] % 2 == 1).all()                  # 4 (mod 8) bytes: no run starts on 16 bytes
    assert not FC.table("dark").offset_and_length.reshape(-1, 2)[:, 1].any()
    for name in ("two_sided", "rgb_long"):           # positive functions: the truth's f is positive where the table has energy
        wo, wi, _ = FC.inputs(name)
        e = FC.truth_eval(name, R.ALL)
        assert (e.f >= 0).all() and (e.pdf >= 0).all() and (e.f[:FC.N_BULK] > 0).mean() > 0.9


def _corrupt(tmp_path, name, edit):
    """A copy of the two_sided file with `edit(bytearray, table)` applied."""
    t = FC.table("two_sided")
    path = FT.write_bsdf(tmp_path / name, t)
    raw = bytearray(open(path, "rb").read())
    raw = edit(raw, t) or raw
    open(path, "wb").write(bytes(raw))
    return path


def _set_i32(raw, at, v):
    raw[at:at + 4] = struct.pack("<i", v)


def _pairs_at(t):
    return 64 + 4 * t.n_mu + 4 * t.n_mu * t.n_mu


REFUSALS = {
    "truncated": (lambda raw, t: raw[:len(raw) - 40], "truncated"),
    "truncated_header": (lambda raw, t: raw[:30], "truncated"),
    "bad_magic": (lambda raw, t: raw.__setitem__(slice(0, 8), b"SCATFUN\x02"), "magic"),
    "flags_2": (lambda raw, t: _set_i32(raw, 8, 2), "flags is 2"),
    "n_channels_2": (lambda raw, t: _set_i32(raw, 8 + 16, 2), "n_channels is 2"),
    "n_bases_2": (lambda raw, t: _set_i32(raw, 8 + 20, 2), "n_bases is 2"),
    "offset_and_length_past_the_end": (lambda raw, t: _set_i32(raw, _pairs_at(t) + 8 * 3, t.n_coeffs - 1), "past the end"),
    "negative_length": (lambda raw, t: _set_i32(raw, _pairs_at(t) + 8 * 3 + 4, -1), "negative length"),
    "length_above_m_max": (lambda raw, t: _set_i32(raw, _pairs_at(t) + 8 * 3 + 4, t.m_max + 1), "above m_max"),
    "negative_offset": (lambda raw, t: _set_i32(raw, _pairs_at(t) + 8 * 3, -4), "negative offset"),
    "mu_steps_back": (lambda raw, t: raw.__setitem__(slice(64 + 8, 64 + 12), struct.pack("<f", -0.7)), "mu steps back at node 2"),
    "mu_repeats_with_other_cdf": (lambda raw, t: raw.__setitem__(slice(64 + 8, 64 + 12), struct.pack("<f", -0.6)), "mu repeats at node 2 and the cdf columns"),
    "huge_n_mu_in_a_short_file": (lambda raw, t: _set_i32(raw, 8 + 4, 32768), "truncated (mu)"),
    "huge_n_coeffs_in_a_short_file": (lambda raw, t: _set_i32(raw, 8 + 8, 2 ** 31 - 1), "truncated (coefficients)"),
    "mu_not_finite": (lambda raw, t: raw.__setitem__(slice(64 + 4, 64 + 8), struct.pack("<f", float("nan"))), "not finite"),
    "n_mu_1": (lambda raw, t: _set_i32(raw, 8 + 4, 1), "n_mu is 1"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_reader_refuses_a_corrupted_copy_by_name(tmp_path, case):
    edit, phrase = REFUSALS[case]
    path = _corrupt(tmp_path, case + ".bsdf", edit)
    with pytest.raises(capi.PtError) as e:
        capi.read_fourier_table(path)
    assert e.value.status == 1              # PT_ERR_INVALID_ARGUMENT
    assert os.path.basename(path) in str(e.value) and phrase in str(e.value), str(e.value)


def test_reader_refuses_a_missing_file_by_name(tmp_path):
    with pytest.raises(capi.PtError) as e:
        capi.read_fourier_table(tmp_path / "nowhere.bsdf")
    assert e.value.status == 1 and "nowhere.bsdf" in str(e.value) and "cannot be opened" in str(e.value)


# ---------------------------------------------------------------- the descriptor
def test_abi_constants_and_struct_sizes():
    assert capi.PT_MATERIAL_FOURIER == 11
    assert C_.sizeof(capi.pt_material) == 164          # "bumpmap" rides in a field the struct already has, the table in a side record
    assert C_.sizeof(capi.pt_fourier_table) == 64 and C_.sizeof(capi.pt_fourier) == 16
    assert C_.sizeof(capi.pt_scene_info) == 96 and capi.pt_scene_info.fourier_capped.offset == 92          # the counter took the reserved word
    assert capi.PTH_FEATURE_FOURIER_MATERIAL == 64 and capi.PT_KERNELS_FOURIER == 5
    header = open(os.path.join(ROOT, "include", "pbrtgpu.h")).read()
    host = open(os.path.join(ROOT, "include", "pbrtgpu_host.h")).read()
    assert re.search(r"PT_MATERIAL_FOURIER = 11\b", header) and re.search(r"#define PT_KERNELS_FOURIER 5\b", header)
    assert re.search(r"#define PT_ABI_VERSION 9\b", header)
    assert re.search(r"#define PTH_FEATURE_FOURIER_MATERIAL 64u", host)
    lib = capi.load_library()
    for sym in ("pt_scene_set_fourier", "pth_fourier_read", "pth_fourier_table_of", "pth_fourier_free", "pth_scene_get_fourier"):
        assert hasattr(lib, sym), sym


PROGRAM = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include "pt_lobes.h"
int main() {
    std::printf("%u %u %u %u %u %u %u\n", pt_lobes_most(PT_MATERIAL_FOURIER), (unsigned)PT_LOBE_FOURIER, (unsigned)sizeof(PtLobe), (unsigned)sizeof(PtMaterial),
                (unsigned)sizeof(PtFourierTable), (unsigned)sizeof(PtScene), (unsigned)sizeof(PtInstance));
    return 0;
}
"""


def test_lobes_most_and_the_device_record_sizes(tmp_path):
    """pt_lobes_most gains its entry (1); PtLobe, PtMaterial, PtScene and PtInstance keep the sizes they had before the material."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # host code only (a .cpp file): pt_device.h names HIP's vector types
    cxx = [hipcc] if os.path.exists(hipcc) else [shutil.which("g++") or "c++", "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    src = tmp_path / "fourier_sizes.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "fourier_sizes"
    subprocess.check_call(cxx + ["-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[:5] == [1, 13, 80, 464, 80], got
    assert got[5:] == [1632, 144], got
