"""The pooled leaf round fetches a triangle's 48-byte record in THREE vector loads, read from the built library's own device code (no GPU).

load_tri asks for three 16-byte loads.  Left to itself the compiler fetched the first vertex twice, as the two register pairs tri_core's
packed subtractions want: four lane requests per record in kernels that run near the vector L1's request rate.  An
empty asm over the nine vertex components in leaf_finish keeps it to three, and nothing but this test holds that: it rests on what the
compiler does.  bench.py's request-rate model counts three requests per triangle test and is only right while this passes.

The site is found by its address: the one 64-bit multiply-add by the record's stride of 48 in each pooled-leaf kernel; the loads counted
are the ones that follow it off the register pair it writes."""
import os
import re
import subprocess
import sys

import pytest

from helpers import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POOLED = ["k_trace", "k_trace_far", "k_trace_sph_dist"]


def _objdump():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "llvm-objdump")
    if not os.path.exists(path):
        path = "/opt/rocm/llvm/bin/llvm-objdump"
    assert os.path.exists(path), "llvm-objdump of the ROCm toolchain not found"
    return path


@pytest.fixture(scope="module")
def disassembly(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    d = tmp_path_factory.mktemp("code_objects")
    for i, img in enumerate(kernel_resources.code_objects(pkg.capi.LIB_PATH)):
        f = d / ("co_%d.elf" % i)
        f.write_bytes(img)
        out = subprocess.run([_objdump(), "-d", "--no-show-raw-insn", str(f)], capture_output=True, text=True, check=True).stdout
        if "<k_trace>:" in out:
            return out
    raise AssertionError("no code object with k_trace in %s" % pkg.capi.LIB_PATH)


def record_sites(body):
    """[(address register pair, [load mnemonic, ...])] for every multiply-add by 48 in a kernel's disassembly."""
    sites = []
    for n, line in enumerate(body):
        m = re.search(r"v_mad_u64_u32 (v\[\d+:\d+\]), .*, (48|0x30), ", line)
        if m:
            reg = m.group(1)
            loads = [x.split()[0] for x in body[n + 1:n + 16] if "global_load" in x and reg + ", off" in x]
            sites.append((reg, loads))
    return sites


@pytest.mark.parametrize("kernel", POOLED)
def test_pooled_leaf_round_loads_a_record_in_three(disassembly, kernel):
    body = disassembly.split("<%s>:" % kernel)[1].split("\n\n")[0].splitlines()
    sites = record_sites(body)
    print(kernel, sites)
    assert len(sites) == 1, sites                         # the leaf round's helper lanes are the only readers of triangle records in these kernels
    loads = sites[0][1]
    assert len(loads) == 3, loads
    assert sorted(loads) == ["global_load_dwordx3", "global_load_dwordx3", "global_load_dwordx4"], loads      # p0, p2 and p1 + flags: nothing fetched twice
