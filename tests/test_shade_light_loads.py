"""The Matte shading kernels read the light record through an address space the compiler knows, read from the built library's own device
code (no GPU).

Next-event estimation picks the record out of the LDS copy (scenes with at most PT_LIGHTS_IN_LDS lights) or out of the global table.  Through
one generic reference every field was a flat load, and a flat load counts on both wait counters: the compiler followed each with a wait for
vmcnt(0) AND lgkmcnt(0), which also sat out the next iteration's prefetches.  shade_body now instantiates the block once per address space
under the kernel-uniform `lights_lds`; nothing but this test holds the compiler to it.

The LDS site is found by its address: the record's stride of 112 bytes (sizeof(PtLight)) times the light number, as a 32-bit multiply
whose product is the address register of the LDS reads that follow."""
import os
import re
import subprocess
import sys

import pytest

from helpers import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MATTE = ["k_shade", "k_shade_matte_sorted"]
STRIDE = 112                  # sizeof(PtLight)


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
        if "<k_shade>:" in out:
            return out
    raise AssertionError("no code object with k_shade in %s" % pkg.capi.LIB_PATH)


def kernel_body(disassembly, kernel):
    return [x.split("//")[0].rstrip() for x in disassembly.split("<%s>:" % kernel)[1].split("\n\n")[0].splitlines()]      # without the address / encoding comment


def lds_record_sites(body):
    """[(address register, [LDS read mnemonic, ...], the first wait after them)] for every 32-bit multiply by the record's stride."""
    sites = []
    for n, line in enumerate(body):
        m = re.search(r"v_mul_lo_u32 (v\d+), v\d+, (s\d+)\s*$", line)
        if not m:
            continue
        reg, sreg = m.group(1), m.group(2)
        if not any(re.search(r"s_mov(k_i32|_b32) %s, (0x%x|%d)\s*$" % (sreg, STRIDE, STRIDE), x) for x in body[max(0, n - 6):n]):
            continue
        reads, wait = [], None
        for x in body[n + 1:n + 40]:
            if re.search(r"\bds_read\w* .*, %s( |$)" % reg, x):
                reads.append(x.split()[0])
            elif "s_waitcnt" in x and reads:
                wait = x.strip()
                break
        sites.append((reg, reads, wait))
    return sites


@pytest.mark.parametrize("kernel", MATTE)
def test_no_flat_access(disassembly, kernel):
    body = kernel_body(disassembly, kernel)
    flat = [x.strip() for x in body if re.search(r"\bflat_(load|store|atomic)", x)]
    print(kernel, len(body), "instructions,", len(flat), "flat")
    assert len(body) > 1000
    assert flat == [], flat[:8]


@pytest.mark.parametrize("kernel", MATTE)
def test_light_record_by_lds_reads_waited_on_lgkmcnt_alone(disassembly, kernel):
    body = kernel_body(disassembly, kernel)
    sites = lds_record_sites(body)
    print(kernel, sites)
    assert len(sites) == 1, sites                        # next-event estimation over the LDS copy is the kernel's one reader of s_lights
    reg, reads, wait = sites[0]
    assert len(reads) >= 3 and all(r in ("ds_read_b96", "ds_read_b128", "ds_read_b64") for r in reads), reads      # the vertices, in wide reads
    assert wait is not None and "lgkmcnt" in wait and "vmcnt" not in wait, wait
