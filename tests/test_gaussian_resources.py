"""Resource budget of gym_amd/csrc/mxv_gaussian.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

All four instantiations of gaussian_kernel — D = 1, 2, 3, 4 — keep everything in registers: no scratch, no spilled vector or scalar
register, no LDS, no AGPRs, and the occupancy the compiler reported when the kernel was written: 8 waves per SIMD for D = 1, 2, 3 and
7 for D = 4 (DESIGN.md §13 records the register counts).  The report of a kernel includes the out-of-line dims_pair it calls.  Read from
the compiler's resource report of the code object only."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "gym_amd", "csrc", "mxv_gaussian.hip")
OCCUPANCY = {1: 8, 2: 8, 3: 8, 4: 7}      # waves per SIMD, as reported at the time of the change
MAX_VGPRS = {1: 40, 2: 40, 3: 48, 4: 48}  # reported: 33, 36, 46, 48; the bound is the allocation granule (8) above each


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_gaussian_res_")
    try:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", SRC,
                            "-o", os.path.join(d, "k.o"), "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        yield p.stderr
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _resources(text):
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None:
            cur[k.split(" [")[0]] = int(v)
    return out


def _symbol(d):
    return f"_ZN12_GLOBAL__N_115gaussian_kernelILi{d}EEEvNS_12GaussianArgsE"


def test_every_instantiation_stays_in_registers(remarks):
    from gym_amd.policy import MAX_ACTION_DIM

    assert sorted(OCCUPANCY) == list(range(1, MAX_ACTION_DIM + 1))
    res = {k: r for k, r in _resources(remarks).items() if "gaussian_kernel" in k}
    assert sorted(res) == sorted(_symbol(d) for d in OCCUPANCY)
    assert not [k for k in _resources(remarks) if "policy_kernel" in k]      # other tools select the categorical kernels by that name
    for d in OCCUPANCY:
        r = res[_symbol(d)]
        print(d, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0 and r["AGPRs"] == 0, (d, r)
        assert r["Occupancy"] >= OCCUPANCY[d] and r["VGPRs"] <= MAX_VGPRS[d], (d, r)


def test_the_source_uses_no_lds_atomics_or_assembly():
    src = re.sub(r"//.*", "", open(SRC).read())
    for word in ("__shared__", "atomic", "asm"):
        assert word not in src, word
