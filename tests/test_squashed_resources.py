"""Resource budget of gym_amd/csrc/mxv_squashed.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

All eight instantiations — squashed_kernel and squashed_backward_kernel for D = 1, 2, 3, 4 — keep everything in registers: no scratch,
no spilled vector or scalar register, no LDS, no AGPRs, and the occupancy the compiler reported when the kernels were written: 8 waves
per SIMD for D = 1, 2 and 7 for D = 3, 4, forwards and backwards (DESIGN.md §21 records the register counts).  The report of a kernel
includes the out-of-line functions it calls.  Read from the compiler's resource report of the code object only."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT
from test_gaussian_resources import HIPCC, _resources

SRC = os.path.join(ROOT, "gym_amd", "csrc", "mxv_squashed.hip")
OCCUPANCY = {"squashed_kernel": {1: 8, 2: 8, 3: 7, 4: 7}, "squashed_backward_kernel": {1: 8, 2: 8, 3: 7, 4: 7}}      # as reported at the time of the change
# reported: forward 42, 48, 52, 56; backward 40, 50, 56, 61; the bound is the allocation granule (8) above each
MAX_VGPRS = {"squashed_kernel": {1: 48, 2: 48, 3: 56, 4: 56}, "squashed_backward_kernel": {1: 40, 2: 56, 3: 56, 4: 64}}
ARGS = {"squashed_kernel": "12SquashedArgs", "squashed_backward_kernel": "16SquashedGradArgs"}


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_squashed_res_")
    try:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", SRC,
                            "-o", os.path.join(d, "k.o"), "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        yield p.stderr
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _symbol(kernel, d):
    return f"_ZN12_GLOBAL__N_1{len(kernel)}{kernel}ILi{d}EEEvNS_{ARGS[kernel]}E"


def test_every_instantiation_stays_in_registers(remarks):
    from gym_amd.squashed import MAX_ACTION_DIM

    res = {k: r for k, r in _resources(remarks).items() if "squashed" in k and "kernel" in k}
    assert sorted(res) == sorted(_symbol(k, d) for k in OCCUPANCY for d in OCCUPANCY[k])
    for kernel in OCCUPANCY:
        assert sorted(OCCUPANCY[kernel]) == list(range(1, MAX_ACTION_DIM + 1))
        for d in OCCUPANCY[kernel]:
            r = res[_symbol(kernel, d)]
            print(kernel, d, r)
            assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0 and r["AGPRs"] == 0, (kernel, d, r)
            assert r["Occupancy"] >= OCCUPANCY[kernel][d] and r["VGPRs"] <= MAX_VGPRS[kernel][d], (kernel, d, r)


def test_the_source_uses_no_lds_atomics_or_assembly():
    src = re.sub(r"//.*", "", open(SRC).read())
    for word in ("__shared__", "atomic", "asm"):
        assert word not in src, word
    assert src.count("__attribute__((noinline))") == 3      # the Box-Muller pair, one dim forwards, one dim backwards
