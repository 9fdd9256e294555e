"""Resource budget of gym_amd/csrc/mxv_policy_eval.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

Every instantiation of the four kernels — eval_cat_fwd / eval_cat_bwd for A = 2, 3, 4, 6 and the loop (0), eval_gauss_fwd / eval_gauss_bwd
for D = 1, 2, 3, 4 — keeps everything in registers: no scratch, no spilled vector or scalar register, no LDS, no AGPRs, and at least the
occupancy and at most the vector registers (rounded up to the allocation granule of 8) the compiler reported when the kernels were
written (DESIGN.md §14 records the figures).  The report of a kernel includes the out-of-line LOG it calls.  Read from the compiler's
resource report of the code object only."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "gym_amd", "csrc", "mxv_policy_eval.hip")
# (waves per SIMD, VGPR bound) as reported at the time of the change; reported VGPRs in the comments
BUDGET = {
    "eval_cat_fwd": {2: (8, 40), 3: (8, 40), 4: (8, 48), 6: (8, 56), 0: (8, 32)},        # 33, 37, 41, 50, 30
    "eval_cat_bwd": {2: (7, 48), 3: (7, 56), 4: (7, 64), 6: (7, 72), 0: (8, 40)},        # 42, 51, 62, 68, 40
    "eval_gauss_fwd": {1: (8, 32), 2: (8, 40), 3: (8, 40), 4: (8, 48)},                  # 26, 33, 37, 41
    "eval_gauss_bwd": {1: (8, 32), 2: (8, 40), 3: (8, 48), 4: (8, 56)},                  # 32, 38, 44, 50
}


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_policy_eval_res_")
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


def _symbol(kernel, n):
    args = "7CatArgs" if "cat" in kernel else "9GaussArgs"
    return f"_ZN12_GLOBAL__N_1{len(kernel)}{kernel}ILi{n}EEEvNS_{args}E"


def test_every_instantiation_stays_in_registers(remarks):
    from gym_amd.policy_eval import MAX_ACTION_DIM, STRAIGHT_LINE_ACTIONS

    assert sorted(BUDGET["eval_cat_fwd"]) == sorted(BUDGET["eval_cat_bwd"]) == sorted(STRAIGHT_LINE_ACTIONS + (0,))
    assert sorted(BUDGET["eval_gauss_fwd"]) == sorted(BUDGET["eval_gauss_bwd"]) == list(range(1, MAX_ACTION_DIM + 1))
    res = _resources(remarks)
    kernels = {k: r for k, r in res.items() if "eval_" in k}
    assert sorted(kernels) == sorted(_symbol(k, n) for k, per in BUDGET.items() for n in per)
    # benchmarks and the other resource tests select the samplers' kernels by these names
    assert not [k for k in res if "policy_kernel" in k or "gaussian_kernel" in k]
    for kernel, per in BUDGET.items():
        for n, (occupancy, vgprs) in per.items():
            r = kernels[_symbol(kernel, n)]
            print(kernel, n, r)
            assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0 and r["AGPRs"] == 0, (kernel, n, r)
            assert r["Occupancy"] >= occupancy and r["VGPRs"] <= vgprs, (kernel, n, r)


def test_the_source_uses_no_lds_atomics_or_assembly():
    src = re.sub(r"//.*", "", open(SRC).read())
    for word in ("__shared__", "atomic", "asm"):
        assert word not in src, word
