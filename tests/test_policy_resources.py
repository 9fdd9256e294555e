"""Resource budget of gym_amd/csrc/mxv_policy.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

All five instantiations of policy_kernel — the straight-line ones for A = 2, 3, 4, 6 and the loop for any A — keep everything in
registers: no scratch, no spilled vector register, no LDS, and at most 64 VGPRs, i.e. the 7 waves per SIMD the kernel is meant to run at (the
arithmetic hides the one load of a lane; what caps the occupancy is the scalar registers).  Read from the compiler's resource report
of the code object only."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "gym_amd", "csrc", "mxv_policy.hip")
INSTANCES = (0, 2, 3, 4, 6)


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_policy_res_")
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


def _symbol(a):
    return f"_ZN12_GLOBAL__N_113policy_kernelILi{a}EEEvNS_10PolicyArgsE"


def test_every_instantiation_stays_in_registers(remarks):
    from gym_amd.policy import STRAIGHT_LINE_ACTIONS

    assert tuple(a for a in INSTANCES if a) == STRAIGHT_LINE_ACTIONS
    res = {k: r for k, r in _resources(remarks).items() if "policy_kernel" in k}
    assert sorted(res) == sorted(_symbol(a) for a in INSTANCES)
    for a in INSTANCES:
        r = res[_symbol(a)]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["LDS Size"] == 0 and r["AGPRs"] == 0, (a, r)
        assert r["VGPRs"] <= 64 and r["Occupancy"] >= 7, (a, r)
