"""Resource budget of gym_amd/csrc/mxv_subnorm.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

Exactly twelve kernels: subnorm_obs_kernel<D, OUT> for D in 1, 2, 3, 4, 6 and OUT in float, double, and subnorm_rew_kernel<RT> for float
and double.  Each keeps its statistics in registers — no scratch, no spilled vector or scalar register — at an occupancy not below the one
the build reported before this test existed (waves per SIMD, from the compiler's kernel-resource-usage remarks):

    observation, D = 1          8
    observation, D = 2          8
    observation, D = 3          7
    observation, D = 4          5
    observation, D = 6          4
    reward, both dtypes         8

The kernel file's header says that 6 waves change nothing for D = 4 and that 8 spill: a change that trades registers for occupancy, or the
other way, shows here.  The test reads the remarks only."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "gym_amd", "csrc", "mxv_subnorm.hip")
OBS_WAVES = {1: 8, 2: 8, 3: 7, 4: 5, 6: 4}
REW_WAVES = 8


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_subnorm_res_")
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
        m = re.search(r"remark: +(?:\S+:\d+:\d+: +)?(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None:
            cur[k.split(" [")[0]] = int(v)
    return out


def _obs(D, out):
    return f"_ZN12_GLOBAL__N_118subnorm_obs_kernelILi{D}E{out}EEvNS_10SubObsArgsE"


def _rew(rt):
    return f"_ZN12_GLOBAL__N_118subnorm_rew_kernelI{rt}EEvNS_10SubRewArgsE"


def test_the_twelve_kernels_hold_their_statistics_in_registers_at_the_recorded_occupancy(remarks):
    res = _resources(remarks)
    want = {_obs(D, o): w for D, w in OBS_WAVES.items() for o in "fd"}
    want.update({_rew(rt): REW_WAVES for rt in "fd"})
    assert len(want) == 12 and sorted(k for k in res if "subnorm_" in k) == sorted(want)
    for sym, waves in want.items():
        r = res[sym]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, (sym, r)
        assert r["Occupancy"] >= waves, (sym, r)
