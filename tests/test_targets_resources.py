"""Resource budget of gym_amd/csrc/mxv_targets.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

Every kernel — targets_dqn, targets_c51, targets_qr — keeps everything in registers: no scratch, no spilled vector or scalar register,
no AGPRs, no LDS, and at least the occupancy and at most the vector registers (rounded up to the allocation granule of 8) and the scalar
registers (rounded up to their granule of 16) the compiler reported when the kernels were written (DESIGN.md §24 records the figures).
Read from the compiler's resource report of the code object only.  Also: the source includes the shared rule, the shared sum tree and
the host checks and defines no copy of them, no EXP of its own, and has no read-modify-write memory operation, no assembly, no shuffle,
no LDS and no barrier."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT
from policy_host import RULE_NAMES
from test_c51_resources import TREE_COPIES, VALUE, VALUE_COPIES, barriers, value_header
from test_policy_eval_resources import HIPCC, _resources

CSRC = os.path.join(ROOT, "gym_amd", "csrc")
SRC = os.path.join(CSRC, "mxv_targets.hip")
KERNELS = ("targets_dqn", "targets_c51", "targets_qr")

# symbol: (waves per SIMD, VGPR bound, SGPR bound) as reported at the time of the change; reported VGPRs and SGPRs in the comments
BUDGET = {
    "_ZN12_GLOBAL__N_111targets_dqnENS_11TargetsArgsE": (8, 24, 48),      # 17, 48
    "_ZN12_GLOBAL__N_111targets_c51ENS_11TargetsArgsE": (8, 24, 80),      # 24, 80
    "_ZN12_GLOBAL__N_110targets_qrENS_11TargetsArgsE": (8, 16, 48),       # 16, 36
}


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_targets_res_")
    try:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", SRC,
                            "-o", os.path.join(d, "k.o"), "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        yield p.stderr
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _sgprs(text):
    """{symbol: TotalSGPRs} of the resource report."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: +(Function Name|TotalSGPRs): (\S+)", line)
        if m and m.group(1) == "Function Name":
            cur = m.group(2)
        elif m and cur is not None:
            out[cur] = int(m.group(2))
    return out


def test_every_kernel_stays_in_registers_and_has_no_lds(remarks):
    res, sgprs = _resources(remarks), _sgprs(remarks)
    assert sorted(res) == sorted(BUDGET) == sorted(sgprs)
    for kernel, (occupancy, vgprs, sbound) in BUDGET.items():
        r = res[kernel]
        print(kernel, r, sgprs[kernel])
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (kernel, r)
        assert r["LDS Size"] == 0, (kernel, r)
        assert r["Occupancy"] >= occupancy and r["VGPRs"] <= vgprs and sgprs[kernel] <= sbound, (kernel, r, sgprs[kernel])
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 24."):]
    for name in KERNELS:      # the table of §24: | kernel | VGPRs | SGPRs | waves/SIMD | LDS | scratch |
        row = re.search(rf"\| `{name}` \| (\d+) \| (\d+) \| (\d+) \| 0 \| 0 \|", section)
        assert row, name
        key = next(k for k in res if f"{name}E" in k)
        assert (res[key]["VGPRs"], sgprs[key], res[key]["Occupancy"]) == tuple(int(x) for x in row.groups()), (name, res[key], sgprs[key], row.groups())


def test_the_source_shares_the_rule_the_tree_and_the_host_checks():
    src = re.sub(r"//.*", "", open(SRC).read())
    for header in ("mxv_policy_rule.hpp", "mxv_policy_host.hpp", "mxv_sum_tree.hpp", "mxv_value_loss.hpp"):
        assert f'#include "{header}"' in src, header
    value = value_header()
    assert "kThreads" in src and "kMaxBlocks" not in src      # targets_dqn strides through Call::launch's grid_of
    assert "Call<mxv::TargetsCall>" in src and "check_ranges(" in src and "check_stride(" in src and "check_counts(" in src
    assert "launch_rows(" in src and "grid_rows(" in value and "ArgNames" in src and "tile_of_block()" in src and "wave_of_block()" in src
    for copy in (r"\bkThreads\s*=", r"\bkMaxActions\s*=", r"\bkMaxElems\s*=", r"\bkMaxBlocks\s*=", r"struct\s+Range\b", r"\bint\s+check_ranges\b",
                 r"\bint\s+check_counts\b", r"struct\s+ArgNames\b", r"\bdouble\s+(exp_rule|log_rule|e_of)\b",
                 r"\b(exp|log|expf|logf|__expf|__logf)\s*\(") + TREE_COPIES + VALUE_COPIES:
        assert not re.search(copy, src), copy
    assert not RULE_NAMES.search(src)      # none of the rule's constants is defined here
    assert "wave_tree<Add>(" in src and "wave_tree<Max>(" in src and "lane_value(" in src and "e_of(" in src
    for word in ("atomic", "asm", "__shfl", "#if MXV_", "__shared__", "hipMalloc", "Synchronize"):
        assert word not in src, word
    assert barriers(src) == 0
    assert sorted(re.findall(r"__global__ void __launch_bounds__\(kThreads\) (\w+)\(", src)) == sorted(KERNELS)
    for script in ("build.sh", "build_asan.sh"):
        assert "mxv_targets.hip" in open(os.path.join(CSRC, script)).read(), script
    host = open(os.path.join(CSRC, "mxv_policy_host.hpp")).read()
    assert "struct TargetsCall {" in host and "struct QrCall {" in host


def test_the_launch_constants_the_module_exports_are_the_kernels():
    from gym_amd import c51, targets

    src, value = open(SRC).read(), open(VALUE).read()
    rule = open(os.path.join(CSRC, "mxv_policy_rule.hpp")).read()
    assert (targets.TILE_ROWS, targets.GRID_X, targets.MAX_BLOCKS) == (c51.TILE_ROWS, c51.GRID_X, c51.MAX_BLOCKS)
    assert f"constexpr int kGridX = 1 << {targets.GRID_X.bit_length() - 1};" in value
    assert "constexpr int kWaves = kThreads / 64;" in value and f"constexpr int kThreads = {targets.LANE_ROWS};" in rule
    assert targets.LANE_ROWS == 64 * targets.TILE_ROWS and f"constexpr int kMaxBlocks = {targets.MAX_BLOCKS};" in rule
    assert f"constexpr int kMaxAtoms = {targets.MAX_ATOMS};" in src and f"constexpr int kMaxQuantiles = {targets.MAX_QUANTILES};" in src
