"""Resource budget of gym_amd/csrc/mxv_sac.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

Every kernel — the three instantiations (C = 1, 2 straight-line, 0 = the loops) of sac_targets, sac_q_leaf, sac_q_bwd, sac_pi_leaf and
sac_pi_bwd, and sac_tree — keeps everything in registers: no scratch, no spilled vector or scalar register, no AGPRs, and at least the
occupancy and at most the vector registers (rounded up to the allocation granule of 8) and the scalar registers (rounded up to their
granule of 16) the compiler reported when the kernels were written; DESIGN.md §25 records the reported figures in a table, which is
compared with the report.  The only LDS is the four-wave combine — 4 waves x 8 values x 8 bytes in the kernels that reduce — and the
staging of the two loop backwards: a float64 target and a float32 weight per row of a tile for the critics' (256 x 12 bytes), a float and
a column index for the actor's (256 x 8 bytes); the straight-line backwards and the targets have none.  Read from the compiler's resource
report of the code object only.  Also: the source includes the shared rule, the shared sum tree, the shared value-loss core and the host
checks and defines no copy of them, no exp or log, and has no read-modify-write memory operation, assembly or shuffle."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT
from policy_host import RULE_NAMES
from test_c51_resources import TREE_COPIES, VALUE_COPIES, barriers, tree_header, value_header
from test_policy_eval_resources import HIPCC, _resources
from test_targets_resources import _sgprs

CSRC = os.path.join(ROOT, "gym_amd", "csrc")
SRC = os.path.join(CSRC, "mxv_sac.hip")
COMBINE_LDS = 4 * 8 * 8
Q_STAGING_LDS = 256 * (8 + 4)
PI_STAGING_LDS = 256 * (4 + 4)
KERNELS = ("sac_targets", "sac_q_leaf", "sac_q_bwd", "sac_pi_leaf", "sac_pi_bwd")


def _symbol(kernel, n):
    return f"_ZN12_GLOBAL__N_1{len(kernel)}{kernel}ILi{n}EEEvNS_7SacArgsE"


TREE = "_ZN12_GLOBAL__N_18sac_treeEN3mxv10value_loss8TreeArgsE"
# symbol: (waves per SIMD, VGPR bound, SGPR bound, LDS bytes) as reported at the time of the change; reported VGPRs and SGPRs in the comments
BUDGET = {
    TREE: (8, 48, 32, COMBINE_LDS),                                   # 45, 26
    _symbol("sac_targets", 1): (8, 24, 48, 0),                        # 19, 42
    _symbol("sac_targets", 2): (8, 24, 48, 0),                        # 19, 42
    _symbol("sac_targets", 0): (8, 24, 48, 0),                        # 20, 48
    _symbol("sac_q_leaf", 1): (8, 40, 64, COMBINE_LDS),               # 37, 58
    _symbol("sac_q_leaf", 2): (8, 48, 64, COMBINE_LDS),               # 48, 56
    _symbol("sac_q_leaf", 0): (8, 56, 80, COMBINE_LDS),               # 51, 70
    _symbol("sac_q_bwd", 1): (8, 24, 64, 0),                          # 24, 56
    _symbol("sac_q_bwd", 2): (8, 32, 64, 0),                          # 28, 56
    _symbol("sac_q_bwd", 0): (8, 40, 80, Q_STAGING_LDS),              # 34, 74
    _symbol("sac_pi_leaf", 1): (8, 40, 32, COMBINE_LDS),              # 34, 26
    _symbol("sac_pi_leaf", 2): (8, 40, 32, COMBINE_LDS),              # 36, 26
    _symbol("sac_pi_leaf", 0): (8, 40, 48, COMBINE_LDS),              # 36, 36
    _symbol("sac_pi_bwd", 1): (8, 24, 48, 0),                         # 19, 33
    _symbol("sac_pi_bwd", 2): (8, 24, 48, 0),                         # 20, 34
    _symbol("sac_pi_bwd", 0): (8, 24, 64, PI_STAGING_LDS),            # 24, 50
}


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_sac_res_")
    try:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", SRC,
                            "-o", os.path.join(d, "k.o"), "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        yield p.stderr
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_every_kernel_stays_in_registers_and_the_lds_is_the_combine_and_the_staging(remarks):
    from gym_amd import sac

    assert sorted(BUDGET) == sorted([TREE] + [_symbol(k, n) for k in KERNELS for n in sac.STRAIGHT_LINE_CRITICS + (0,)])
    res, sgprs = _resources(remarks), _sgprs(remarks)
    assert sorted(res) == sorted(BUDGET) == sorted(sgprs)
    for kernel, (occupancy, vgprs, sbound, lds) in BUDGET.items():
        r = res[kernel]
        print(kernel, r, sgprs[kernel])
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (kernel, r)
        assert r["LDS Size"] == lds, (kernel, r)
        assert r["Occupancy"] >= occupancy and r["VGPRs"] <= vgprs and sgprs[kernel] <= sbound, (kernel, r, sgprs[kernel])
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 25."):]
    names = {TREE: "sac_tree"}
    names.update({_symbol(k, n): f"{k}<{n}>" for k in KERNELS for n in (1, 2, 0)})
    for key, name in names.items():      # the table of §25: | kernel | VGPRs | SGPRs | waves/SIMD | LDS | scratch |
        row = re.search(rf"\| `{re.escape(name)}` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \| 0 \|", section)
        assert row, name
        assert (res[key]["VGPRs"], sgprs[key], res[key]["Occupancy"], res[key]["LDS Size"]) == tuple(int(x) for x in row.groups()), \
            (name, res[key], sgprs[key], row.groups())


def test_the_source_shares_the_rule_the_tree_and_the_host_checks():
    src = re.sub(r"//.*", "", open(SRC).read())
    for header in ("mxv_policy_rule.hpp", "mxv_policy_host.hpp", "mxv_sum_tree.hpp", "mxv_value_loss.hpp"):
        assert f'#include "{header}"' in src, header
    value = value_header()      # the limits of a batch and the levels of the tree are used there
    assert "kThreads" in src and "kMaxActions" in src and "kMaxElems" in src and "run_tree(" in value
    assert "wave_tree<Add>(" in src and "wave_tree<Max>(" in src and "wave_tree<Min>(" in src and "tree_level(sm, t)" in src
    assert "check_targets(" in src and "finish_tree(" in src and "check_workspace(" in src and "workspace_slots(" in src
    assert src.count("write_partials<Partials>(") == 2 and "static_assert(MXV_SAC_STATS == kV" in src      # its two leaves write the shared partials
    assert "Call<mxv::SacCall>" in src and "check_ranges(" in src and "check_stride(" in src and "launch_blocks(" in src
    for copy in (r"\bkThreads\s*=", r"\bkMaxActions\s*=", r"\bkMaxElems\s*=", r"\bkMaxBlocks\s*=", r"struct\s+Range\b", r"\bint\s+check_ranges\b",
                 r"\bint\s+check_targets\b", r"\bint\s+check_workspace\b", r"struct\s+ArgNames\b", r"\bdouble\s+nan64\b", r"\bfloat\s+to_f32\b",
                 r"\bdouble\s+(exp_rule|log_rule|e_of)\b", r"\b(exp|log|expf|logf|__expf|__logf)\s*\(") + TREE_COPIES + VALUE_COPIES:
        assert not re.search(copy, src), copy
    assert not RULE_NAMES.search(src)      # none of the rule's constants is defined here
    for word in ("atomic", "asm", "__shfl", "#if MXV_", "hipMalloc", "Synchronize"):
        assert word not in src, word
    tree_header()      # nor has the shared tree any of them
    # one combine in each of the three kernels that reduce, and the two staging arrays of each loop backward between its two barriers
    assert src.count("__shared__") == 3 + 2 + 2 and barriers(src) == 3 + 2 + 2
    kernels = re.findall(r"__global__ void __launch_bounds__\(kThreads\) (\w+)\(", src)
    assert sorted(kernels) == sorted(KERNELS + ("sac_tree",))
    assert "case 1: return K<1>::ptr();" in src and "case 2: return K<2>::ptr();" in src and "default: return K<0>::ptr();" in src
    for script in ("build.sh", "build_asan.sh"):
        assert "mxv_sac.hip" in open(os.path.join(CSRC, script)).read(), script
    flags = open(os.path.join(CSRC, "build.sh")).read()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-ffast-math" not in flags
    host = open(os.path.join(CSRC, "mxv_policy_host.hpp")).read()
    assert "struct SacCall {" in host and "struct TargetsCall {" in host


def test_the_launch_constants_the_module_exports_are_the_kernels():
    from gym_amd import sac
    from gym_amd._policy_args import LEAF_ROWS, MAX_ACTIONS

    rule = open(os.path.join(CSRC, "mxv_policy_rule.hpp")).read()
    tree = open(os.path.join(CSRC, "mxv_sum_tree.hpp")).read()
    assert sac.MAX_CRITICS == MAX_ACTIONS and f"constexpr int kMaxActions = {sac.MAX_CRITICS};" in rule
    assert sac.LEAF_ROWS == LEAF_ROWS and f"constexpr int kLeafRows = {sac.LEAF_ROWS};" in tree and f"constexpr int kTreeFan = {sac.LEAF_ROWS};" in tree
