"""Resource budget of gym_amd/csrc/mxv_c51.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

Every kernel — c51_rows, c51_leaf, c51_tree, c51_bwd, c51_q — keeps everything in registers: no scratch, no spilled vector or scalar
register, no AGPRs, and at least the occupancy and at most the vector registers (rounded up to the allocation granule of 8) the compiler
reported when the kernels were written (DESIGN.md §20 records the figures).  The only LDS is the four-wave combine — 4 waves x 8 values
x 8 bytes — in the two kernels that reduce over rows; the kernels that own a row per wave have none.  Read from the compiler's
resource report of the code object only.  Also: the source includes the shared rule, the shared sum tree and the host checks and
defines no copy of them, no EXP or LOG of its own, and has no read-modify-write memory operation, no assembly and no shuffle."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT
from policy_host import RULE_NAMES
from test_policy_eval_resources import HIPCC, _resources

CSRC = os.path.join(ROOT, "gym_amd", "csrc")
SRC = os.path.join(CSRC, "mxv_c51.hip")
COMBINE_LDS = 4 * 8 * 8
TREE = os.path.join(CSRC, "mxv_sum_tree.hpp")
# what only mxv_sum_tree.hpp defines: no file that includes it keeps a copy (tests/test_ppo_resources.py, test_dqn_resources.py and the
# normalisation kernels' test in test_kernel_resources.py use the same list)
TREE_COPIES = (r"\bwave_tree\s*\(double", r"\bwave_tree_sum\b", r"struct\s+(Add|Min|Max)\b", r"\bdpp_f64\s*\(double", r"\bgroup_value\s*\(const",
               r"\bleaves_of\s*\(int64_t", r"\bint\s+run_tree\s*\(const", r"\bkLeafRows\s*=", r"\bkTreeFan\s*=", r"permlane\d+_swap")
TREE_BARRIER_HELPERS = ("leave_wave_values(", "fold_level<")      # each ends in the one barrier of the kernel that calls it
VALUE = os.path.join(CSRC, "mxv_value_loss.hpp")
# what only mxv_value_loss.hpp defines: none of mxv_dqn.hip, mxv_c51.hip and mxv_qr.hip keeps a copy (their tests use the same list)
VALUE_COPIES = (r"struct\s+TreeArgs\b", r"struct\s+LeafArgs\b", r"struct\s+Partials\b", r"\bgrid_rows\s*\(int64_t", r"\bint64_t\s+tile_of_block\s*\(",
                r"\bint\s+wave_of_block\s*\(", r"\bvoid\s+finish\s*\(", r"\bint\s+launch_rows\s*\(", r"\bworkspace_doubles\s*\(int64_t",
                r"\bkGridX\s*=", r"\bkGridY\s*=", r"\bkWaves\s*=", r"\bkV\s*=", r"\bkCols\s*=", r"four_waves<", r"exactly one target mode")
VALUE_BARRIER_HELPERS = ("leaf_columns(", "tree_level(")      # each calls one of TREE_BARRIER_HELPERS once: the one barrier of its kernel


def tree_header():
    """mxv_sum_tree.hpp without its comments: no read-modify-write memory operation, no assembly, no shuffle, and one barrier in each of the
    two helpers that leave the waves' values in LDS."""
    tree = re.sub(r"//.*", "", open(TREE).read())
    for word in ("atomic", "asm", "__shfl", "#if MXV_"):
        assert word not in tree, word
    assert tree.count("__syncthreads()") == len(TREE_BARRIER_HELPERS) and "__shared__" not in tree
    for helper in ("void leave_wave_values(", "void fold_level("):
        body = tree[tree.index(helper):]
        assert body[:body.index("\n}\n")].rstrip().endswith("__syncthreads();"), helper
    return tree


def value_header():
    """mxv_value_loss.hpp without its comments: it shares the tree and the rule's limits and defines no copy of them; no read-modify-write
    memory operation, no assembly, no shuffle, no LDS and no barrier of its own — its two bodies take the kernel's LDS and each calls one
    helper of mxv_sum_tree.hpp that ends in the barrier."""
    value = re.sub(r"//.*", "", open(VALUE).read())
    assert '#include "mxv_sum_tree.hpp"' in value and '#include "mxv_policy_rule.hpp"' in value
    for word in ("atomic", "asm", "__shfl", "#if MXV_", "__shared__", "__syncthreads", "__global__"):
        assert word not in value, word
    for copy in (r"\bkThreads\s*=", r"\bkMaxActions\s*=", r"\bkMaxElems\s*=") + TREE_COPIES:
        assert not re.search(copy, value), copy
    for copy in VALUE_COPIES[:-2]:      # (the last two are uses, not definitions)
        assert len(re.findall(copy, value)) == 1, copy
    for helper, calls in (("void leaf_columns(", "leave_wave_values("), ("void tree_level(", "fold_level<Partials>(")):
        body = value[value.index(helper):]
        body = body[:body.index("\n}\n")]
        assert sum(body.count(h) for h in TREE_BARRIER_HELPERS) == 1 and calls in body, helper
        assert "write_partials<Partials>(" in body and "finish(sm, " in body, helper
    assert "run_tree(" in value and "kMaxActions" in value and "kMaxElems" in value and "check_stride" not in value
    return value


def barriers(src):
    """Barriers of a kernel source: its own, and one for every call of a helper of mxv_sum_tree.hpp or of mxv_value_loss.hpp that ends in one."""
    return src.count("__syncthreads()") + sum(src.count(h) for h in TREE_BARRIER_HELPERS + VALUE_BARRIER_HELPERS)


# symbol: (waves per SIMD, VGPR bound, LDS bytes) as reported at the time of the change; reported VGPRs in the comments
BUDGET = {
    "_ZN12_GLOBAL__N_18c51_rowsENS_7C51ArgsE": (8, 40, 0),               # 38
    "_ZN12_GLOBAL__N_18c51_leafEN3mxv10value_loss8LeafArgsE": (8, 48, COMBINE_LDS),    # 45
    "_ZN12_GLOBAL__N_18c51_treeEN3mxv10value_loss8TreeArgsE": (8, 48, COMBINE_LDS),    # 45
    "_ZN12_GLOBAL__N_17c51_bwdENS_7C51ArgsE": (8, 32, 0),                # 30
    "_ZN12_GLOBAL__N_15c51_qENS_7C51ArgsE": (8, 24, 0),                  # 22
}


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_c51_res_")
    try:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", SRC,
                            "-o", os.path.join(d, "k.o"), "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        yield p.stderr
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_every_kernel_stays_in_registers_and_the_only_lds_is_the_combine(remarks):
    res = _resources(remarks)
    assert sorted(res) == sorted(BUDGET)
    for kernel, (occupancy, vgprs, lds) in BUDGET.items():
        r = res[kernel]
        print(kernel, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (kernel, r)
        assert r["LDS Size"] == lds, (kernel, r)
        assert r["Occupancy"] >= occupancy and r["VGPRs"] <= vgprs, (kernel, r)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 20."):]
    for name in ("c51_rows", "c51_leaf", "c51_tree", "c51_bwd", "c51_q"):      # the table of §20: VGPRs, SGPRs, waves / SIMD, LDS bytes
        row = re.search(rf"\| `{name}` \| \d+ \| \d+ \| (\d+) \| (\d+) \| 0 \|", section)
        assert row, name
        r = next(v for k, v in res.items() if f"{name}E" in k)
        assert (r["Occupancy"], r["LDS Size"]) == tuple(int(x) for x in row.groups()), (name, r, row.groups())


def test_the_source_shares_the_rule_the_tree_and_the_host_checks():
    src = re.sub(r"//.*", "", open(SRC).read())
    for header in ("mxv_policy_rule.hpp", "mxv_policy_host.hpp", "mxv_sum_tree.hpp", "mxv_value_loss.hpp"):
        assert f'#include "{header}"' in src, header
    value = value_header()      # the limits of a batch and the levels of the tree are used there
    assert "kThreads" in src and "kMaxActions" in value
    assert "Call<mxv::C51Call>" in src and "check_ranges(" in src and "check_stride(" in src
    assert "check_batch(" in src and "check_targets(" in src and "sum_columns(" in src and "static_assert(MXV_C51_STATS == kV" in src
    for copy in (r"\bkThreads\s*=", r"\bkMaxActions\s*=", r"\bkMaxElems\s*=", r"\bkMaxBlocks\s*=", r"struct\s+Range\b", r"\bint\s+check_ranges\b",
                 r"\bdouble\s+(exp_rule|log_rule|e_of)\b", r"\b(exp|log|expf|logf|__expf|__logf)\s*\(") + TREE_COPIES + VALUE_COPIES:
        assert not re.search(copy, src), copy
    assert not RULE_NAMES.search(src)      # none of the rule's constants is defined here
    assert "e_of(" in src and "log_rule(" in src
    # the only atomics would be on integer types: there is none at all, no assembly and no shuffle
    for word in ("atomic", "asm", "__shfl", "#if MXV_"):
        assert word not in src, word
    tree_header()
    # one combine in each of the two kernels that reduce over rows
    assert src.count("__shared__") == 2 and barriers(src) == 2
    for script in ("build.sh", "build_asan.sh"):
        assert "mxv_c51.hip" in open(os.path.join(CSRC, script)).read(), script
    flags = open(os.path.join(CSRC, "build.sh")).read()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-ffast-math" not in flags
    host = open(os.path.join(CSRC, "mxv_policy_host.hpp")).read()
    assert "struct C51Call {" in host and "struct DqnCall {" in host


def test_the_launch_constants_the_module_exports_are_the_kernels():
    from gym_amd import c51, dqn, ppo

    src, value = open(SRC).read(), open(VALUE).read()
    rule = open(os.path.join(CSRC, "mxv_policy_rule.hpp")).read()
    tree = open(TREE).read()
    assert f"constexpr int kLeafRows = {c51.LEAF_ROWS};" in tree and f"constexpr int kTreeFan = {c51.LEAF_ROWS};" in tree
    assert ppo.LEAF_ROWS == dqn.LEAF_ROWS == c51.LEAF_ROWS      # the one tree of the three losses
    assert f"constexpr int kGridX = 1 << {c51.GRID_X.bit_length() - 1};" in value and c51.GRID_X & (c51.GRID_X - 1) == 0
    assert "constexpr int kWaves = kThreads / 64;" in value and f"constexpr int kThreads = {64 * c51.TILE_ROWS};" in rule
    assert f"constexpr int kMaxBlocks = {c51.MAX_BLOCKS};" in rule and f"constexpr int kMaxAtoms = {c51.MAX_ATOMS};" in src
