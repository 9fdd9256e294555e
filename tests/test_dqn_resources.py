"""Resource budget of gym_amd/csrc/mxv_dqn.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

Every kernel — the five instantiations of dqn_leaf and of dqn_bwd (A = 2, 3, 4, 6 straight-line, 0 = the loops) and dqn_tree — keeps
everything in registers: no scratch, no spilled vector or scalar register, no AGPRs, and at least the occupancy and at most the vector
registers (rounded up to the allocation granule of 8) the compiler reported when the kernels were written (DESIGN.md §17 records the
figures).  The only LDS is the four-wave combine — 4 waves x 8 values x 8 bytes in the kernels that reduce — and the backward's staging
of the loop instantiation: one float and one column index per row of a tile, 256 x 8 bytes; the straight-line backward has none.  Read
from the compiler's resource report of the code object only.  Also: the source includes the shared rule, the shared sum tree and the host
checks and defines no copy of them, and neither it nor the tree has a read-modify-write memory operation, assembly or a shuffle."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT
from test_c51_resources import TREE_COPIES, VALUE_COPIES, barriers, tree_header, value_header
from test_policy_eval_resources import HIPCC, _resources

SRC = os.path.join(ROOT, "gym_amd", "csrc", "mxv_dqn.hip")
COMBINE_LDS = 4 * 8 * 8
STAGING_LDS = 256 * (4 + 4)
LEAF, BWD = "_ZN12_GLOBAL__N_18dqn_leafILi%dEEEvNS_7DqnArgsE", "_ZN12_GLOBAL__N_17dqn_bwdILi%dEEEvNS_7DqnArgsE"
# symbol: (waves per SIMD, VGPR bound, LDS bytes) as reported at the time of the change; reported VGPRs in the comments
BUDGET = {
    LEAF % 2: (8, 40, COMBINE_LDS),                                   # 34
    LEAF % 3: (8, 40, COMBINE_LDS),                                   # 34
    LEAF % 4: (8, 40, COMBINE_LDS),                                   # 34
    LEAF % 6: (8, 40, COMBINE_LDS),                                   # 34
    LEAF % 0: (8, 40, COMBINE_LDS),                                   # 34
    "_ZN12_GLOBAL__N_18dqn_treeEN3mxv10value_loss8TreeArgsE": (8, 48, COMBINE_LDS),  # 45
    BWD % 2: (8, 32, 0),                                              # 26
    BWD % 3: (8, 32, 0),                                              # 28
    BWD % 4: (8, 32, 0),                                              # 30
    BWD % 6: (8, 32, 0),                                              # 32
    BWD % 0: (8, 32, STAGING_LDS),                                    # 26
}


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_dqn_res_")
    try:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", SRC,
                            "-o", os.path.join(d, "k.o"), "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        yield p.stderr
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_every_kernel_stays_in_registers_and_the_lds_is_the_combine_and_the_staging(remarks):
    res = _resources(remarks)
    assert sorted(res) == sorted(BUDGET)
    for kernel, (occupancy, vgprs, lds) in BUDGET.items():
        r = res[kernel]
        print(kernel, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (kernel, r)
        assert r["LDS Size"] == lds, (kernel, r)
        assert r["Occupancy"] >= occupancy and r["VGPRs"] <= vgprs, (kernel, r)


def test_the_source_shares_the_rule_and_the_host_checks():
    src = re.sub(r"//.*", "", open(SRC).read())
    value = value_header()      # the limits of a batch and the levels of the tree are used there
    assert '#include "mxv_policy_rule.hpp"' in src and '#include "mxv_policy_host.hpp"' in src and "kThreads" in src and "kMaxActions" in value
    assert '#include "mxv_sum_tree.hpp"' in src and "wave_tree<" in src and "run_tree(" in value
    assert '#include "mxv_value_loss.hpp"' in src and "check_batch(" in src and "check_targets(" in src and "finish_tree(" in src
    assert "write_partials<Partials>(" in src and "static_assert(MXV_DQN_STATS == kV" in src      # its own leaf writes the shared partials
    assert "Call<mxv::DqnCall>" in src and "check_ranges(" in src and "check_stride(" in src
    for copy in (r"\bkThreads\s*=", r"\bkMaxActions\s*=", r"\bkMaxElems\s*=", r"\bkMaxBlocks\s*=", r"struct\s+Range\b", r"\bint\s+check_ranges\b") + TREE_COPIES + VALUE_COPIES:
        assert not re.search(copy, src), copy
    for word in ("atomic", "asm", "__shfl"):
        assert word not in src, word
    tree_header()      # nor has the shared tree any of them
    # one combine in each of the two kernels that reduce, and the two staging arrays of the loop backward between its two barriers
    assert src.count("__shared__") == 4 and barriers(src) == 4
    for script in ("build.sh", "build_asan.sh"):
        assert "mxv_dqn.hip" in open(os.path.join(ROOT, "gym_amd", "csrc", script)).read(), script
    flags = open(os.path.join(ROOT, "gym_amd", "csrc", "build.sh")).read()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-ffast-math" not in flags
    host = open(os.path.join(ROOT, "gym_amd", "csrc", "mxv_policy_host.hpp")).read()
    assert "struct DqnCall {" in host and "struct VtraceCall {" in host
