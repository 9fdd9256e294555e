"""Resource budget of gym_amd/csrc/mxv_ppo.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

Every kernel — ppo_leaf, moments_leaf, the two instantiations of ppo_tree, ppo_bwd — keeps everything in registers: no scratch, no spilled
vector or scalar register, no AGPRs, and at least the occupancy and at most the vector registers (rounded up to the allocation granule
of 8) the compiler reported when the kernels were written (DESIGN.md §15 records the figures).  The only LDS is the four-wave combine:
4 waves x 8 values x 8 bytes in the kernels that reduce, none in the backward.  Read from the compiler's resource report of the code
object only.  Also: the source includes the shared rule and the shared sum tree and defines no copy of them, and neither it nor the tree
uses atomics or assembly."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT
from test_c51_resources import TREE_COPIES, barriers, tree_header
from test_policy_eval_resources import HIPCC, _resources

SRC = os.path.join(ROOT, "gym_amd", "csrc", "mxv_ppo.hip")
COMBINE_LDS = 4 * 8 * 8
# symbol: (waves per SIMD, VGPR bound, LDS bytes) as reported at the time of the change; reported VGPRs in the comments
BUDGET = {
    "_ZN12_GLOBAL__N_18ppo_leafENS_7PpoArgsE": (8, 32, COMBINE_LDS),               # 32
    "_ZN12_GLOBAL__N_112moments_leafENS_11MomentsArgsE": (8, 16, COMBINE_LDS),     # 12
    "_ZN12_GLOBAL__N_18ppo_treeILb1EEEvNS_8TreeArgsE": (8, 40, COMBINE_LDS),       # 38
    "_ZN12_GLOBAL__N_18ppo_treeILb0EEEvNS_8TreeArgsE": (8, 24, COMBINE_LDS),       # 22
    "_ZN12_GLOBAL__N_17ppo_bwdENS_7PpoArgsE": (8, 32, 0),                          # 27
}


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_ppo_res_")
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
        assert r["LDS Size"] == lds <= COMBINE_LDS, (kernel, r)
        assert r["Occupancy"] >= occupancy and r["VGPRs"] <= vgprs, (kernel, r)


def test_the_source_shares_the_rule_and_uses_no_atomics_or_assembly():
    src = re.sub(r"//.*", "", open(SRC).read())
    assert '#include "mxv_policy_rule.hpp"' in src and "exp_rule(" in src and "kThreads" in src
    assert '#include "mxv_sum_tree.hpp"' in src and "wave_tree<" in src and "run_tree(" in src
    for copy in (r"\bexp_rule\s*\(\s*double", r"\bkThreads\s*=", r"\bkExpC\b", r"\bkInvLn2\b", r"\bkMaxElems\s*=") + TREE_COPIES:
        assert not re.search(copy, src), copy
    for word in ("atomic", "asm", "__shfl"):
        assert word not in src, word
    tree_header()      # nor has the shared tree any of them
    assert src.count("__shared__") == 3 and barriers(src) == 3      # one combine in each kernel that reduces
    for script in ("build.sh", "build_asan.sh"):
        assert "mxv_ppo.hip" in open(os.path.join(ROOT, "gym_amd", "csrc", script)).read(), script
    flags = open(os.path.join(ROOT, "gym_amd", "csrc", "build.sh")).read()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-ffast-math" not in flags
