"""Resource budget of gym_amd/csrc/mxv_nstep.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

Every kernel — the five instantiations of nstep_insert_rows (W = 2, 3, 4, 6 straight-line, 0 = the loop), the two of nstep_insert_wide
(16-byte pieces, dwords) and nstep_gather_rows — keeps everything in registers: no scratch, no spilled vector or scalar register, no
AGPRs, no LDS, and at least the occupancy and at most the vector registers (rounded up to the allocation granule of 8) the compiler
reported when the kernels were written (DESIGN.md §22 records the figures).  Read from the compiler's resource report of the code object
only.  Also: the source includes the shared rule, host checks and row copiers and defines no copy of them, and has no read-modify-write
memory operation, no assembly, no shuffle, no LDS and no barrier."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT
from test_policy_eval_resources import HIPCC, _resources

SRC = os.path.join(ROOT, "gym_amd", "csrc", "mxv_nstep.hip")
INSERT_ROWS, INSERT_WIDE = "_ZN12_GLOBAL__N_117nstep_insert_rowsILi%dEEEvNS_9NStepArgsE", "_ZN12_GLOBAL__N_117nstep_insert_wideILb%dEEEvNS_9NStepArgsE"
GATHER = "_ZN12_GLOBAL__N_117nstep_gather_rowsENS_10GatherArgsE"
# symbol: (waves per SIMD, VGPR bound) as reported at the time of the change; reported VGPRs in the comments
BUDGET = {
    INSERT_ROWS % 0: (8, 32),   # 28
    INSERT_ROWS % 2: (8, 32),   # 26
    INSERT_ROWS % 3: (8, 32),   # 27
    INSERT_ROWS % 4: (8, 32),   # 26
    INSERT_ROWS % 6: (8, 32),   # 32
    INSERT_WIDE % 1: (8, 24),   # 24
    INSERT_WIDE % 0: (8, 24),   # 23
    GATHER: (8, 16),            # 12
}


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_nstep_res_")
    try:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", SRC,
                            "-o", os.path.join(d, "k.o"), "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        yield p.stderr
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_every_kernel_stays_in_registers_and_uses_no_lds(remarks):
    res = _resources(remarks)
    assert sorted(res) == sorted(BUDGET)
    for kernel, (occupancy, vgprs) in BUDGET.items():
        r = res[kernel]
        print(kernel, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0 and r["LDS Size"] == 0, (kernel, r)
        assert r["Occupancy"] >= occupancy and r["VGPRs"] <= vgprs, (kernel, r)


def test_the_source_shares_the_rule_the_host_checks_and_the_row_copiers():
    src = re.sub(r"//.*", "", open(SRC).read())
    for include in ('#include "mxv_policy_rule.hpp"', '#include "mxv_policy_host.hpp"', '#include "mxv_replay_rows.hpp"', '#include "../../include/mxv_nstep.h"'):
        assert include in src, include
    assert "kThreads" in src and "kMaxElems" in src and "Call<mxv::NStepCall>" in src and "check_ranges(" in src and "check_stride(" in src
    for shared in ("copy_rows<WT>(", "copy_pieces<VEC>(", "Aligned al{wanted_alignment(W)}", "launch_wide(call,", "kNarrow"):
        assert shared in src, shared
    for copy in (r"\bkThreads\s*=", r"\bkMaxElems\s*=", r"\bkMaxBlocks\s*=", r"struct\s+Range\b", r"\bint\s+check_ranges\b", r"\bkNarrow\s*=", r"\bkPiece\s*=",
                 r"\bkWideRows\s*=", r"\bvoid\s+copy_rows\b", r"\bvoid\s+copy_pieces\b", r"struct\s+Aligned\b", r"\bwanted_alignment\s*\([^)]*\)\s*\{",
                 r"\bint\s+launch_wide\b", r"add_word_kernel"):
        assert not re.search(copy, src), copy
    for word in ("atomic", "asm", "__shfl", "__shared__", "__syncthreads"):
        assert word not in src, word
    # the cut is a branch of the walk, and the return is accumulated in float64 one operation at a time
    assert "&& !done)" in src and "g = g * p.gamma;" in src and "G = G + g * reward_of(p, re);" in src and "fma" not in src
    # the device row counter is advanced by the existing one-thread kernel, nowhere else
    assert src.count("launch_add_word(") == 1
    for script in ("build.sh", "build_asan.sh"):
        assert "mxv_nstep.hip" in open(os.path.join(ROOT, "gym_amd", "csrc", script)).read(), script
    flags = open(os.path.join(ROOT, "gym_amd", "csrc", "build.sh")).read()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-ffast-math" not in flags
    host = open(os.path.join(ROOT, "gym_amd", "csrc", "mxv_policy_host.hpp")).read()
    assert "struct NStepCall {" in host and "struct ReplayCall {" in host
    # the one-step buffers' sources are as they were: the n-step kernels are this file's own
    for other in ("mxv_replay.hip", "mxv_prio.hip"):
        assert "nstep" not in open(os.path.join(ROOT, "gym_amd", "csrc", other)).read(), other
