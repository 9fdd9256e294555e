"""Resource budget of gym_amd/csrc/mxv_prio.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

Every kernel — prio_insert, prio_clear, prio_raise, prio_draw, the five instantiations of prio_gather_rows and the two of
prio_gather_wide — keeps everything in registers: no scratch, no spilled vector or scalar register, no AGPRs, and at least the
occupancy, at most the vector registers (rounded up to the allocation granule of 8) and exactly the LDS the compiler reported when the
kernels were written (DESIGN.md §19 records the figures).  Read from the compiler's resource report of the code object only.  Also: the
source includes the shared rule, host checks and row copiers and defines no copy of them, and every atomic in it is on an integer
type."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT
from test_policy_eval_resources import HIPCC, _resources

SRC = os.path.join(ROOT, "gym_amd", "csrc", "mxv_prio.hip")
ROWS = os.path.join(ROOT, "gym_amd", "csrc", "mxv_replay_rows.hpp")
GATHER_ROWS, GATHER_WIDE = "_ZN12_GLOBAL__N_116prio_gather_rowsILi%dEEEvNS_10SampleArgsE", "_ZN12_GLOBAL__N_116prio_gather_wideILb%dEEEvNS_10SampleArgsE"
TOP_BYTES = (1 + 16 + 256) * 8      # the three top levels of the tree in LDS
# symbol: (waves per SIMD, VGPR bound, LDS bytes) as reported at the time of the change; reported VGPRs in the comments
BUDGET = {
    "_ZN12_GLOBAL__N_111prio_insertENS_10InsertArgsE": (8, 40, TOP_BYTES),   # 37
    "_ZN12_GLOBAL__N_110prio_clearENS_10UpdateArgsE": (8, 16, 0),            # 12
    "_ZN12_GLOBAL__N_110prio_raiseENS_10UpdateArgsE": (8, 32, TOP_BYTES),    # 30
    "_ZN12_GLOBAL__N_19prio_drawENS_10SampleArgsE": (8, 48, 16),             # 48
    GATHER_ROWS % 0: (7, 32, 0),   # 26
    GATHER_ROWS % 2: (7, 24, 0),   # 22
    GATHER_ROWS % 3: (7, 32, 0),   # 26
    GATHER_ROWS % 4: (7, 32, 0),   # 26
    GATHER_ROWS % 6: (7, 32, 0),   # 32
    GATHER_WIDE % 1: (7, 24, 0),   # 24
    GATHER_WIDE % 0: (7, 24, 0),   # 24
}


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_prio_res_")
    try:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", SRC,
                            "-o", os.path.join(d, "k.o"), "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        yield p.stderr
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_every_kernel_stays_in_registers(remarks):
    res = _resources(remarks)
    assert sorted(res) == sorted(BUDGET)
    for kernel, (occupancy, vgprs, lds) in BUDGET.items():
        r = res[kernel]
        print(kernel, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0 and r["LDS Size"] == lds, (kernel, r)
        assert r["Occupancy"] >= occupancy and r["VGPRs"] <= vgprs, (kernel, r)


def test_the_source_shares_the_rule_the_host_checks_and_the_row_copiers():
    src = re.sub(r"//.*", "", open(SRC).read())
    for include in ('#include "mxv_policy_rule.hpp"', '#include "mxv_policy_host.hpp"', '#include "mxv_replay_rows.hpp"', '#include "../../include/mxv_prio.h"'):
        assert include in src, include
    assert "Call<mxv::PrioCall>" in src and "check_ranges(" in src and "check_stride(" in src and "mxv::philox4x32_10(" in src
    assert "log_rule(" in src and "exp_rule(" in src and "copy_rows<WT>(" in src and "copy_pieces<VEC>(" in src and "launch_wide(" in src
    for copy in (r"\bkThreads\s*=", r"\bkMaxElems\s*=", r"\bkMaxBlocks\s*=", r"struct\s+Range\b", r"\bint\s+check_ranges\b", r"\bphilox4x32_10\s*\([^)]*\)\s*\{",
                 r"0xD2511F53", r"add_word_kernel", r"\bkLogC\b", r"\bkExpC\b", r"double\s+log_rule\s*\(", r"double\s+exp_rule\s*\(", r"void\s+copy_rows\s*\(",
                 r"void\s+copy_pieces\s*\(", r"struct\s+Aligned\b", r"\bkPiece\s*=", r"\bkNarrow\s*="):
        assert not re.search(copy, src), copy
    for word in ("asm", "__expf", "__logf", "log(", "exp(", "pow("):
        assert word not in src.replace("log_rule(", "").replace("exp_rule(", ""), word
    assert src.count("call.advance(") == 1 and "launch_add_word(" not in src
    for script in ("build.sh", "build_asan.sh"):
        assert "mxv_prio.hip" in open(os.path.join(ROOT, "gym_amd", "csrc", script)).read(), script
    host = open(os.path.join(ROOT, "gym_amd", "csrc", "mxv_policy_host.hpp")).read()
    assert "struct PrioCall {" in host and "struct ReplayCall {" in host
    # the copiers live in the shared header, once, and the uniform buffer uses the same text
    rows = open(ROWS).read()
    for piece in ("void copy_rows(", "void copy_pieces(", "constexpr int row_align()", "uint64_t wanted_alignment(", "struct Aligned {", "int launch_wide("):
        assert rows.count(piece) == 1, piece
    assert "__global__" not in rows and "atomic" not in rows
    assert '#include "mxv_replay_rows.hpp"' in open(os.path.join(ROOT, "gym_amd", "csrc", "mxv_replay.hip")).read()


def test_every_atomic_is_on_an_integer_type():
    """Integer sums commute, so the tree has the same bits in any arrival order; a float atomic would not (and none is needed)."""
    src = re.sub(r"//.*", "", open(SRC).read())
    calls = re.findall(r"\b(atomic\w+)\s*\(\s*([^,]+),", src)
    assert len(calls) == 7 and sorted({c[0] for c in calls}) == ["atomicAdd", "atomicExch", "atomicMax"], calls
    for fn, target in calls:
        if fn == "atomicAdd":      # 64-bit sums: the LDS words, a node, a node at the flush
            assert target.startswith(("&top[", "word", "reinterpret_cast<unsigned long long *>(t.node")), (fn, target)
        else:                       # 32-bit leaves and qmax
            assert target.strip() in ("&p.tree.leaf[k]", "p.qmax"), (fn, target)
    for decl in (r"unsigned long long \*word = reinterpret_cast<unsigned long long \*>\(t\.node", r"__shared__ unsigned long long top\[kTopWords\];", r"uint32_t \*leaf;",
                 r"uint32_t \*qmax;", r"uint64_t \*node;"):
        assert re.search(decl, src), decl
    assert not re.search(r"atomic\w*\s*\(\s*(\(float|\(double|reinterpret_cast<\s*(float|double))", src)
    assert "unsafeAtomic" not in src and "__hip_atomic" not in src and "atomicCAS" not in src
