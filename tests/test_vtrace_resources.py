"""Resource budget of gym_amd/csrc/mxv_vtrace.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

All eight instantiations of vtrace_kernel — reward dtype x final_values x envs per lane — hold their ring of loaded rows in registers:
no scratch, no spilled vector register, no LDS (scalar registers that the compiler parks in the lanes of a vector register touch no
memory); the occupancy and the vector registers are at least / at most what the compiler reported when the kernel was written
(DESIGN.md §16 records the figures).  And the ring stays deep: in the K loop of the
instantiations without final_values — one basic block per group of steps — every wait in front of a row's arithmetic is a counted one
that leaves the loads of kRing later rows in flight (6 loads per row, one more for float64 rewards at V = 4), never vmcnt(0).  The
source is in both build scripts, includes the shared rule and defines no copy of it, and uses no atomics, LDS or assembly; it and
mxv_gae.hip take the walk, the host checks and the limits from mxv_trajectory.hpp and the rule header and define no copy of those."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import policy_host
from conftest import ROOT
from test_gae_resources import HIPCC, _function_body, _resources

SRC = os.path.join(ROOT, "gym_amd", "csrc", "mxv_vtrace.hip")
ALL = [(f64, fv, v) for f64 in (0, 1) for fv in (0, 1) for v in (1, 4)]
# (float64 rewards, final_values, envs per lane): (waves per SIMD, VGPR bound) — the reported VGPRs rounded up to the granule of 8
BUDGET = {(0, 0, 1): (5, 96), (0, 1, 1): (4, 112), (1, 0, 1): (4, 104), (1, 1, 1): (4, 112),
          (0, 0, 4): (2, 192), (0, 1, 4): (2, 200), (1, 0, 4): (2, 208), (1, 1, 4): (2, 232)}


def _symbol(f64, fv, v):
    return f"_ZN12_GLOBAL__N_113vtrace_kernelI{'d' if f64 else 'f'}Lb{int(fv)}ELi{v}EEEvNS_6VtArgsE"


@pytest.fixture(scope="module")
def build():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_vtrace_res_")
    try:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", SRC,
                            "-o", os.path.join(d, "k.o"), "-Rpass-analysis=kernel-resource-usage", "-save-temps"], cwd=d, capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        asm = [f for f in os.listdir(d) if f.endswith("gfx950.s")]
        assert asm
        yield p.stderr, open(os.path.join(d, asm[0])).read()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_every_instantiation_has_no_scratch_and_no_spill(build):
    res = {k: r for k, r in _resources(build[0]).items() if "vtrace_kernel" in k}
    assert sorted(res) == sorted(_symbol(*i) for i in ALL)
    for inst in ALL:
        r = res[_symbol(*inst)]
        print(inst, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["LDS Size"] == 0, (inst, r)
        occupancy, vgprs = BUDGET[inst]
        assert r["Occupancy"] >= occupancy and r["VGPRs"] <= vgprs, (inst, r)


def test_the_ring_is_waited_for_with_counted_waits(build):
    from gym_amd.vtrace import RING_DEPTH

    asm = build[1]
    for f64, fv, v in ALL:
        body = _function_body(asm, _symbol(f64, fv, v))
        assert "scratch_" not in body and "ds_" not in body.replace("ds_nop", "") and "global_atomic" not in body
        if fv:
            continue
        blocks = re.split(r"\n(?=\.LBB\d+_\d+:|; %bb\.\d+:)", body)
        loop = [b for b in blocks if "Depth=2" in "\n".join(b.splitlines()[:4]) and "global_store" in b]
        assert len(loop) == 1, (f64, v, len(loop))           # the group of RING_DEPTH + 1 steps: one block, no exits
        per_row = 6 + (1 if f64 and v == 4 else 0)          # log_prob, old_log_prob, reward, values, two flag rows
        assert loop[0].count("global_load") == per_row * (RING_DEPTH + 1) and loop[0].count("global_store") == 2 * (RING_DEPTH + 1)
        waits = [int(n) for n in re.findall(r"s_waitcnt[^\n]*vmcnt\((\d+)\)", loop[0])]
        assert waits and min(waits) >= per_row * RING_DEPTH, ((f64, v), waits)
        width = "dwordx4" if v == 4 else "dword"
        assert all(re.search(rf"global_store_{width}\b", l) for l in loop[0].splitlines() if "global_store" in l)


def test_the_source_is_built_by_both_scripts_and_shares_the_rule():
    block, src = policy_host.rule_block("mxv_vtrace.hip")       # includes mxv_policy_rule.hpp, defines none of RULE_NAMES
    assert "kExpC" in block
    code = re.sub(r"//.*", "", src)
    assert "exp_rule(" in code and "kThreads" in code
    for copy in (r"\bexp_rule\s*\(\s*double", r"\bkThreads\s*=", r"\bkMaxBlocks\s*=", r"\bkExpC\b", r"\bkInvLn2\b", r"\bkMaxElems\s*="):
        assert not re.search(copy, code), copy
    for word in ("atomic", "asm", "__shfl", "__shared__", "__syncthreads"):
        assert word not in code, word
    # mxv_gae.hip takes the launch shape and the limits from the same header, and both take what the two recurrences share from
    # mxv_trajectory.hpp: neither defines a copy
    gae = re.sub(r"//.*", "", policy_host.rule_block("mxv_gae.hip")[1])
    assert "kThreads" in gae
    for copy in (r"\bkThreads\s*=", r"\bkMaxBlocks\s*=", r"\bkMaxElems\s*="):
        assert not re.search(copy, gae), copy
    shared = re.sub(r"//.*", "", open(os.path.join(ROOT, "gym_amd", "csrc", "mxv_trajectory.hpp")).read())
    for name, text in (("mxv_gae.hip", gae), ("mxv_vtrace.hip", code)):
        assert '#include "mxv_trajectory.hpp"' in text and "MXV_TRAJECTORY_WALK(" in text, name
        for copy in (r"\bshares_bytes\s*\(\s*Span\b", r"\bstruct\s+Span\b", r"\bto_f32\s*\(\s*double\b", r"\bkRing\s*=", r"\bkVecMinN\s*=",
                     r"sched_barrier", r"\bstruct\s+LastLaunch\b"):
            assert not re.search(copy, text), (name, copy)
            assert re.search(copy, shared), copy
    for script in ("build.sh", "build_asan.sh"):
        assert "mxv_vtrace.hip" in open(os.path.join(ROOT, "gym_amd", "csrc", script)).read(), script
    flags = open(os.path.join(ROOT, "gym_amd", "csrc", "build.sh")).read()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-ffast-math" not in flags
