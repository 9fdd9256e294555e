"""Resource budget of gym_amd/csrc/mxv_gae.hip, guarded on the CPU (hipcc cross-compiles gfx950 without a GPU; seconds).

All sixteen instantiations of gae_kernel — reward dtype x mode x final_values x envs per lane — hold their ring of loaded rows in
registers: no scratch, no spilled vector register.  At V = 1 the float32 instantiations without final_values fit 64 VGPRs, i.e. 8 waves
per SIMD: the occupancy the V = 4 threshold counts on (32 wave slots per CU); every other V = 1 one keeps at least 5 waves.  And the ring
stays deep: in the K loop of the instantiations without final_values — one basic block per group of steps — every wait in front of a
row's arithmetic is a counted one that leaves the loads of kRing later rows in flight (3 loads per row for returns, 4 for GAE, one more
for float64 rewards at V = 4), never vmcnt(0)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "gym_amd", "csrc", "mxv_gae.hip")


@pytest.fixture(scope="module")
def build():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="mxv_gae_res_")
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


def _resources(remarks):
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: [^ ]+ +(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None:
            cur[k.split(" [")[0]] = int(v)
    return out


def _symbol(f64, gae, fv, v):
    return f"_ZN12_GLOBAL__N_110gae_kernelI{'d' if f64 else 'f'}Lb{int(gae)}ELb{int(fv)}ELi{v}EEEvNS_7GaeArgsE"


ALL = [(f64, gae, fv, v) for f64 in (0, 1) for gae in (0, 1) for fv in (0, 1) for v in (1, 4)]


def test_every_instantiation_has_no_scratch_and_no_spill(build):
    res = {k: r for k, r in _resources(build[0]).items() if "gae_kernel" in k}
    assert sorted(res) == sorted(_symbol(*i) for i in ALL)
    for inst in ALL:
        r = res[_symbol(*inst)]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["LDS Size"] == 0, (inst, r)
        if inst[3] == 1:
            f64, _, fv, _ = inst
            assert r["Occupancy"] >= (5 if f64 or fv else 8), (inst, r)


def _function_body(asm, sym):
    start = asm.index(f"\n{sym}:")
    return asm[start:asm.index(".end_amdhsa_kernel", start)]


def test_the_ring_is_waited_for_with_counted_waits(build):
    from gym_amd.returns import RING_DEPTH

    asm = build[1]
    for f64, gae, fv, v in ALL:
        body = _function_body(asm, _symbol(f64, gae, fv, v))
        assert "scratch_" not in body and "ds_" not in body.replace("ds_nop", "") and "global_atomic" not in body
        if fv:
            continue
        blocks = re.split(r"\n(?=\.LBB\d+_\d+:|; %bb\.\d+:)", body)
        loop = [b for b in blocks if "Depth=2" in "\n".join(b.splitlines()[:4]) and "global_store" in b]
        assert len(loop) == 1, (f64, gae, v, len(loop))           # the group of RING_DEPTH + 1 steps: one block, no exits
        per_row = (4 if gae else 3) + (1 if f64 and v == 4 else 0)
        assert loop[0].count("global_load") == per_row * (RING_DEPTH + 1) and loop[0].count("global_store") == (2 if gae else 1) * (RING_DEPTH + 1)
        waits = [int(n) for n in re.findall(r"s_waitcnt[^\n]*vmcnt\((\d+)\)", loop[0])]
        assert waits and min(waits) >= per_row * RING_DEPTH, ((f64, gae, v), waits)
        width = "dwordx4" if v == 4 else "dword"
        assert all(re.search(rf"global_store_{width}\b", l) for l in loop[0].splitlines() if "global_store" in l)
