"""The host validation of include/mxv_vtrace.h without Python between the caller and the library: tests/c_consumer/vtrace_args.c — a
stand-alone plain-C program — built against the shipped library, and built with AddressSanitizer + UBSan and linked against the
sanitized library (gym_amd/_lib/asan/libmxv_asan.so, gym_amd/csrc/build_asan.sh).  Every call is an argument error and returns before
the device is touched, so both run on the CPU; nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_abi_fuzz import CLANG, ENV, SAN, _asan_library

SRC = os.path.join(ROOT, "tests", "c_consumer", "vtrace_args.c")
CALLS = 49


def _build_and_run(compiler, flags, lib, exe, env=None):
    libdir, libname = os.path.dirname(lib), os.path.basename(lib)[3:-3]
    p = subprocess.run([compiler] + flags + ["-std=gnu99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, f"-L{libdir}",
                                             f"-l{libname}", f"-Wl,-rpath,{libdir}", "-lm"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    return r.returncode, r.stdout + r.stderr


def test_every_call_is_refused_with_a_message_naming_the_argument(tmp_path):
    from gym_amd import _native

    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    rc, out = _build_and_run(cc, ["-O1"], _native.LIB_PATH, str(tmp_path / "vtrace_args"))
    assert rc == 0 and f"vtrace_args: calls={CALLS} bad=0" in out, out[-3000:]


def test_argument_checks_hold_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang with sanitizer runtimes")
    rc, out = _build_and_run(CLANG, SAN, _asan_library(), str(tmp_path / "vtrace_args_san"), env=ENV)
    assert "AddressSanitizer" not in out and "runtime error:" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert rc == 0 and f"vtrace_args: calls={CALLS} bad=0" in out, out[-3000:]
