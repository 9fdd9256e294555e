"""The host validation of the calls of include/mxv_sac.h under AddressSanitizer + UBSan, without Python between the caller
and the library: tests/c_consumer/sac_args.c — a stand-alone program — is built with the sanitizers and linked against the
sanitized library (gym_amd/_lib/asan/libmxv_asan.so, gym_amd/csrc/build_asan.sh).  Every call is an argument error and returns before
the device is touched, so this runs on the CPU."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_abi_fuzz import CLANG, ENV, SAN, _asan_library


def test_argument_checks_hold_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang with sanitizer runtimes")
    lib = _asan_library()
    libdir, libname = os.path.dirname(lib), os.path.basename(lib)[3:-3]
    exe = str(tmp_path / "sac_args")
    p = subprocess.run([CLANG] + SAN + ["-std=gnu99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", exe,
                                        os.path.join(ROOT, "tests", "c_consumer", "sac_args.c"), f"-L{libdir}", f"-l{libname}",
                                        f"-Wl,-rpath,{libdir}", "-lm"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=60)
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error:" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert r.returncode == 0 and "sac_args: calls=237 bad=0" in out, out[-3000:]
