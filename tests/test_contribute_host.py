"""The host half of zk_groth16_pk_contribute without a GPU and without Python: csrc/contribute_scalar.h -- delta' as 256-bit words, its range checks
and its inverse mod r, computed once per call -- includes no HIP, so tests/host/contribute_main.cpp is built here as a stand-alone program with g++
under AddressSanitizer + UBSan and run (as tests/test_ctx_tables.py runs its program).  The program checks k k^-1 = 1 for the edge scalars and 1000
random ones with arithmetic of its own.  (It also checked the endomorphism split and the signed 4-bit digits while the call had a kernel that took
them by value; that kernel was measured and dropped, DESIGN 2q, and the shipped route splits and recodes on the device.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zukelang_amd", "csrc")


def test_the_scalar_header_holds_no_hip():
    text = open(os.path.join(CSRC, "contribute_scalar.h")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"hip|__device__|__global__|\.cuh", code), "contribute_scalar.h is the host-only half: plain C++"
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', code) == ["stdint.h", "string.h"]


def test_split_recoding_and_inverse_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/host/contribute_main.cpp")
    exe = str(tmp_path / "contribute_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "contribute_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == "contribute_scalar ok", res.stdout + res.stderr
    assert "runtime error:" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
