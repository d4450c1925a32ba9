"""The host half of zk_groth16_srs_check and zk_groth16_srs_contribute without a GPU and without Python: csrc/srs_plan.h -- the length checks, the
factor checks and which index of which list carries which coefficient (the shifted copies, the zeros at every list's and relation's end) -- includes
no HIP, so tests/host/srs_plan_main.cpp is built here as a stand-alone program with g++ under AddressSanitizer + UBSan and run (as
tests/test_contribute_host.py runs its program).  The program holds the plan to a naive enumeration of the four relations for every
(N1, NAB, N2) with N1 <= 9, for (300, 7, 9) and (257, 257, 2), and at N1 = 2^25."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zukelang_amd", "csrc")


def test_the_plan_header_holds_no_hip():
    text = open(os.path.join(CSRC, "srs_plan.h")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"hip|__device__|__global__|\.cuh", code), "srs_plan.h is the host-only half: plain C++"
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', code) == ["stddef.h", "stdint.h"]


def test_the_kernel_is_launched_from_the_plan():
    unit = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "srs.hip")).read())
    assert '#include "srs_plan.h"' in unit and "srs_plan_make(" in unit and "srs_lengths_check(" in unit and "srs_factors_check(" in unit
    assert re.findall(r"__global__\s+void\s+(\w+)\s*\(", unit) == ["k_srs_coefficients", "k_srs_factors_to_mont"]
    # the kernel takes the plan by value and asks the header's own function, the one the host program holds to the relations, for every scalar
    body = unit[unit.index("void k_srs_coefficients("):unit.index("void k_srs_factors_to_mont(")]
    assert "SrsPlan p" in body and "srs_plan_coef(p, g)" in body and "seed_expand_at(seed, (uint64_t)c.rho)" in body
    assert not re.search(r"\b(lo|hi|shift|first)\b", body), "no list-end arithmetic of the kernel's own"


def test_plan_and_refusals_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/host/srs_plan_main.cpp")
    exe = str(tmp_path / "srs_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "srs_plan_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == "srs_plan ok", res.stdout + res.stderr
    assert "runtime error:" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
