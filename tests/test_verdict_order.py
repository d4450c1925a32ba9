"""csrc/verdict_order.h on the CPU: the order in which the verifiers meet the points of a proof and of a key, written once for the kernel
k_vk_status and the two key builders of csrc/verify_resident.hip, which the resident keys' uploads and the zk_*_verify_many calls share.

tests/host/verdict_order_main.cpp includes only that header; it is built here as a stand-alone program with g++ under AddressSanitizer + UBSan and run
(nothing is loaded into Python).  Against lists written out in the program it checks each plan's order (Groth16: A B C; Pinocchio: vv ww yy h vavv waww
yayy bvwy, ww and waww in G2) and offsets, that of two bad verdicts the earlier position wins, that a scalar defect loses to any point defect and a clean
proof gives 0 -- for proofs 0 and 2 of 3 --, the key-defect order and messages of both protocols for 0, 1 and 3 public inputs with a later defect of a
stronger kind planted, verdict_code over 0, 1, 2, 4, 8, and the 576 bytes of 1."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_verdict_order_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/host/verdict_order_main.cpp")
    exe = str(tmp_path / "verdict_order_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "verdict_order_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == "verdict_order ok", res.stdout + res.stderr
    assert "runtime error:" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
