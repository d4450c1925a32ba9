"""csrc/handle_table.h on the CPU: the one table type behind every kind of handle, and the handle ranges.

tests/host/handle_table_main.cpp includes only that header; it is built here as a stand-alone program with g++ under AddressSanitizer + UBSan and run
(nothing is loaded into Python).  It checks that the ranges are pairwise disjoint, the add / find / take round trip, that another table's live number,
0 and a taken number give null, that take destroys exactly once, that the registry's sum (what guards zk_set_device_list) follows adds and takes across
three tables, and that release visits every live entry once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handle_table_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/host/handle_table_main.cpp")
    exe = str(tmp_path / "handle_table_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "handle_table_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == "handle_table ok", res.stdout + res.stderr
    assert "runtime error:" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
