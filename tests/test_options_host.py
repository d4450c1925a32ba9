"""The option table without a GPU and without Python: csrc/zk_options.h -- every ZK_* name the library reads, when each is read, who may set it, the
parse rules and the fingerprint of the kernel forms that a captured graph is held to -- includes no HIP, so tests/host/options_main.cpp is built here
as a stand-alone program with g++, once under AddressSanitizer + UBSan and once under ThreadSanitizer (as tests/test_srs_plan_host.py builds its
program), and each build runs twice: in test mode (ZK_TEST_FORMS=1 in the environment at start: FORM rows follow every set) and outside it (the
shipped path: they keep their first value).  The program's last part races eight first reads of one cached row against a ninth thread that sets it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zukelang_amd", "csrc")


def test_the_options_header_holds_no_hip():
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "zk_options.h")).read()))
    assert not re.search(r"\bhip\w*\b|__device__|__global__|\.cuh", code), "zk_options.h is host-only: plain C++"
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["zk_err.h"]
    err = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "zk_err.h")).read())
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', err) == ["../../include/zkmi355x.h"]


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_the_table_under_sanitizers(tmp_path, sanitizer):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/host/options_main.cpp")
    exe = str(tmp_path / "options_main")
    flags = ["-fsanitize=" + sanitizer] + (["-fno-sanitize-recover=undefined"] if "undefined" in sanitizer else [])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags
                          + ["-o", exe, os.path.join(ROOT, "tests", "host", "options_main.cpp")])
    base = {k: v for k, v in os.environ.items() if not k.startswith("ZK_")}
    base.update(ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    for forms in ("1", "0"):
        env = dict(base, ZK_TEST_FORMS="1") if forms == "1" else base
        res = subprocess.run([exe, forms], capture_output=True, text=True, timeout=120, env=env)
        assert res.returncode == 0, res.stdout + res.stderr
        assert res.stdout.strip() == "options ok", res.stdout + res.stderr
        assert "runtime error:" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr
