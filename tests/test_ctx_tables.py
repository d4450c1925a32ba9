"""State that every handle of a device shares, on the CPU: the growth policy of the context tables, and the inventory of what is shared.

1. csrc/ctx_tables.h (GrowingTable: the Fr twiddle heaps of ntt.hip, the residue-system heap of rns_ntt.hip).  The rule it keeps -- include/zkmi355x.h
   next to ZK_GRAPH, DESIGN.md "Context-owned tables" -- is that a device pointer to a context table, once handed to an enqueue or a capture, stays valid
   and keeps its values until zk_shutdown.  tests/host/ctx_tables_main.cpp includes only that header; it is built here as a stand-alone program with g++
   under AddressSanitizer + UBSan and run (nothing is loaded into Python): a table grows 2^12 -> 2^13 -> 2^15 with malloc / free as the allocator, and
   after every growth the program reads through every pointer handed out before and compares with the prefix of the new table; then everything is
   released, each buffer exactly once.  A policy that frees on growth (what ntt_ensure_twiddles did through DevBuf::alloc) ends in a heap-use-after-free
   report at the first of those reads: that is how the property shows without a GPU, where the same mistake is a read of freed device memory by a replayed
   graph (tests/test_gpu_live_together.py runs the replays on the fixed library).

2. The inventory.  Every member of Ctx and CtxBufs (csrc/zk_common.h), every mutable file-scope variable and per-device array of the library's sources,
   and every cleanup hook is listed below with its lifetime class.  A new DevBuf in CtxBufs, a new per-device global table or a new hook fails the test
   by name until it has a row here -- and the row asks the question the heaps got wrong: can it be replaced while somebody holds a pointer to it?
   DESIGN.md "Context-owned tables" has the prose for every row."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zukelang_amd", "csrc")

# lifetime classes
ONCE = "once"            # created once per context (zk_init or first use), same handle / pointer until zk_shutdown; never replaced
GROWS = "grows"          # a GrowingTable: replaced by a larger one, old buffers retired until zk_shutdown (ctx_tables.h)
BLOCKING = "blocking"    # device buffers replaced only by a blocking call that drains its stream before it returns; no enqueue or capture is handed them
HOST = "host"            # host-side bookkeeping: no device pointer in it
HANDLES = "handles"      # a handle table (handle_table.h): objects die by their own free call, after a device-wide wait

CTX_MEMBERS = {
    "inited": HOST, "vdev": HOST, "device": HOST, "profiling": HOST, "timers": HOST, "counters": HOST,
    "stream": ONCE,          # set-up work and every blocking call; the heaps are generated on it and complete before the call returns
    "stream2": ONCE,         # the combines of multi-device proofs (device_group.cuh), the key side of verify_resident.hip: in-stream order, per-slot buffers
    "stream3": ONCE, "ev_fork": ONCE, "ev_join": ONCE, "ev_join3": ONCE,          # created and destroyed with the context; nothing records or waits on them
    "tw_fwd": GROWS, "tw_inv": GROWS, "tw_log": GROWS,          # the live pair of CtxBufs::tw_fwd / tw_inv and the levels both hold
    "bufs": ONCE,
    "event_pool": HOST,      # timing events of ScopedTimer, recycled by zk_profile_reset only; profiling switches graphs off (groth16.hip prove_enqueue)
}
CTXBUFS_MEMBERS = {
    "tw_fwd": ("GrowingTable", GROWS), "tw_inv": ("GrowingTable", GROWS),
    "inv_pow2": ("DevBuf", ONCE),          # 66 elements, filled with the first heaps and complete with them
    "pow2": ("DevBuf", ONCE),              # fixed_base_mul: filled on first use on the caller's stream; every caller passes the context's main stream
}
GLOBALS = {
    "rns_ntt.hip:g_rns_tw": GROWS,
    "groth16.hip:g_keys": HANDLES, "groth16_multi.hip:g_groups": HANDLES, "pinocchio.hip:g_pin": HANDLES, "pinocchio.hip:g_pin_groups": HANDLES,
    "verify_resident.hip:g_vk": HANDLES, "msm_resident.hip:g_res": HANDLES,
    "groth16.hip:g_combine": BLOCKING,          # zk_groth16_combine: grows with `world`, on the main stream, synchronised before the call returns
    "zk_api.hip:tl_vdev": HOST,
    "msm_sort.hip:lds_limit": HOST,             # a device attribute, cached per HIP device
}
CLEANUP_HOOKS = {
    "ntt.hip:ntt_release": "the Fr twiddle heaps, live and retired",
    "rns_ntt.hip:rns_release": "the residue-system heap, live and retired",
    "groth16.hip:handles_release": "Groth16 keys and multi-device keys, their slots and graphs",
    "groth16.hip:combine_release": "the buffers of zk_groth16_combine",
    "pinocchio.hip:pin_release": "Pinocchio keys and multi-device keys",
    "verify_resident.hip:vk_release": "resident verification keys",
    "msm_resident.hip:res_release": "resident MSM bases",
}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _struct_members(text, name):
    """[(type text, member name)] of `struct name { ... };` -- data members only, by their declarations"""
    m = re.search(r"\bstruct %s\s*\{" % re.escape(name), text)
    assert m, "struct %s not found in zk_common.h" % name
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    body = text[m.end():i - 1]
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt or "(" in stmt.split("=")[0]:          # member functions (none today) are not state
            continue
        while re.search(r"<[^<>]*>", stmt):                # template arguments hold commas
            stmt = re.sub(r"<[^<>]*>", "", stmt)
        pieces = [re.sub(r"=.*", "", p).strip() for p in stmt.split(",")]
        first = re.match(r"(.*?)([A-Za-z_]\w*)\s*(\[\w*\])?$", pieces[0])
        assert first, stmt
        typ = first.group(1).strip()
        out.append((typ, first.group(2)))
        for p in pieces[1:]:
            nm = re.match(r"[*&\s]*([A-Za-z_]\w*)\s*(\[\w*\])?$", p)
            assert nm, stmt
            out.append((typ, nm.group(1)))
    return out


def _sources():
    return sorted(p for ext in ("*.hip", "*.cuh", "*.h") for p in glob.glob(os.path.join(CSRC, ext)))


def _mutable_statics():
    """file:name of every mutable variable at file scope, and of every static array with one entry per device wherever it stands"""
    found = set()
    for path in _sources():
        base = os.path.basename(path)
        for line in _strip_comments(open(path).read()).split("\n"):
            m = re.match(r"(\s*)static\s+(.*)", line)
            if not m:
                continue
            indent, rest = m.groups()
            if re.match(r"(const|constexpr|inline|CleanupRegistrar)\b", rest):
                continue
            decl = re.split(r"[=;{]", rest)[0]
            if "(" in decl:                                 # a function
                continue
            nm = re.search(r"([A-Za-z_]\w*)\s*(\[\w*\])?\s*$", decl)
            if not nm:
                continue
            per_device = nm.group(2) == "[64]"
            if indent == "" or per_device:
                found.add("%s:%s" % (base, nm.group(1)))
    return found


def _cleanup_hooks():
    found = set()
    for path in _sources():
        for m in re.finditer(r"static\s+CleanupRegistrar\s+\w+\((\w+)\)", _strip_comments(open(path).read())):
            found.add("%s:%s" % (os.path.basename(path), m.group(1)))
    return found


def _common():
    return _strip_comments(open(os.path.join(CSRC, "zk_common.h")).read())


def test_every_member_of_the_context_is_in_the_inventory():
    members = _struct_members(_common(), "Ctx")
    names = [n for _t, n in members]
    assert len(names) == len(set(names))
    missing = [n for n in names if n not in CTX_MEMBERS]
    assert not missing, "Ctx members without a row in tests/test_ctx_tables.py CTX_MEMBERS (who may hold a pointer to them?): %s" % missing
    assert sorted(CTX_MEMBERS) == sorted(names), "rows of members that are gone: %s" % sorted(set(CTX_MEMBERS) - set(names))


def test_every_device_table_of_the_context_is_in_the_inventory():
    members = _struct_members(_common(), "CtxBufs")
    missing = [n for _t, n in members if n not in CTXBUFS_MEMBERS]
    assert not missing, "CtxBufs members without a row in tests/test_ctx_tables.py CTXBUFS_MEMBERS (can they be replaced after first use?): %s" % missing
    assert sorted(CTXBUFS_MEMBERS) == sorted(n for _t, n in members), "rows of members that are gone"
    for typ, n in members:
        want, cls = CTXBUFS_MEMBERS[n]
        assert typ == want, "CtxBufs::%s is a %s, the inventory has %s" % (n, typ, want)
        # the type IS the policy: what may be replaced is a GrowingTable, and a DevBuf (whose alloc frees what it held) is allocated once
        assert (typ == "GrowingTable") == (cls == GROWS), n
    # the live pointers of the context mirror the two growing tables and nothing else
    assert {n for n, c in CTX_MEMBERS.items() if c == GROWS} == {"tw_fwd", "tw_inv", "tw_log"}


def test_every_global_table_and_cleanup_hook_is_in_the_inventory():
    found = _mutable_statics()
    missing = sorted(found - set(GLOBALS))
    assert not missing, "mutable globals / per-device arrays without a row in tests/test_ctx_tables.py GLOBALS: %s" % missing
    assert not sorted(set(GLOBALS) - found), "rows of globals that are gone: %s" % sorted(set(GLOBALS) - found)
    hooks = _cleanup_hooks()
    assert hooks == set(CLEANUP_HOOKS), "cleanup hooks and their rows differ: %s" % sorted(hooks ^ set(CLEANUP_HOOKS))
    # what grows goes through the one policy: the two translation units that own a growing table, and no DevBuf::alloc on a context table beside them
    for unit in ("ntt.hip", "rns_ntt.hip"):
        text = _strip_comments(open(os.path.join(CSRC, unit)).read())
        assert ".grow(" in text and ".release_all(" in text, unit
        assert "hipDeviceSynchronize()" in text, "%s: the wait before a table is replaced is explicit" % unit
    ntt = _strip_comments(open(os.path.join(CSRC, "ntt.hip")).read())
    assert not re.search(r"tw_(fwd|inv)\.alloc\(", ntt)


def test_growing_table_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/host/ctx_tables_main.cpp")
    exe = str(tmp_path / "ctx_tables_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "ctx_tables_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == "ctx_tables ok", res.stdout + res.stderr
    assert "runtime error:" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
