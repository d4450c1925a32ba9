"""CPU guard of the option table (tests/option_cases.py): one row per public option of csrc/zk_api.hip, the `read` column true to the C sources,
and every name accepted by zk_set_option.  A knob added without a parity case, a row deleted, or a knob newly cached fails here, without a GPU."""
import glob
import os
import re

from zukelang_amd import _lib

from option_cases import CACHED_GROUPS, CASES, live_runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zukelang_amd", "csrc")


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def public_options():
    text = open(os.path.join(CSRC, "zk_api.hip")).read()
    m = re.search(r"PUBLIC_OPTIONS\[\]\s*=\s*\{(.*?)\};", text, flags=re.S)
    assert m, "PUBLIC_OPTIONS not found in zk_api.hip"
    names = re.findall(r'"([A-Z0-9_]+)"', _strip_comments(m.group(1)))
    assert len(names) == len(set(names)), "a name listed twice in PUBLIC_OPTIONS"
    return names


def read_sites():
    """name -> set of read kinds found in the sources: "cached" (ZK_ENV, or a function-local static initialised from ::zk::opt), "form" (ZK_FORM_ENV)"""
    sites = {}
    files = glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cuh"))
    for f in files:
        code = _strip_comments(open(f).read())
        for name in re.findall(r'(?<![A-Za-z0-9_])ZK_ENV\(\s*"(ZK_[A-Z0-9_]+)"\s*\)', code):
            sites.setdefault(name, set()).add("cached")
        for stmt in re.findall(r"\bstatic\s+const\b[^;{}]*?=[^;]*;", code):
            for name in re.findall(r'::zk::opt\(\s*"(ZK_[A-Z0-9_]+)"\s*\)', stmt):
                sites.setdefault(name, set()).add("cached")
        for name in re.findall(r'\bZK_FORM_ENV\(\s*"(ZK_[A-Z0-9_]+)"\s*\)', code):
            sites.setdefault(name, set()).add("form")
    return sites


def test_the_table_has_one_row_per_public_option():
    names = public_options()
    assert len(names) == 28
    assert sorted(CASES) == sorted(names), ("rows without a public option: %s; public options without a row: %s"
                                            % (sorted(set(CASES) - set(names)), sorted(set(names) - set(CASES))))
    for name, c in CASES.items():
        assert c.values, name
        assert c.read in ("cached", "setup", "call"), name
        assert c.size in ("small", "ba"), name
        assert name not in c.with_, name


def test_every_cached_read_is_marked_cached():
    sites = read_sites()
    public = set(public_options())
    # the scan itself must find the known sites (a regex that matches nothing would pass everything below)
    assert "cached" in sites.get("ZK_SLOT_STREAMS", ()) and "cached" in sites.get("ZK_SORT_SCALAR_MAJOR", ())
    assert "cached" in sites.get("ZK_MSM_TARGET_THREADS", ()) and "form" in sites.get("ZK_TAIL_SLOTS", ())
    for name, kinds in sorted(sites.items()):
        if name not in public:
            continue                                                 # test-only and experiment switches have no row
        if "cached" in kinds:
            assert CASES[name].read == "cached", "%s is read once per process (ZK_ENV / static): mark it cached and give it a child-process group" % name
        elif "form" in kinds:
            assert CASES[name].read == "call", "%s is a kernel-form switch (ZK_FORM_ENV): read per call under ZK_TEST_FORMS=1" % name
    for name, c in CASES.items():
        if c.read == "cached":
            assert "cached" in sites.get(name, ()), "%s is marked cached but no cached read site was found" % name


def test_every_cached_value_runs_in_a_child_process():
    assert 1 <= len(CACHED_GROUPS) <= 3
    for g in CACHED_GROUPS:
        for name in g:
            assert CASES[name].read == "cached", name
    for name, c in CASES.items():
        if c.read == "cached":
            for v in c.values:
                assert any(g.get(name) == v for g in CACHED_GROUPS), "%s=%s is in no child-process group" % (name, v)
    runs = live_runs()
    assert len(runs) == sum(len(c.values) for c in CASES.values() if c.read != "cached" and not c.special)
    for _id, _c, settings in runs:
        assert all(CASES[k].read != "cached" for k in settings), _id


def test_zk_set_option_accepts_every_name_of_the_table():
    L = _lib.lib()
    for name in CASES:
        for spelling in (name, name[3:].lower()):
            _lib.check(L.zk_set_option(spelling.encode(), b"1"))
            _lib.check(L.zk_set_option(spelling.encode(), None))     # back to the environment
    assert L.zk_set_option(b"ZK_NOT_AN_OPTION", b"1") != 0
