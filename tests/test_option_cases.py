"""CPU guard of the option table (tests/option_cases.py): one row per public option of csrc/zk_api.hip, the `read` column true to the C sources,
and every name accepted by zk_set_option.  A knob added without a parity case, a row deleted, or a knob newly cached fails here, without a GPU.
The same for the route table (ROUTES): every entry point of include/zkmi355x.h that makes, fills or uses a handle has a row or a reason, the
verifiers' lack of one is true to their sources, and the key-check route's batch-affine rows reach their rounds."""
import glob
import os
import re

from zukelang_amd import _lib

from option_cases import (CACHED_GROUPS, CASES, EXEMPT, FLIPS, KEY_CHECK_POOLS, PROVE_ROUTE, ROUTED_WORDS, ROUTES, VERIFIER_SOURCES, live_runs,
                          route_settings)

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


# ---- the routes (option_cases.ROUTES): every way to a handle has a row
def header_entry_points():
    text = _strip_comments(open(os.path.join(ROOT, "include", "zkmi355x.h")).read())
    names = re.findall(r"^\s*int\s+(zk_[a-z0-9_]+)\s*\(", text, flags=re.M)
    assert len(names) == len(set(names)) and "zk_groth16_prove" in names and "zk_msm_resident_many" in names and "zk_pinocchio_keygen" in names
    return names


def uncovered_entry_points(routes):
    """the routed entry points of the header that neither a row of `routes`, nor the first route, nor EXEMPT names"""
    named = set(PROVE_ROUTE) | set(EXEMPT) | {e for r in routes.values() for e in r.entry}
    return sorted(f for f in header_entry_points() if any(w in f for w in ROUTED_WORDS) and f not in named)


def test_every_routed_entry_point_of_the_header_has_a_route():
    missing = uncovered_entry_points(ROUTES)
    assert not missing, "no row of option_cases.ROUTES (and no EXEMPT line) for %s: no public option is held to the oracle on that route" % missing
    header = set(header_entry_points())
    places = list(PROVE_ROUTE) + list(EXEMPT) + [e for r in ROUTES.values() for e in r.entry]
    assert len(places) == len(set(places)), "an entry point stands in two places: %s" % sorted(p for p in set(places) if places.count(p) > 1)
    for name in places:
        assert name in header, "%s is not an entry point of include/zkmi355x.h" % name
        assert any(w in name for w in ROUTED_WORDS), "%s is none of the routed kinds" % name
    for name, why in EXEMPT.items():
        assert why and "\n" not in why, name
    for rid, r in ROUTES.items():
        assert r.entry and r.protocol in ("groth16", "pinocchio", "msm") and r.multi in ("proofs", "bytes", None), rid
        assert all(k in CASES for k in r.with_ba), rid


def test_a_deleted_row_is_noticed_by_name():
    """every row is the only cover of its entry points: without it they are reported"""
    for rid, r in ROUTES.items():
        rest = {k: v for k, v in ROUTES.items() if k != rid}
        assert uncovered_entry_points(rest) == sorted(r.entry), rid


def test_the_verifiers_read_no_option():
    """why they have no route; if one of them ever reads a knob, they get one"""
    for name in VERIFIER_SOURCES:
        code = _strip_comments(open(os.path.join(CSRC, name)).read())
        for word in ("::zk::opt", "ZK_ENV", "ZK_FORM_ENV"):
            assert word not in code, "%s reads an option (%s): the verifiers need a row in option_cases.ROUTES" % (name, word)
    assert "::zk::opt" in _strip_comments(open(os.path.join(CSRC, "msm.hip")).read())          # the scan does find what is there


def test_the_key_check_route_reaches_the_automatic_batch_affine_rounds():
    """msm.hip, ba_rounds_for: no round below a mean of 8 entries per bucket, n nw / nbuckets.  The key of the key-check route has one size, so its
    "ba" rows force the window the table says; with it every pool of both key forms is far above 8."""
    src = _strip_comments(open(os.path.join(CSRC, "msm.hip")).read())
    assert re.search(r"mean\s*=\s*b\.n\s*\*\s*b\.nw\s*/\s*nbuckets", src) and re.search(r"\(uint64_t\)8\s*<<\s*r\)\s*<=\s*mean", src), "ba_rounds_for changed its rule"
    c = int(ROUTES["g16_key_check"].with_ba["ZK_MSM_WINDOW"])
    assert 255 % c, "a width that folds would make the window count depend on the subgroup verdict"
    nw, nbuckets = 255 // c + 1, 1 << (c - 1)          # msm.cuh: msm_windows, and one bucket set for a table (msm_workspace_alloc)
    assert sorted(KEY_CHECK_POOLS) == ["lagrange", "tau_powers"]
    n, n_mid = 1025, 1035                                # tests/test_gpu_key_check.py: CIRCUITS["n1025"] = random_r1cs(1025, 1100, 5): 1035 of its 1100 variables are mids
    assert KEY_CHECK_POOLS["tau_powers"] == (3 + (n + 2) + (n - 1) + n_mid, 2 + (n + 2)) and KEY_CHECK_POOLS["lagrange"] == (3 + n + (n - 1) + n_mid, 2 + n)
    for form, pools in KEY_CHECK_POOLS.items():
        for points in pools:
            assert points * nw // nbuckets >= 8, (form, points)
    for name, case_ in CASES.items():
        if case_.size == "ba":
            for v in case_.values:
                s = route_settings("g16_key_check", case_, dict(case_.with_, **{name: v}))
                assert s["ZK_MSM_WINDOW"] == str(c) and s[name] == v
        elif "ZK_MSM_WINDOW" not in case_.with_ and name != "ZK_MSM_WINDOW":
            assert "ZK_MSM_WINDOW" not in route_settings("g16_key_check", case_, dict(case_.with_, **{name: case_.values[0]}))


def test_the_flips_are_live_settings():
    for fid, settings in FLIPS.items():
        assert settings and all(CASES[k].read != "cached" for k in settings), fid


def test_zk_set_option_accepts_every_name_of_the_table():
    L = _lib.lib()
    for name in CASES:
        for spelling in (name, name[3:].lower()):
            _lib.check(L.zk_set_option(spelling.encode(), b"1"))
            _lib.check(L.zk_set_option(spelling.encode(), None))     # back to the environment
    assert L.zk_set_option(b"ZK_NOT_AN_OPTION", b"1") != 0
