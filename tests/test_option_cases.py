"""CPU guard of the option table (tests/option_cases.py): one row per PUBLIC row of csrc/zk_options.h, the `read` column true to each row's kind,
and every name accepted by zk_set_option.  A knob added without a parity case, a row deleted, or a knob newly cached fails here, without a GPU.
The same for the route table (ROUTES): every entry point of include/zkmi355x.h that makes, fills or uses a handle has a row or a reason, the
verifiers' lack of one is true to their sources, and the key-check route's batch-affine rows reach their rounds."""
import glob
import os
import re

from zukelang_amd import _lib

from option_cases import (CACHED_GROUPS, CASES, CSRC, EXEMPT, FLIPS, KEY_CHECK_POOLS, OPTION_READ, OPTIONS_UNIT, PROVE_ROUTE, ROUTED_WORDS, ROUTES,
                          VERIFIER_SOURCES, live_runs, option_table, public_options, route_settings)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def read_sites():
    """name -> the units of csrc/ outside the options unit that read it, by the row's id or through one of the named readers of csrc/zk_options.h"""
    named = {"key_subgroup_check": ["ZK_KEY_SUBGROUP_CHECK"], "trace_on": ["ZK_TRACE"], "forms_live": ["ZK_TEST_FORMS"],
             "opt_form_fingerprint": [r.name for r in option_table() if r.kind == "FORM" and r.name != "ZK_GRAPH"]}
    sites = {}
    for f in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cuh")) + glob.glob(os.path.join(CSRC, "*.h"))):
        if os.path.basename(f) == OPTIONS_UNIT:
            continue
        for fn, by_id, reader in OPTION_READ.findall(_strip_comments(open(f).read())):
            if fn == "opt_set":
                continue                                                 # zk_set_option itself (zk_api.hip): a write, by name
            assert by_id or reader or fn in named, "%s: %s( is handed something other than a row's literal id" % (os.path.basename(f), fn)
            for name in (["ZK_" + by_id] if by_id else named[reader or fn]):
                sites.setdefault(name, set()).add(os.path.basename(f))
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
    rows = {r.name: r for r in option_table()}
    sites = read_sites()
    # the scan itself must find the known sites (a regex that matches nothing would pass everything below)
    assert {"groth16.hip", "pinocchio.hip"} <= sites["ZK_SERIAL_STREAMS"] and sites["ZK_SLOT_STREAMS"] == {"groth16.hip"} and sites["ZK_SORT_SCALAR_MAJOR"] == {"msm_sort.hip"}
    assert sites["ZK_MSM_TARGET_THREADS"] == {"msm.hip"} and {"msm.hip", "groth16.hip"} <= sites["ZK_TAIL_SLOTS"] and sites["ZK_GRAPH"] == {"groth16.hip"}
    assert len(sites["ZK_KEY_SUBGROUP_CHECK"]) == 5 and sites["ZK_TRACE"] == {"zk_api.hip", "ctx_tables.h", "groth16_multi.hip"}
    assert rows["ZK_SLOT_STREAMS"].kind == "CACHED" and rows["ZK_TAIL_SLOTS"].kind == "FORM" and rows["ZK_MSM_WINDOW"].kind == "LIVE"
    for name, c in CASES.items():
        kind = rows[name].kind
        assert (kind == "CACHED") == (c.read == "cached"), "%s is %s in zk_options.h: a row read once per process is marked cached and has a child-process group, no other is" % (name, kind)
        if kind == "FORM":
            assert c.read == "call", "%s is a kernel-form switch: read per call under ZK_TEST_FORMS=1" % name
        if kind == "LIVE":
            assert c.read in ("setup", "call"), name
    for r in rows.values():
        assert sites.get(r.name), "%s has a row in zk_options.h and no unit reads it" % r.name
    assert set(sites) <= set(rows), "read by an id that is no row: %s" % sorted(set(sites) - set(rows))


def test_only_the_options_unit_reads_by_name():
    """no getenv and no "ZK_..." literal handed to a reader outside csrc/zk_options.h; names inside error texts ("... must be ZK_KEY_FORM_...") are not reads"""
    seen = 0
    for f in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cuh")) + glob.glob(os.path.join(CSRC, "*.h")):
        code = _strip_comments(open(f).read())
        seen += len(re.findall(r'"ZK_[A-Z0-9_]+"', code))
        if os.path.basename(f) == OPTIONS_UNIT:
            assert "getenv(" in code                                     # the scan does find what is there
            continue
        assert not re.search(r"\bgetenv\s*\(", code), "%s calls getenv: options are read through csrc/zk_options.h" % os.path.basename(f)
        hits = re.findall(r'\b\w+\s*\(\s*"ZK_[A-Z0-9_]+"\s*[,)]', code)
        assert not hits, "%s hands an option's name to %s: read it by its id (csrc/zk_options.h)" % (os.path.basename(f), hits)
    assert seen >= 34


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
        m = OPTION_READ.search(code)
        assert not m and '#include "zk_options.h"' not in code, "%s reads an option (%s): the verifiers need a row in option_cases.ROUTES" % (name, m and m.group(0))
    assert OPTION_READ.search(_strip_comments(open(os.path.join(CSRC, "msm.hip")).read()))          # the scan does find what is there


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
