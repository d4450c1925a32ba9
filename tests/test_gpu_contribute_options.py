"""zk_groth16_pk_contribute under every public option.  include/zkmi355x.h promises that no knob of zk_set_option changes a result, and
tests/option_cases.py holds every key, proving and pool call to that promise through its ROUTES table -- by the words in a call's name.  The
contribution's name holds none of them on purpose (tests/test_contribute_surface.py), because that table cannot gain a row here; this module keeps the
promise for it: the call rebuilds both pools' window tables and drops every slot, so it reads the same options an upload and a first proof read.

Every run: upload the n1025 key of tests/test_gpu_contribute.py (3089 / 1029 points in the reference's format, 3087 / 1027 in Lagrange form -- the
pools of option_cases.KEY_CHECK_POOLS), contribute, prove.  Expected: the pools of the host keygen and the trapdoor oracle's proofs for the trapdoor
with delta * delta', computed once before any option is set.  The rows of size "ba" get the key-check route's companions (route_settings: window 8),
with which the rebuilt tables reach the batch-affine rounds at this size."""
import os
import subprocess
import sys

import pytest

import test_gpu_contribute as TC
import test_gpu_options as T
from option_cases import CACHED_GROUPS, FLIPS, live_runs, route_settings
from zukelang_amd import _lib

pytestmark = pytest.mark.gpu

NAME, D = "n1025", TC.D1
ROUTE = "g16_key_check"          # whose companions the "ba" rows take: its key is this one


def prepare():
    _lib.check(_lib.lib().zk_init(0))
    return TC.world(NAME, 1), TC.world(NAME, D)


def contribute_and_prove(pr, old, new, form, tag):
    c = pr.contribute(D)
    TC.is_link(c, old, new, D, tag)
    TC.is_key(pr, new, form, tag)
    assert pr.prove_many(TC.BLINDS, [new.w] * 2, in_flight=2) == new.wire, (tag, "prove_many")


def run(settings, tag):
    old, new = prepare()
    for form in TC.FORMS:
        pr = TC.make(old, form, "upload")
        try:
            contribute_and_prove(pr, old, new, form, (tag, form))
        finally:
            pr.close()


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    yield
    _lib.set_device_list([0])


@pytest.mark.parametrize("c,settings", [pytest.param(c, settings, id=rid) for rid, c, settings in live_runs()])
def test_a_live_option_leaves_a_contributed_key_as_the_oracle_has_it(c, settings):
    prepare()
    settings = route_settings(ROUTE, c, settings)
    with T.options(settings):
        run(settings, settings)


def _flip(fid, direction):
    return ({}, FLIPS[fid]) if direction == "set" else (FLIPS[fid], {})


@pytest.mark.parametrize("fid,direction", [pytest.param(fid, d, id="%s-%s" % (fid, d)) for fid in FLIPS for d in ("set", "unset")])
def test_a_handle_made_under_one_setting_contributes_and_proves_under_another(fid, direction):
    """two handles per form made under A: the first meets B untouched; the second has proved under A, so the call under B drops slots that hold
    A's workspaces and builds B's tables beside what is left of A"""
    old, new = prepare()
    a, b = _flip(fid, direction)
    for form in TC.FORMS:
        made = []
        try:
            with T.options(a):
                made.append(TC.make(old, form, "upload"))
                made.append(TC.make(old, form, "upload"))
                assert made[1].prove_many(TC.BLINDS, [old.w] * 2, in_flight=2) == old.wire, (a, b, form, "under A")
            with T.options(b):
                for k, pr in enumerate(made):
                    contribute_and_prove(pr, old, new, form, (a, b, form, k))
        finally:
            for pr in made:
                pr.close()


# ---- cached knobs: one fresh process per group, without ZK_TEST_FORMS (tests/test_gpu_options.py)
def child_main(group):
    _lib.check(_lib.lib().zk_init(0))
    for k, v in CACHED_GROUPS[group].items():
        T.set_option(k, v)                      # before anything else: they are cached at first use
    run(CACHED_GROUPS[group], CACHED_GROUPS[group])
    print("CACHED-CONTRIBUTE-OK %d" % group)


@pytest.mark.parametrize("group", range(len(CACHED_GROUPS)))
def test_cached_options_in_a_fresh_process(group):
    assert len(CACHED_GROUPS) <= 3
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_contribute_options as M; M.child_main(%d)" % (root, here, group)
    keep = ("ZK_LIBZKMI355X_PATH", "ZK_ORACLE_SO")                  # which build of the library / oracle, not knobs
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZK_") or k in keep}
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert res.returncode == 0 and "CACHED-CONTRIBUTE-OK %d" % group in res.stdout, (CACHED_GROUPS[group], res.stdout[-2000:] + res.stderr[-4000:])
