"""zk_groth16_pk_specialize under every public option.  include/zkmi355x.h promises that no knob of zk_set_option changes a result, and
tests/option_cases.py holds every key, proving and pool call to that promise through its ROUTES table -- by the words in a call's name.  The names of
the specialisation hold none of them on purpose (tests/test_specialize_surface.py), because that table cannot gain a row here; this module keeps the
promise for it, as tests/test_gpu_contribute_options.py does for the contribution: the call derives (ZK_DERIVE_SIDE_BY_SIDE), checks outside points
(ZK_KEY_SUBGROUP_CHECK) and builds both pools' window tables, so it reads what an upload, a derivation and a first proof read.

Every run: specialise the honest string of tests/specialize_cases.py to iterated cubic at n = 64 (196 / 68 points in the reference's format, 194 / 66
in Lagrange form), in both forms, and prove.  Expected: the oracle's key bytes and trapdoor proof of tests/test_gpu_specialize.py, computed once
before any option is set.  The rows of size "ba" get a 4-bit window: 16 buckets, so that the G1 pool's mean of 12 entries per bucket passes the 8 from
which the automatic batch-affine rounds run (csrc/msm.hip: ba_rounds_for)."""
import os
import subprocess
import sys

import pytest

import specialize_cases as SC
import test_gpu_options as T
import test_gpu_specialize as TS
from option_cases import CACHED_GROUPS, FLIPS, live_runs
from zukelang_amd import _lib
from zukelang_amd.groth16 import Groth16

pytestmark = pytest.mark.gpu

NAME = "cubic64"
BA = {"ZK_MSM_WINDOW": "4"}


def prepare():
    _lib.check(_lib.lib().zk_init(0))
    return TS.world(NAME), SC.honest_srs(64)


def specialize(wd, srs, form, tag):
    pr, pk, vk = Groth16.specialize(wd.cs, srs, form=form)
    assert (bytes(pk.g1), bytes(pk.g2)) == (wd.pk1, wd.pk2) and TS.vk_bytes(vk) == (wd.vk1, wd.vk2), (tag, form, "bytes")
    return pr


def run(tag):
    wd, srs = prepare()
    for form in TS.FORMS:
        pr = specialize(wd, srs, form, tag)
        try:
            TS.is_key(pr, wd, form, (tag, form))
        finally:
            pr.close()


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    yield
    _lib.set_device_list([0])


@pytest.mark.parametrize("c,settings", [pytest.param(c, settings, id=rid) for rid, c, settings in live_runs()])
def test_a_live_option_leaves_a_specialised_key_as_the_oracle_has_it(c, settings):
    wd, srs = prepare()
    settings = dict(BA if c.size == "ba" else {}, **settings)
    with T.options(settings):          # ZK_KEY_SUBGROUP_CHECK=0 among them: the string is honest, the same key from points that were not tested
        run(settings)
    if c.multi:          # a device list of two entries offers no handle; the bytes are the same there
        with T.device_list([0, 0]), T.options(settings):
            rc, g1, g2, v1, v2, h = TS.raw(wd.cs, srs, "lagrange", handle=False)
            assert rc == 0 and (g1, g2, v1, v2) == (wd.pk1, wd.pk2, wd.vk1, wd.vk2), (settings, "device list")


def _flip(fid, direction):
    return ({}, FLIPS[fid]) if direction == "set" else (FLIPS[fid], {})


@pytest.mark.parametrize("fid,direction", [pytest.param(fid, d, id="%s-%s" % (fid, d)) for fid in FLIPS for d in ("set", "unset")])
def test_a_handle_made_under_one_setting_proves_under_another(fid, direction):
    wd, srs = prepare()
    a, b = _flip(fid, direction)
    for form in TS.FORMS:
        with T.options(a):
            pr = specialize(wd, srs, form, (a, b))
        try:
            with T.options(b):
                TS.is_key(pr, wd, form, (a, b, form))
        finally:
            pr.close()


# ---- cached knobs: one fresh process per group, without ZK_TEST_FORMS (tests/test_gpu_options.py)
def child_main(group):
    _lib.check(_lib.lib().zk_init(0))
    for k, v in CACHED_GROUPS[group].items():
        T.set_option(k, v)                      # before anything else: they are cached at first use
    run(CACHED_GROUPS[group])
    print("CACHED-SPECIALIZE-OK %d" % group)


@pytest.mark.parametrize("group", range(len(CACHED_GROUPS)))
def test_cached_options_in_a_fresh_process(group):
    assert len(CACHED_GROUPS) <= 3
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_specialize_options as M; M.child_main(%d)" % (root, here, group)
    keep = ("ZK_LIBZKMI355X_PATH", "ZK_ORACLE_SO")                  # which build of the library / oracle, not knobs
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZK_") or k in keep}
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert res.returncode == 0 and "CACHED-SPECIALIZE-OK %d" % group in res.stdout, (CACHED_GROUPS[group], res.stdout[-2000:] + res.stderr[-4000:])
