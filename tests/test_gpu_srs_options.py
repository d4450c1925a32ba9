"""zk_groth16_srs_check and zk_groth16_srs_contribute under every public option.  include/zkmi355x.h promises that no knob of zk_set_option changes a
result, and tests/option_cases.py holds every key, proving and pool call to that promise through its ROUTES table -- by the words in a call's name.
The names of the string calls hold none of them on purpose (tests/test_srs_surface.py), because that table cannot gain a row here; this module keeps
the promise for them, as tests/test_gpu_specialize_options.py does for the specialisation: the check builds base sets, sorts, accumulates and
reduces on the Pippenger chain (the window, sort and tail knobs), the contribution checks outside points (ZK_KEY_SUBGROUP_CHECK) and multiplies on the
derivation's kernels.

Every run: the crafted string "cancelling" (12 / 6 / 8 points) through the check, the honest string of 127 / 64 / 66 points (a circuit of 64
constraints) and the crafted one through the contribution.  Expected: the table's mask, the oracle's string of the product trapdoor and the model's
map -- computed before any option is set, never by the library.  The default setting's verdicts on every other string are
tests/test_gpu_srs_check.py's."""
import os
import subprocess
import sys

import pytest

import specialize_cases as SC
import specialize_model as SM
import srs_cases as S
import srs_model as M
import test_gpu_options as T
import test_gpu_srs_contribute as TC
from option_cases import CACHED_GROUPS, live_runs
from zukelang_amd import _lib

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
CRAFTED = ("cancelling",)
BA = {"ZK_MSM_WINDOW": "4"}
R = S.R


def prepare():
    _lib.check(_lib.lib().zk_init(0))
    lens = SM.srs_sizes(64)
    am, bm, tm = S.MUL
    want = TC.flat(S.honest_srs(*lens, S.ALPHA * am % R, S.BETA * bm % R, S.TAU * tm % R))
    crafted_after = TC.flat(SC.srs_of_exponents(*M.contributed(*S.crafted("cancelling"), *S.MUL)))
    return S.honest_srs(*lens), want, crafted_after, [S.crafted_srs(name) for name in CRAFTED]


def run(tag):
    honest, want, crafted_after, crafted = prepare()
    # ONE check per run (a 22-bit window without tables is 12 x 2^21 buckets per sum, seconds per call): the string whose two errors cancel under
    # equal coefficients -- TAU_G1 must differ, and ALPHA, BETA, TAU_G2, which its errors do not touch, must hold as on the honest string
    for name, srs in zip(CRAFTED, crafted):
        assert srs.check(seed=SEED).failed == S.CRAFTED[name][1] == M.TAU_G1, (tag, name)
    new, _ = honest.contribute(S.MUL)
    assert TC.flat(new) == want, (tag, "contributed")
    new, _ = crafted[0].contribute(S.MUL)
    assert TC.flat(new) == crafted_after, (tag, "contributed crafted")


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    yield
    _lib.set_device_list([0])


@pytest.mark.parametrize("c,settings", [pytest.param(c, settings, id=rid) for rid, c, settings in live_runs()])
def test_a_live_option_leaves_verdicts_and_contributed_strings_as_they_are(c, settings):
    settings = dict(BA if c.size == "ba" else {}, **settings)
    with T.options(settings):          # ZK_KEY_SUBGROUP_CHECK=0 among them: the check tests the subgroup all the same, the strings are honest
        run(settings)


# ---- cached knobs: one fresh process per group, without ZK_TEST_FORMS (tests/test_gpu_options.py)
def child_main(group):
    _lib.check(_lib.lib().zk_init(0))
    for k, v in CACHED_GROUPS[group].items():
        T.set_option(k, v)                      # before anything else: they are cached at first use
    run(CACHED_GROUPS[group])
    print("CACHED-SRS-OK %d" % group)


@pytest.mark.parametrize("group", range(len(CACHED_GROUPS)))
def test_cached_options_in_a_fresh_process(group):
    assert len(CACHED_GROUPS) <= 3
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_srs_options as M; M.child_main(%d)" % (root, here, group)
    keep = ("ZK_LIBZKMI355X_PATH", "ZK_ORACLE_SO")                  # which build of the library / oracle, not knobs
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZK_") or k in keep}
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert res.returncode == 0 and "CACHED-SRS-OK %d" % group in res.stdout, (CACHED_GROUPS[group], res.stdout[-2000:] + res.stderr[-4000:])
