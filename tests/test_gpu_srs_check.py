"""zk_groth16_srs_check on the device against the integer model (tests/srs_model.py) and the table of crafted strings (tests/srs_cases.py).  Nothing
that is expected comes from the library under test: strings are [exponent] G through the oracle's multiplication, masks the model's five predicates
(held to the masks written out in the table by tests/test_srs_model.py).  Every string is at most a few hundred points."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import specialize_cases as SC
import specialize_model as SM
import srs_cases as S
import srs_model as M
import test_gpu_options as T
import test_gpu_specialize as TS
from zukelang_amd import _lib
from zukelang_amd.groth16 import SRS, _p

pytestmark = pytest.mark.gpu

ARG, NOT_ON_CURVE = -1, -2
SEEDS = (bytes(range(32)), bytes(range(200, 232)))
UNTOUCHED = 0x5A5A5A5A


@pytest.fixture(autouse=True)
def _init_and_leave_nothing_behind():
    _lib.check(_lib.lib().zk_init(0))
    yield
    _lib.set_device_list([0])


def raw(srs, seed=SEEDS[0]):
    """the C call itself: (status, *failed), *failed set to a marker beforehand"""
    s1, n1, nab, s2, n2 = srs._lists("raw")
    failed = C.c_uint32(UNTOUCHED)
    sd = None if seed is None else _p(np.frombuffer(seed, dtype=np.uint8))
    rc = _lib.lib().zk_groth16_srs_check(_p(s1), n1, nab, _p(s2), n2, sd, C.byref(failed))
    return rc, failed.value


def masks(srs):
    """the verdict under two seeds and under a seed the library draws"""
    out = []
    for seed in SEEDS + (None,):
        rc, f = raw(srs, seed)
        assert rc == 0, (rc, _lib.lib().zk_last_error())
        out.append(f)
    return out


# ---------------------------------------------------------------- honest strings
@pytest.mark.parametrize("n", S.HONEST_N)
def test_an_honest_string_of_a_circuits_sizes_holds(n):
    assert masks(SC.honest_srs(n)) == [0, 0, 0]
    v = SC.honest_srs(n).check(seed=SEEDS[0])
    assert v.ok and v.names == [] and SC.honest_srs(n).check().ok


@pytest.mark.parametrize("lens", S.HONEST_FREE, ids=lambda t: "%dx%dx%d" % t)
def test_an_honest_string_of_free_lengths_holds(lens):
    assert masks(S.honest_srs(*lens)) == [0, 0, 0]


# ---------------------------------------------------------------- crafted strings: a verdict, not an error
@pytest.mark.parametrize("name", sorted(S.CRAFTED))
def test_a_crafted_string_gets_the_models_mask(name):
    want = M.mask(*S.crafted(name))
    assert want == S.CRAFTED[name][1] and want != 0
    assert masks(S.crafted_srs(name)) == [want] * 3, name
    v = S.crafted_srs(name).check(seed=SEEDS[1])
    assert not v.ok and v.failed == want and v.names == [M.NAMES[b] for b in sorted(M.NAMES) if want & b]


@pytest.mark.parametrize("name", sorted(S.DEGENERATE))
def test_degenerate_trapdoors(name):
    (a, b, t), want = S.DEGENERATE[name]
    for lens in ((S.N1, S.NAB, S.N2), (2, 1, 2)):
        assert M.mask(*M.honest(*lens, a, b, t)) == want
        assert masks(S.honest_srs(*lens, a, b, t)) == [want] * 3, (name, lens)


def test_an_all_zero_string_is_a_string_of_identities():
    srs = SRS(np.zeros(96 * 5, dtype=np.uint8), np.zeros(96 * 3, dtype=np.uint8), np.zeros(96 * 3, dtype=np.uint8), bytes(192), np.zeros(192 * 4, dtype=np.uint8))
    assert masks(srs) == [M.GENERATORS | M.TRIVIAL] * 3


def test_a_relation_without_an_index_holds():
    t1, a1, b1, b2, t2 = M.honest(4, 1, 2, S.ALPHA, S.BETA, S.TAU)
    assert masks(SC.srs_of_exponents(t1, [12345], b1, b2, t2)) == [0, 0, 0]


@pytest.mark.parametrize("which,want", [("alpha", M.ALPHA), ("high_power", M.TAU_G1)])
def test_the_specialisations_failing_strings_are_named_by_the_string(which, want):
    craft = SM.crafted_alpha if which == "alpha" else SM.crafted_high_power
    ex = craft(8, S.ALPHA, S.BETA, S.TAU)
    assert M.mask(*ex) == want
    assert masks(SC.srs_of_exponents(*ex)) == [want] * 3


# ---------------------------------------------------------------- bad points: a status, *failed untouched
@pytest.mark.parametrize("which", TS.LISTS)
def test_a_bad_point_in_any_list_is_a_status(which):
    srs = SC.honest_srs(5)
    for kind, want in (("curve", NOT_ON_CURVE), ("torsion", NOT_ON_CURVE), ("encoding", ARG)):
        for at in (0, -1):
            assert raw(TS._with_point(srs, which, TS._bad(which, kind), at)) == (want, UNTOUCHED), (which, kind, at)
    with pytest.raises(ValueError):
        TS._with_point(srs, which, TS._bad(which, "curve")).check()


def test_the_first_bad_list_decides():
    srs = SC.honest_srs(5)
    L = TS.LISTS
    for i in range(len(L)):
        for j in range(i + 1, len(L)):
            a = TS._with_point(TS._with_point(srs, L[i], TS._bad(L[i], "curve")), L[j], TS._bad(L[j], "encoding"))
            assert raw(a) == (NOT_ON_CURVE, UNTOUCHED), (L[i], L[j])
            b = TS._with_point(TS._with_point(srs, L[i], TS._bad(L[i], "encoding")), L[j], TS._bad(L[j], "torsion"))
            assert raw(b) == (ARG, UNTOUCHED), (L[i], L[j])


@pytest.mark.parametrize("setting", [None, "0", "1"])
def test_torsion_points_are_refused_whatever_the_option_says(setting):
    """every point of tests/golden/torsion_points.json that lies on its curve outside the subgroup, in every list of its group"""
    srs = SC.honest_srs(5)
    with T.options({} if setting is None else {"ZK_KEY_SUBGROUP_CHECK": setting}):
        for group, lists in ((0, TS.LISTS[:3]), (1, TS.LISTS[3:])):
            pts = [bytes.fromhex(t["hex"]) for t in json.load(open(os.path.join(TS.GOLDEN, "torsion_points.json")))["points"]
                   if t["group"] == group and (t["what"].startswith("torsion") or t["what"] == "random curve point")]
            assert len(pts) == 12
            for k, pt in enumerate(pts):
                which = lists[k % len(lists)]
                assert raw(TS._with_point(srs, which, pt, 0 if which == "beta_g2" else 1)) == (NOT_ON_CURVE, UNTOUCHED), (setting, group, k)
        assert raw(srs) == (0, 0)


def test_a_device_list_of_two_is_refused():
    with T.device_list([0, 0]):
        assert raw(SC.honest_srs(5)) == (ARG, UNTOUCHED)
