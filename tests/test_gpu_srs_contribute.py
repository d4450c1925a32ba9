"""zk_groth16_srs_contribute on the device against the oracle and the integer model (tests/srs_model.py): a contributed honest string is, byte for
byte, the oracle's string of the product trapdoor; a crafted string comes out as the model's map of it; links are the oracle's points of the model's
exponents and verify as a chain; and once, on iterated cubic at n = 5, the whole route from a string to a proof."""
import ctypes as C

import numpy as np
import pytest

import specialize_cases as SC
import specialize_model as SM
import srs_cases as S
import srs_model as M
import test_gpu_options as T
import test_gpu_specialize as TS
import oracle_lib as O
from zukelang_amd import _lib
from zukelang_amd import groth16 as G
from zukelang_amd.groth16 import SRS, Groth16, _p

pytestmark = pytest.mark.gpu

R = S.R
ARG, NOT_ON_CURVE, RANGE, DOMAIN = -1, -2, -3, -8
SEED = bytes(range(32))
AM, BM, TM = S.MUL


@pytest.fixture(autouse=True)
def _init_and_leave_nothing_behind():
    _lib.check(_lib.lib().zk_init(0))
    yield
    _lib.set_device_list([0])


def _kbytes(mul):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in mul), dtype=np.uint8).copy()


def raw(srs, mul, in_place=False, links=True):
    """the C call itself: (status, out_g1, out_g2, link_g1, link_g2); the outputs are 0x5a-filled beforehand, or the inputs' own memory"""
    s1, n1, nab, s2, n2 = srs._lists("raw")
    s1, s2 = s1.copy(), s2.copy()
    o1, o2 = (s1, s2) if in_place else (np.full(len(s1), 0x5A, dtype=np.uint8), np.full(len(s2), 0x5A, dtype=np.uint8))
    l1, l2 = np.full(6 * 96, 0x5A, dtype=np.uint8), np.full(3 * 192, 0x5A, dtype=np.uint8)
    rc = _lib.lib().zk_groth16_srs_contribute(_p(s1), n1, nab, _p(s2), n2, _p(_kbytes(mul)), _p(o1), _p(o2), _p(l1) if links else None, _p(l2) if links else None)
    return rc, bytes(o1), bytes(o2), bytes(l1), bytes(l2)


def flat(srs):
    s1, _, _, s2, _ = srs._lists("flat")
    return bytes(s1), bytes(s2)


def link_bytes(ex, mul):
    """the link of contributing `mul` to the string of exponents `ex`, as the oracle's points of the model's exponents"""
    after = M.contributed(*ex, *mul)
    g1, g2 = M.link(ex[0], ex[1], ex[2], after, *mul)
    return O.points_of_exponents_g1(SC.frs(g1)), O.points_of_exponents_g2(SC.frs(g2))


# ---------------------------------------------------------------- honest strings: the string of the product trapdoor
def _honest_cases():
    return [SM.srs_sizes(n) for n in (1, 2, 5, 64)] + list(S.HONEST_FREE[:2])


@pytest.mark.parametrize("lens", _honest_cases(), ids=lambda t: "%dx%dx%d" % t)
def test_a_contributed_honest_string_is_the_oracles_string_of_the_product_trapdoor(lens):
    ex = M.honest(*lens, S.ALPHA, S.BETA, S.TAU)
    srs = S.honest_srs(*lens)
    want = flat(S.honest_srs(*lens, S.ALPHA * AM % R, S.BETA * BM % R, S.TAU * TM % R))
    want_link = link_bytes(ex, S.MUL)
    for in_place in (False, True):
        rc, o1, o2, l1, l2 = raw(srs, S.MUL, in_place)
        assert rc == 0, _lib.lib().zk_last_error()
        assert (o1, o2) == want, (lens, in_place)
        assert (l1, l2) == want_link, (lens, in_place, "link")
    rc, o1, o2, l1, l2 = raw(srs, S.MUL, links=False)
    assert rc == 0 and (o1, o2) == want and set(l1 + l2) == {0x5A}
    new, link = srs.contribute(S.MUL)
    assert flat(new) == want and link.tau_before + link.tau_after + link.alpha_before + link.alpha_after + link.beta_before + link.beta_after == want_link[0]
    assert link.tau_g2 + link.alpha_g2 + link.beta_g2 == want_link[1]


def test_unit_factors_return_the_inputs_bytes():
    for srs in (S.honest_srs(S.N1, S.NAB, S.N2), S.crafted_srs("cancelling"), S.honest_srs(S.N1, S.NAB, S.N2, S.ALPHA, S.BETA, 0)):
        rc, o1, o2, l1, l2 = raw(srs, (1, 1, 1))
        assert rc == 0 and (o1, o2) == flat(srs)
        assert l1[:96] == l1[96:192] and l1[192:288] == l1[288:384] and l1[384:480] == l1[480:] and l2 == O.g2_generator() * 3


def test_tau_factor_r_minus_1_and_full_width_factors():
    lens = (S.N1, S.NAB, S.N2)
    for mul in ((1, 1, R - 1), (R - 1, R - 1, R - 1), (R - 2, (R + 1) // 2, R - 3)):
        rc, o1, o2, l1, l2 = raw(S.honest_srs(*lens), mul)
        a, b, t = (S.ALPHA * mul[0] % R, S.BETA * mul[1] % R, S.TAU * mul[2] % R)
        assert rc == 0 and (o1, o2) == flat(S.honest_srs(*lens, a, b, t)), mul
        assert (l1, l2) == link_bytes(M.honest(*lens, S.ALPHA, S.BETA, S.TAU), mul), mul


def test_a_tau_0_string_keeps_its_identities():
    lens = (S.N1, S.NAB, S.N2)
    srs = S.honest_srs(*lens, S.ALPHA, S.BETA, 0)
    new, link = srs.contribute(S.MUL)
    assert flat(new) == flat(S.honest_srs(*lens, S.ALPHA * AM % R, S.BETA * BM % R, 0))
    ident = O.points_of_exponents_g1(SC.frs([0]))
    assert bytes(new.tau_g1[96:]) == ident * (S.N1 - 1) and link.tau_before == link.tau_after == ident
    assert new.check(seed=SEED).failed == M.TRIVIAL


@pytest.mark.parametrize("name", ["last_tau1", "first_pair_tau1", "generator_g2", "cancelling", "other_beta"])
def test_a_crafted_string_comes_out_as_the_models_map_with_the_models_mask(name):
    ex = S.crafted(name)
    after = M.contributed(*ex, *S.MUL)
    new, link = S.crafted_srs(name).contribute(S.MUL)
    assert flat(new) == flat(SC.srs_of_exponents(*after)), name
    want = M.mask(*after)
    assert want == S.CRAFTED[name][1]
    assert new.check(seed=SEED).failed == want


# ---------------------------------------------------------------- links
def test_links_verify_and_chains_hold_together():
    s0 = S.honest_srs(S.N1, S.NAB, S.N2)
    s1, l1 = s0.contribute(S.MUL)
    s2, l2 = s1.contribute((5, 7, 11))
    assert G.verify_srs_contributions(s0, [l1], s1)
    assert G.verify_srs_contributions(s0, [l1, l2], s2)
    assert G.verify_srs_contributions(s0.link_points(), [l1, l2], s2.link_points())
    assert G.verify_srs_contributions(s0, [], s0)
    assert not G.verify_srs_contributions(s0, [l1], s2)                 # ends elsewhere
    assert not G.verify_srs_contributions(s0, [l2], s2)                 # a gap: l2 does not start at s0
    assert not G.verify_srs_contributions(s0, [l1, l1], s1)
    assert not G.verify_srs_contributions(s1, [l1, l2], s2)
    fields = ("tau_before", "tau_after", "alpha_before", "alpha_after", "beta_before", "beta_after", "tau_g2", "alpha_g2", "beta_g2")
    for i, f in enumerate(fields):          # one point swapped for the same point of the other link, the chain's ends adjusted to it
        bad = G.SRSContribution(**dict(l1.__dict__, **{f: getattr(l2, f)}))
        first = tuple(getattr(bad, k) for k in fields[0:6:2])
        last = tuple(getattr(bad, k) for k in fields[1:6:2])
        assert not G.verify_srs_contributions(first, [bad], last), f
    # the factors went to the right places: the G2 points are [tau']_2, [alpha']_2, [beta']_2
    assert l1.tau_g2 + l1.alpha_g2 + l1.beta_g2 == O.points_of_exponents_g2(SC.frs([TM, AM, BM]))


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("which", TS.LISTS)
def test_a_bad_point_in_any_list_refuses_the_call_and_writes_nothing(which):
    srs = SC.honest_srs(5)
    for kind, want in (("curve", NOT_ON_CURVE), ("torsion", NOT_ON_CURVE), ("encoding", ARG)):
        rc, o1, o2, l1, l2 = raw(TS._with_point(srs, which, TS._bad(which, kind)), S.MUL)
        assert rc == want and set(o1 + o2 + l1 + l2) == {0x5A}, (which, kind, rc)
    a = TS._with_point(TS._with_point(srs, "tau_g1", TS._bad("tau_g1", "encoding")), "tau_g2", TS._bad("tau_g2", "curve"))
    assert raw(a, S.MUL)[0] == ARG
    with pytest.raises(ValueError):
        TS._with_point(srs, which, TS._bad(which, "curve")).contribute(S.MUL)


def test_the_subgroup_option_is_honoured_here():
    srs = TS._with_point(SC.honest_srs(5), "tau_g1", TS._bad("tau_g1", "torsion"))
    assert raw(srs, S.MUL)[0] == NOT_ON_CURVE
    with T.options({"ZK_KEY_SUBGROUP_CHECK": "0"}):
        rc, o1, o2, l1, l2 = raw(srs, S.MUL)
        assert rc == 0 and set(o1) != {0x5A}
        rc, h1, h2, _, _ = raw(SC.honest_srs(5), S.MUL)
        assert rc == 0 and (h1, h2) == flat(S.honest_srs(*SM.srs_sizes(5), S.ALPHA * AM % R, S.BETA * BM % R, S.TAU * TM % R))
        assert (o1[:96 * 8], o1[96 * 9:], o2) == (h1[:96 * 8], h1[96 * 9:], h2)          # every other point is the honest one


def test_factors_lengths_and_a_device_list_of_two_are_refused():
    srs = SC.honest_srs(5)
    for mul, want in (((0, 1, 1), ARG), ((1, 1, 0), ARG), ((R, 1, 1), RANGE), ((1, R + 5, 1), RANGE)):
        rc, o1, o2, l1, l2 = raw(srs, mul)
        assert rc == want and set(o1 + o2 + l1 + l2) == {0x5A}, mul
    short = SRS(srs.tau_g1[:96 * 4], srs.alpha_tau_g1, srs.beta_tau_g1, srs.beta_g2, srs.tau_g2[:192 * 4])          # NAB = 5 > N1 = 4
    assert raw(short, S.MUL)[0] == DOMAIN
    with T.device_list([0, 0]):
        rc, o1, o2, l1, l2 = raw(srs, S.MUL)
        assert rc == ARG and set(o1 + o2 + l1 + l2) == {0x5A}


# ---------------------------------------------------------------- the whole route
@pytest.mark.parametrize("form", TS.FORMS)
def test_from_a_string_to_a_proof(form):
    """check, contribute, check, specialize, contribute, check_key: mask 0 at every station, and the key is the oracle's setup of the product trapdoor"""
    srs = SC.honest_srs(5)
    assert srs.check(seed=SEED).ok
    new, link = srs.contribute(S.MUL)
    assert new.check(seed=SEED).ok and G.verify_srs_contributions(srs, [link], new)
    wd1 = TS.world("cubic5", 1, S.ALPHA * AM % R, S.BETA * BM % R, S.TAU * TM % R)
    wd = TS.world("cubic5", TS.DMUL, S.ALPHA * AM % R, S.BETA * BM % R, S.TAU * TM % R)
    pr, pk, vk = Groth16.specialize(wd.cs, new, form=form)
    try:
        assert (bytes(pk.g1), bytes(pk.g2)) == (wd1.pk1, wd1.pk2) and TS.vk_bytes(vk) == (wd1.vk1, wd1.vk2)
        con = pr.contribute(TS.DMUL)
        vk2 = vk.with_delta(con.vk_d)
        assert TS.vk_bytes(vk2) == (wd.vk1, wd.vk2)
        assert TS.check(pr, form, vk2).failed == 0
        TS.is_key(pr, wd, form, ("route", form))
    finally:
        pr.close()
