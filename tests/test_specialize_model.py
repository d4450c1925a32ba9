"""The integer model of zk_groth16_pk_specialize (tests/specialize_model.py) held to the oracle: on a well-formed string the call's linear map gives
the setup of the trapdoor (alpha, beta, 1, 1, tau), exponent for exponent; on the two crafted strings of the issue the key check's model
(tests/key_check_model.py) gives the bits derived by hand.  No GPU: the model is what tests/test_gpu_specialize.py holds the device to where no
honest setup exists."""
import json
import os

import pytest

import key_check_model as KM
import oracle_lib as O
import specialize_cases as SC
import specialize_model as SM
from oracle import pyref as P

R = P.R
FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readme_groth16_key.json")))
CIRCUITS = ["readme", "handbuilt"] + ["cubic%d" % n for n in (1, 2, 3, 5, 8, 13)]
TRAPDOORS = {"random": (SC.ALPHA, SC.BETA, SC.TAU), "tau_in_domain": (SC.ALPHA, SC.BETA, 2), "zeros": (0, 0, SC.TAU), "tau=0": (SC.ALPHA, SC.BETA, 0)}


@pytest.mark.parametrize("name", CIRCUITS)
@pytest.mark.parametrize("trapdoor", list(TRAPDOORS))
def test_an_honest_string_gives_the_oracles_setup(name, trapdoor):
    a, b, t = (x % R for x in TRAPDOORS[trapdoor])
    cs, _ = SC.circuit(name)
    ex1, ex2, vk = SM.specialize_exponents(cs, *SM.honest_string(cs.n, a, b, t))
    want1, want2, want_io = SC.oracle_exponents(name, a, b, t)
    assert ex1 == want1
    assert ex2 == want2
    assert vk["ltgm_io"] == want_io and (vk["one1"], vk["one2"], vk["gm"], vk["d"]) == (1, 1, 1, 1)
    assert KM.key_check_mask(cs, ex1, ex2) == 0 and KM.key_check_mask(cs, ex1, ex2, vk) == 0


def test_the_models_basis_is_an_interpolation_of_its_own():
    """l_i(j) = [i == j] and sum_i l_i = 1, by Horner on the coefficients; Z(j) = 0 on the domain and Z is monic"""
    for n in (1, 2, 5, 8, 13):
        basis = SM.lagrange_coeffs(n)
        horner = lambda c, x: sum(ck * pow(x, k, R) for k, ck in enumerate(c)) % R
        assert all(horner(basis[i], j) == (1 if i == j else 0) for i in range(n) for j in range(n))
        assert [sum(b[k] for b in basis) % R for k in range(n)] == [1] + [0] * (n - 1)
        z = SM.z_coeffs(n)
        assert len(z) == n + 1 and z[n] == 1 and all(horner(z, j) == 0 for j in range(n))
        assert list(z) == KM.z_coeffs(n)


def test_the_golden_readme_key_where_its_trapdoor_permits():
    """The golden key has its own gamma and delta.  a, b1, ti1, b2, ti2 do not depend on them: the model's exponents give the fixture's points.  tiztd
    and ltd_mid are the model's divided by delta: [model exponent / delta] G is the fixture's point.  d1, d2 are delta itself: not comparable."""
    tox = [int(FIX["toxic"][k], 16) for k in ("alpha", "beta", "gamma", "delta", "tau")]
    a, b, _, d, t = tox
    cs, _ = SC.circuit("readme")
    n = cs.n
    ex1, ex2, _ = SM.specialize_exponents(cs, *SM.honest_string(n, a, b, t))
    dinv = pow(d, R - 2, R)
    g1 = lambda e: P.g1_to_bytes(P.pt_mul(P.G1, e)).hex()
    g2 = lambda e: P.g2_to_bytes(P.pt_mul(P.G2, e)).hex()
    free = [0, 2] + list(range(3, 3 + n + 2))
    assert [g1(ex1[i]) for i in free] == [FIX["pk_g1"][i] for i in free]
    assert [g1(ex1[i] * dinv % R) for i in range(5 + n, len(ex1))] == FIX["pk_g1"][5 + n:]
    assert [g2(ex2[i]) for i in [0] + list(range(2, n + 4))] == [FIX["pk_g2"][i] for i in [0] + list(range(2, n + 4))]
    assert (ex1[1], ex2[1]) == (1, 1)


# ---- the two crafted strings: n = 8, masks by hand.  alpha_tau1 enters the [alpha l_i] and nothing else (a = alpha_tau1[0] stays), so only the
# relation L can see it, and it does: the derivation is a dense map, every [alpha l_i] moves, and every variable with an entry in R is a witness.
# tau1[n+3] lies beyond ti1 (n+2 powers) and beyond the n powers the l_i read; tiztd[i] reads it for i + j = n + 3: H_BASES and nothing else.
def test_a_replaced_alpha_power_sets_bit_L():
    cs, _ = SC.circuit("cubic8")
    ex1, ex2, vk = SM.specialize_exponents(cs, *SM.crafted_alpha(8, SC.ALPHA % R, SC.BETA % R, SC.TAU % R))
    assert KM.key_check_mask(cs, ex1, ex2) & KM.L
    assert KM.key_check_mask(cs, ex1, ex2) == KM.L and KM.key_check_mask(cs, ex1, ex2, vk) == KM.L


def test_a_replaced_high_power_sets_exactly_H_BASES():
    cs, _ = SC.circuit("cubic8")
    ex1, ex2, vk = SM.specialize_exponents(cs, *SM.crafted_high_power(8, SC.ALPHA % R, SC.BETA % R, SC.TAU % R))
    assert KM.key_check_mask(cs, ex1, ex2) == KM.H_BASES
    assert KM.key_check_mask(cs, ex1, ex2, vk) == KM.H_BASES


def test_srs_lengths_and_cut():
    from zukelang_amd.groth16 import SRS
    assert [SRS.sizes(n) for n in (1, 2, 3, 4, 8)] == [(3, 1, 3), (4, 2, 4), (5, 3, 5), (7, 4, 6), (15, 8, 10)]
    assert all(SRS.sizes(n) == SM.srs_sizes(n) for n in range(1, 40))
    srs = SC.honest_srs(5)
    cut = srs.cut(3)
    assert (len(cut.tau_g1), len(cut.alpha_tau_g1), len(cut.beta_tau_g1), len(cut.tau_g2)) == (96 * 5, 96 * 3, 96 * 3, 192 * 5)
    assert bytes(cut.tau_g1) == bytes(srs.tau_g1[:96 * 5]) and cut.beta_g2 == srs.beta_g2
    assert bytes(cut.tau_g1) == bytes(SC.honest_srs(3).tau_g1)
    with pytest.raises(ValueError):
        srs.cut(6)
