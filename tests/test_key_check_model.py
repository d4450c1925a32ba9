"""The key check's integer model (tests/key_check_model.py) held to the golden README key: the honest exponents of its toxic waste ARE the
fixture's points (first-principles double-and-add, oracle/pyref.py), they give mask 0, and every crafted key of tests/key_check_cases.py gives the
bits derived by hand from the relations.  No GPU: the model is the specification the device is held to in tests/test_gpu_key_check.py."""
import json
import os

import pytest

import key_check_cases as KC
import key_check_model as KM
from oracle import pyref as P
from zukelang_amd import r1cs as RC

FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readme_groth16_key.json")))
TOX = [int(FIX["toxic"][k], 16) for k in ("alpha", "beta", "gamma", "delta", "tau")]


def readme_other():
    """the README circuit with ONE coefficient changed (a mid variable's: `input` in the last gate), same n, m and mids"""
    cs, _ = RC.readme_circuit(3)
    L = RC.Matrix.from_rows([{3: 1}, {1: 1}, {2: 1, 3: 2, 0: 3}])
    return RC.R1CS(cs.n, cs.m, L, cs.R, cs.O, cs.mid)


CS = RC.readme_circuit(3)[0]
CASES = KC.crafted(CS, TOX, readme_other())


def test_honest_exponents_are_the_golden_key():
    ex1, ex2, _ = KM.honest_exponents(CS, TOX)
    assert [P.g1_to_bytes(P.pt_mul(P.G1, e)).hex() for e in ex1] == FIX["pk_g1"]
    assert [P.g2_to_bytes(P.pt_mul(P.G2, e)).hex() for e in ex2] == FIX["pk_g2"]


def test_basis_dots_interpolate():
    """<e, l_g> against Lagrange interpolation in pyref: with e = the powers of x, the dot is l_g(x)"""
    for n in (1, 2, 5, 8):
        x = 0xABCDEF + n
        e = [pow(x, j, P.R) for j in range(n)]
        basis = P.lagrange_basis(list(range(n)))
        assert KM.basis_dots(n, e) == [P.poly_eval(b, x) for b in basis]
        assert KM.z_coeffs(n) == (P.z_poly(n) + [0] * (n + 1))[:n + 1]


@pytest.mark.parametrize("name,ex1,ex2,vk", CASES, ids=[c[0] for c in CASES])
def test_crafted_keys_give_their_hand_derived_bits(name, ex1, ex2, vk):
    without, with_vk = KC.BITS[name]
    assert KM.key_check_mask(CS, ex1, ex2) == without, KM.names(KM.key_check_mask(CS, ex1, ex2))
    assert KM.key_check_mask(CS, ex1, ex2, vk) == with_vk, KM.names(KM.key_check_mask(CS, ex1, ex2, vk))


def test_every_case_of_the_issue_is_there():
    assert [c[0] for c in CASES] == list(KC.BITS)


def test_a_consistent_vkey_of_another_gamma_is_a_partner():
    """the proving key holds no gamma: a verification key made with another gamma throughout (gm AND ltgm_io) verifies this key's proofs"""
    ex1, ex2, _ = KM.honest_exponents(CS, TOX)
    _, _, vk2 = KM.honest_exponents(CS, TOX[:2] + [TOX[2] + 5] + TOX[3:])
    assert KM.key_check_mask(CS, ex1, ex2, vk2) == 0
    vk2["gm"] = 0
    assert KM.key_check_mask(CS, ex1, ex2, vk2) & KM.GAMMA


def test_generators():
    ex1, ex2, vk = KM.honest_exponents(CS, TOX)
    e1 = list(ex1)
    e1[3] = 2
    assert KM.key_check_mask(CS, e1, ex2) & KM.GENERATORS
    assert KM.key_check_mask(CS, ex1, ex2, dict(vk, one2=2)) == KM.GENERATORS
