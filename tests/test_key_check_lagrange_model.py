"""The integer model of zk_groth16_key_check_lagrange (tests/key_check_lagrange_model.py) held to first principles: its honest exponents are what
Groth16.keygen(lagrange=True) uploads, they give mask 0 -- for a tau inside the domain and a circuit with a zero row too -- every crafted key of
tests/key_check_lagrange_cases.py gives the bits derived by hand from the relations, the COMBINED form the device runs gives the per-index mask
under several coefficient draws at every size, and the algebra both rest on (the projection to pi, the extrapolation to sigma, tau l_0(tau) / w_0 =
Z(tau)) is held to direct interpolation (oracle/pyref.py).  No GPU: the model is the specification of tests/test_gpu_key_check_lagrange.py."""
import json
import os
import random

import numpy as np
import pytest

import key_check_lagrange_cases as LC
import key_check_lagrange_model as LM
from oracle import pyref as PR
from zukelang_amd import r1cs as RC
from zukelang_amd.groth16 import _lagrange_at

P = LM.P
FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readme_groth16_key.json")))
TOX = [int(FIX["toxic"][k], 16) for k in ("alpha", "beta", "gamma", "delta", "tau")]


def readme_other():
    """the README circuit with ONE coefficient changed (a mid variable's: `input` in the last gate), same n, m and mids"""
    cs, _ = RC.readme_circuit(3)
    return RC.R1CS(cs.n, cs.m, RC.Matrix.from_rows([{3: 1}, {1: 1}, {2: 1, 3: 2, 0: 3}]), cs.R, cs.O, cs.mid)


def zero_row_circuit():
    """gate 1 has an all-zero row in L and O; variable 5 appears in no gate"""
    L = RC.Matrix.from_rows([{3: 1}, {}, {2: 1, 3: 1, 0: 3}, {1: 2}])
    R = RC.Matrix.from_rows([{3: 1}, {3: 1}, {0: 1}, {0: 1}])
    O = RC.Matrix.from_rows([{1: 1}, {}, {4: 1}, {2: 1}])
    return RC.R1CS(4, 6, L, R, O, np.array([0, 1, 1, 1, 0, 1], dtype=np.uint8))


CS = RC.readme_circuit(3)[0]
CASES = LC.crafted(CS, TOX, readme_other())
SIZES = {
    1: lambda: RC.random_r1cs(1, 4, 9, nnz=(1, 2))[0],
    2: lambda: RC.random_r1cs(2, 6, 11, nnz=(1, 3))[0],
    3: lambda: CS,
    5: lambda: RC.random_r1cs(5, 12, 3, nnz=(1, 3))[0],
    13: lambda: RC.random_r1cs(13, 24, 4, nnz=(8, 8))[0],
}


def test_honest_exponents_are_keygens():
    """l_i(tau), lambda_t(tau) Z(tau) / delta and the rest against keygen's own one-inversion formulas, and against the tau-power model's L_k"""
    for n, make in SIZES.items():
        cs = make()
        lx1, lx2, vk = LM.honest_lagrange_exponents(cs, TOX)
        a, b, gm, d, t = (x % P for x in TOX)
        lag, zt = _lagrange_at(n, t)
        lam, _ = _lagrange_at(n - 1, (t - n) % P)
        ex1, ex2, evk = LM.honest_exponents(cs, TOX)
        assert lx1[:3] == [a, d, b] and lx1[3:3 + n] == lag and lx2 == [b, d] + lag
        assert lx1[3 + n:2 + 2 * n] == [x * zt % P * LM.inv(d) % P for x in lam]
        assert lx1[2 + 2 * n:] == ex1[4 + 2 * n:] and vk == evk


@pytest.mark.parametrize("name,lx1,lx2,vk", CASES, ids=[c[0] for c in CASES])
def test_crafted_keys_give_their_hand_derived_bits(name, lx1, lx2, vk):
    without, with_vk = LC.BITS[name]
    assert LM.lagrange_mask(CS, lx1, lx2) == without, LM.names(LM.lagrange_mask(CS, lx1, lx2))
    assert LM.lagrange_mask(CS, lx1, lx2, vk) == with_vk, LM.names(LM.lagrange_mask(CS, lx1, lx2, vk))


def test_every_case_is_there():
    assert [c[0] for c in CASES] == list(LC.BITS)


def test_honest_keys_that_look_odd_are_well_formed():
    for cs in (CS, SIZES[5](), zero_row_circuit()):
        lx1, lx2, vk = LC.honest_inside_domain(cs, TOX, tau=2)
        assert lx1[3:3 + cs.n] == [0, 0, 1] + [0] * (cs.n - 3) and not any(lx1[3 + cs.n:2 + 2 * cs.n])
        assert LM.lagrange_mask(cs, lx1, lx2) == 0 and LM.lagrange_mask(cs, lx1, lx2, vk) == 0
    cs = zero_row_circuit()
    lx1, lx2, vk = LM.honest_lagrange_exponents(cs, TOX)
    assert LM.lagrange_mask(cs, lx1, lx2) == 0 and LM.lagrange_mask(cs, lx1, lx2, vk) == 0
    cs = SIZES[5]()
    lx1, lx2, vk = LM.honest_lagrange_exponents(cs, TOX[:4] + [cs.n + 1])          # tau inside the shifted domain n..2n-2: hl is a unit vector times Z / delta
    assert LM.lagrange_mask(cs, lx1, lx2, vk) == 0


@pytest.mark.parametrize("n", list(SIZES))
def test_the_combined_form_gives_the_per_index_mask(n):
    cs = SIZES[n]()
    rng = random.Random(0x1A6 + n)
    cases = LC.crafted(cs, TOX, readme_other() if n == 3 else None)
    cases.append(("inside_domain", *LC.honest_inside_domain(cs, TOX, tau=n - 1)))
    for name, lx1, lx2, vk in cases:
        want = (LM.lagrange_mask(cs, lx1, lx2), LM.lagrange_mask(cs, lx1, lx2, vk))
        if n == 3:
            assert want == LC.BITS.get(name, (0, 0)), name
        for _ in range(3):
            rho, r, mu = ([rng.randrange(1 << 254) for _ in range(k)] for k in (n, n, cs.m))
            got = (LM.combined_mask(cs, lx1, lx2, None, rho, r, mu), LM.combined_mask(cs, lx1, lx2, vk, rho, r, mu))
            assert got == want, (name, LM.names(got[1]), LM.names(want[1]))


@pytest.mark.parametrize("n", [2, 3, 5, 13])
def test_pi_has_degree_n_minus_2_and_sigma_are_its_values(n):
    rng = random.Random(0x51 + n)
    basis = PR.lagrange_basis(list(range(n)))
    w = LM.weights(n)
    assert [b[n - 1] if len(b) == n else 0 for b in basis] == w                      # w_i IS the leading coefficient of l_i
    for _ in range(3):
        r = [rng.randrange(P) for _ in range(n)]
        pi = LM.project(n, r)
        assert sum(a * b for a, b in zip(w, pi)) % P == 0
        q = []
        for y, b in zip(pi, basis):
            q = PR.poly_add(q, [y * c % P for c in b])
        assert len(q) <= n - 1                                                        # degree <= n - 2
        assert LM.extrapolate(n, pi) == [PR.poly_eval(q, n + t) for t in range(n - 1)]
        # pi = sum_t sigma_t lambda_t on 0..n-1: the bijection H_BASES leans on
        lam = LM.lambda_table(n)
        sigma = LM.extrapolate(n, pi)
        assert [sum(sigma[t] * lam[t][i] for t in range(n - 1)) % P for i in range(n)] == pi
    # onto: any pi of the hyperplane comes back from r = (n-1)! pi
    pi = [rng.randrange(P) for _ in range(n - 1)]
    pi.append((-sum(a * b for a, b in zip(w, pi)) * LM.inv(w[n - 1])) % P)
    assert LM.project(n, [LM.inv(w[n - 1]) * x % P for x in pi]) == pi
    shifted = PR.lagrange_basis(list(range(n, 2 * n - 1)))
    assert LM.lambda_table(n) == [[PR.poly_eval(b, i) for i in range(n)] for b in shifted]


@pytest.mark.parametrize("n", [2, 3, 5, 13])
def test_the_identities_of_the_h_relation(n):
    t = TOX[4] % P
    lag = LM.basis_at(0, n, t)
    assert sum(lag) % P == 1 and sum(i * x for i, x in enumerate(lag)) % P == t
    assert t * lag[0] % P * LM.inv(LM.weights(n)[0]) % P == LM.z_at(n, t) == PR.poly_eval(PR.z_poly(n), t)
    lam, table = LM.basis_at(n, n - 1, t), LM.lambda_table(n)
    assert [sum(i * table[u][i] * lag[i] for i in range(n)) % P for u in range(n - 1)] == [t * x % P for x in lam]
    pi = LM.project(n, [3 + 5 * i * i for i in range(n)])
    q_at_t = sum(a * b for a, b in zip(pi, lag)) % P
    assert sum(i * a * b for i, (a, b) in enumerate(zip(pi, lag))) % P == t * q_at_t % P          # sum i pi_i l_i(tau) = tau q(tau)
