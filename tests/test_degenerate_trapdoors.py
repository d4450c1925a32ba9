"""Degenerate trapdoors without a GPU (tests/degenerate_cases.py: the table): the host keygen's Lagrange basis against the plain product formula at
every point of the domain and of the shifted domain, and the oracle's trapdoor shortcuts -- what the GPU suite trusts at sizes the literal oracle
cannot reach -- against its literal half on every row of the table.  Before the unit-vector branch of groth16._lagrange_at and of
oracle/zk_oracle.c: lagrange_at, the first two tests here fail at every tau in 0 .. n-1 (the batch inversion inverts a product that holds tau - tau).

The Pinocchio trapdoor proof at Z(s) = 0 RAISES (oracle_lib.pinocchio_prove_trapdoor: ValueError): h(s) = (v w - y)(s) / Z(s) is 0 / 0 there."""
import pytest

import degenerate_cases as D
import oracle_lib as O
from zukelang_amd.groth16 import _lagrange_at

R = D.R
frb, frs, csrs = D.frb, D.frs, D.csrs


# ---- the host keygen's basis
@pytest.mark.parametrize("n", [1, 2, 3, 6, 24])
def test_lagrange_at_matches_the_product_formula_at_every_point(n):
    xs = list(range(2 * n)) + [R - 1, D.draws("gate1", "lagrange", 1, 1)[0][0] + n]
    for x in xs:
        lag, z = _lagrange_at(n, x)
        want, zw = D.lagrange_ref(n, 0, x)
        assert (tuple(lag), z) == (want, zw), (n, x)
        if x < n:
            assert z == 0 and lag == [int(i == x) for i in range(n)]
        lam, zl = _lagrange_at(n - 1, (x - n) % R)          # the shifted call of Groth16.keygen: the basis of the points n .. 2n-2, at x
        want, zw = D.lagrange_ref(n - 1, n, x)
        assert (tuple(lam), zl) == (want, zw), ("shifted", n, x)
        if n <= x < 2 * n - 1:
            assert zl == 0 and lam == [int(i == x - n) for i in range(n - 1)]


# ---- the oracle's trapdoor forms against its literal half
def _groth16_rows(name):
    keep = None if name in D.SMALL else {"tau=0", "tau=n-1", "tau=n", "tau=r-1"}
    return [(name, label) for label, _ in D.groth16_rows(name) if keep is None or label in keep]


def _pinocchio_rows(name):
    keep = None if name in D.SMALL else {"s=0", "s=n-1", "s=n", "s=r-1"}
    return [(name, label) for label, _ in D.pinocchio_rows(name) if keep is None or label in keep]


@pytest.mark.parametrize("name,label", [c for name in D.LITERAL for c in _groth16_rows(name)])
def test_groth16_trapdoor_forms_equal_the_literal_forms(name, label):
    cs, w = D.circuit(name)
    tox = D.row(D.groth16_rows, name, label)
    pk1, pk2, vk1, vk2 = D.groth16_key(name, tox)                                       # orc_groth16_setup: Poly.apply on the dense QAP
    e1, e2, eio = O.groth16_setup_exponents(cs.n, cs.m, *csrs(cs), cs.mid, frs(tox))
    assert O.points_of_exponents_g1(e1) == pk1, "pk g1"
    assert O.points_of_exponents_g2(e2) == pk2, "pk g2"
    assert O.g1_generator() + O.points_of_exponents_g1(eio) == vk1, "vkey io"
    r1, r2, rio, _l1, _l2 = D.groth16_exponents_ref(name, tox)                          # and both against the product formula
    assert (frs(r1), frs(r2), frs(rio)) == (e1, e2, eio)
    (r, s), = D.draws(name, label, 1)
    q = D.qap(name)
    rc, a, b, c = q.groth16_prove(pk1, pk2, cs.mid, frs(w), frb(r), frb(s), literal=1)   # per variable, groth16.ml:116-121
    assert rc == 0
    assert O.groth16_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, frs(w), frs(tox), frb(r), frb(s)) == (a, b, c)
    assert D.groth16_proof(name, tox, r, s) == (a, b, c)                                # what the GPU module expects (literal = 0 at n = 64)


@pytest.mark.parametrize("name,label", [c for name in D.LITERAL for c in _pinocchio_rows(name)])
def test_pinocchio_trapdoor_forms_equal_the_literal_forms(name, label):
    cs, w = D.circuit(name)
    tox = D.row(D.pinocchio_rows, name, label)
    q = D.qap(name)
    lit = O.pinocchio_keygen_exponents(q, cs.n, cs.m, *csrs(cs), cs.mid, frs(tox), True)
    assert O.pinocchio_keygen_exponents(None, cs.n, cs.m, *csrs(cs), cs.mid, frs(tox), False) == lit
    d, = D.draws(name, label, 1, 3)
    args = (cs.n, cs.m, *csrs(cs), cs.mid, frs(w), frs(tox), *(frb(x) for x in d))
    if D.in_domain(name, tox[D.PIN["s"]]):
        with pytest.raises(ValueError):
            O.pinocchio_prove_trapdoor(*args)
        out = (O.C.c_uint8 * 960)(*([0xA5] * 960))                                      # the raw call: its status, and not one byte written
        assert O.lib.orc_pinocchio_prove_trapdoor(*args[:2], *(x for M in args[2:5] for x in M.args()), O._b(bytes(cs.mid)), *(O._b(x) for x in args[6:]), out) == -4
        assert bytes(out) == b"\xa5" * 960
    else:
        assert O.pinocchio_prove_trapdoor(*args) == D.pinocchio_proof(name, tox, d)      # ZKCompute.f, literal, on the literal key's points


# ---- the table itself
@pytest.mark.parametrize("name", D.CIRCUITS)
def test_the_table_holds_what_it_says(name):
    n = D.n_of(name)
    cs, w = D.circuit(name)
    assert cs.n == n
    taus = D.tau_values(name)
    assert len({v for _, v in taus}) == len(taus) == len({label for label, _ in taus})   # distinct field elements after the drops
    assert all(0 <= v < R for _, v in taus)
    want = {0, n - 1, 2 * n - 2, R - 1} if n == 1025 else {0, 1, 2, n - 1, n, 2 * n - 2, 2 * n - 1, R - 1, D.I4}
    assert {v for _, v in taus} == {v % R for v in want}                                # nothing dropped but a coincidence
    assert pow(D.I4, 4, R) == 1 and pow(D.I4, 2, R) != 1
    for rows, names, key in ((D.groth16_rows(name), D.G16, "tau"), (D.pinocchio_rows(name), D.PIN, "s")):
        assert len({label for label, _ in rows}) == len(rows) == len({t for _, t in rows})
        for label, tox in rows:
            assert len(tox) == len(names) and all(0 <= x < R for x in tox)
            changed = {k for k, i in names.items() if tox[i] != D._base(name, len(names))[i]}
            assert changed == set(label.split("=")[:-1]), label                          # "alpha=beta=0" replaces alpha and beta and nothing else
        assert [label for label, _ in rows if label.startswith(key + "=")] == [key + "=" + t for t, _ in taus if n != 1025 or key == "tau" or t in ("2n-2", "r-1")]
    if name == "random1025":
        assert [label for label, _ in D.pinocchio_rows(name)] == ["s=2n-2", "s=r-1"]       # no oracle serves s inside the domain at this size


@pytest.mark.parametrize("name", D.LITERAL)
def test_the_blinding_that_zeroes_a_and_b_does(name):
    cs, w = D.circuit(name)
    for label in ("tau=0", "tau=r-1", "alpha=beta=0"):
        tox = D.row(D.groth16_rows, name, label)
        (tag, (r, s)), zero, minus = D.blindings(name, tox)
        assert tag == "A=B=identity" and zero[1] == (0, 0) and minus[1] == (R - 1, R - 1)
        pk1, pk2, _, _ = D.groth16_key(name, tox)
        rc, a, b, _c = D.qap(name).groth16_prove(pk1, pk2, cs.mid, frs(w), frb(r), frb(s), literal=name in D.SMALL)
        assert rc == 0 and a == D.IDENT1 and b == D.IDENT2, (name, label)
        assert O.g1_compress(a) == D.IDENT1_WIRE and O.g2_compress(b) == D.IDENT2_WIRE


# ---- the rules the GPU module expects a verifier's verdict from
@pytest.mark.parametrize("label", ["s=0", "s=r-1", "rv=0"])
def test_the_changed_input_rule_is_the_big_integer_verifier(label):
    """degenerate_cases.pinocchio_accepts_changed_input against Verify.f in Python integers (oracle_lib.pinocchio_verify, 13 pairings)"""
    name = "cubic6"
    cs, w = D.circuit(name)
    tox = D.row(D.pinocchio_rows, name, label)
    _, _, vk1, vk2 = D.pinocchio_key(name, tox)
    d, = D.draws(name, label, 1, 3)
    io = [w[k] for k in D.public(name)]
    io[1] = (io[1] + 1) % R
    want = D.pinocchio_accepts_changed_input(name, tox, d, 1)
    assert want == (label != "s=r-1")                                                  # both verdicts occur
    assert O.pinocchio_verify(vk1, vk2, io, D.pinocchio_proof(name, tox, d)) == want


def test_the_groth16_changed_input_rule_names_the_identity_points():
    for name in D.SMALL:
        for label, tox in D.groth16_rows(name):
            _, _, vk1, _ = D.groth16_key(name, tox)
            for j in range(len(D.public(name))):
                assert D.groth16_accepts_changed_input(name, tox, j) == (vk1[96 * (1 + j):96 * (2 + j)] == D.IDENT1), (name, label, j)
