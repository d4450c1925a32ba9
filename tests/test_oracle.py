"""Pins the CPU oracle (oracle/zk_oracle.c) before anything trusts it.

The reference holds no golden vectors ("parity unpinned"), so the oracle is
pinned by (1) oracle/pyref.py -- first-principles Python big ints, (2) the hand-derived
README-circuit fixture tests/golden/readme_circuit.json, (3) the reference's own algebraic
self-tests restated here (curve.ml:224-239, polynomial.ml:94-97,135-139,180-209,232-246;
FFT.ml:88-108), (4) `verify = true` through a pairing (src/lib/test/test.ml:178).
"""
import json
import os
import random

import pytest

import oracle_lib as O
from oracle import pyref as P
from zukelang_amd import r1cs as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readme_circuit.json")
rnd = random.Random(20261003)


def frb(x):
    return P.fr_to_bytes(x)


def frs(xs):
    return b"".join(P.fr_to_bytes(x) for x in xs)


def csrs(cs):
    return [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]


def test_constants_and_generators():
    d = json.load(open(GOLDEN))
    assert O.fr_omega() == frb(int(d["omega_2_32"], 16))
    assert O.g1_compress(O.g1_generator()).hex() == d["g1_generator_compressed"]
    assert O.g2_compress(O.g2_generator()).hex() == d["g2_generator_compressed"]
    assert d["g1_generator_compressed"].startswith("97f1d3a7")
    assert d["g2_generator_compressed"].startswith("93e02b60")
    assert P.on_curve(P.G1, P.B1) and P.on_curve(P.G2, P.B2)
    assert P.pt_mul(P.G1, P.R) is None and P.pt_mul(P.G2, P.R) is None
    assert pow(P.OMEGA, 1 << 32, P.R) == 1 and pow(P.OMEGA, 1 << 31, P.R) != 1


def test_public_known_answers():
    """Encodings of 2 G1, 3 G1 and 2 G2 in the zcash / IETF compressed format, as they circulate in public BLS12-381
    test suites (e.g. the BLS public keys of the secret keys 2 and 3).  There is no network here, so they were written
    down from memory and not fetched: 48- and 96-byte strings from outside this repository that the C oracle and the
    big-int restatement both reproduce."""
    kat1 = {2: "a572cbea904d67468808c8eb50a9450c9721db309128012543902d0ac358a62ae28f75bb8f1c7c42c39a8c5529bf0f4e",
            3: "89ece308f9d1f0131765212deca99697b112d61f9be9a5f1f3780a51335b3ff981747a0b2ca2179b96d2c0c9024e5224"}
    for k, hx in kat1.items():
        assert P.g1_compress(P.pt_mul(P.G1, k)).hex() == hx
        assert O.g1_compress(O.g1_mul(O.g1_generator(), frb(k))).hex() == hx
    kat2 = ("aa4edef9c1ed7f729f520e47730a124fd70662a904ba1074728114d1031e1572c6c886f6b57ec72a6178288c47c33577"
            "1638533957d540a9d2370f17cc7ed5863bc0b995b8825e0ee1ea1e1e4d00dbae81f14b0bf3611b78c952aacab827a053")
    assert P.g2_compress(P.pt_mul(P.G2, 2)).hex() == kat2
    assert O.g2_compress(O.g2_mul(O.g2_generator(), frb(2))).hex() == kat2


def test_public_known_answers_eip2537():
    """More pins from OUTSIDE this repository: the uncompressed coordinates that the published
    EIP-2537 precompile vectors carry for -G1, 2 G1 (`bls_g1add_(g1+g1=2*g1)`), -G2 (the pairing vector
    e(G1,G2) e(G1,-G2) = 1) and 2 G2 (`bls_g2add_(g2+g2=2*g2)`), written down from memory (no network) and reproduced
    by both restatements -- a wrong recollection could not match by accident.  The reference still holds no vector of
    its own: parity stays "unpinned" by /root/reference; these tie the oracle to the public BLS12-381 it claims to be."""
    neg_g1_y = "114d1d6855d545a8aa7d76c8cf2e21f267816aef1db507c96655b9d5caac42364e6f38ba0ecb751bad54dcd6b939c2ca"
    two_g1 = ("0572cbea904d67468808c8eb50a9450c9721db309128012543902d0ac358a62ae28f75bb8f1c7c42c39a8c5529bf0f4e",
              "166a9d8cabc673a322fda673779d8e3822ba3ecb8670e461f73bb9021d5fd76a4c56d9d4cd16bd1bba86881979749d28")
    neg_g2_y = ("13fa4d4a0ad8b1ce186ed5061789213d993923066dddaf1040bc3ff59f825c78df74f2d75467e25e0f55f8a00fa030ed",     # y.c1
                "0d1b3cc2c7027888be51d9ef691d77bcb679afda66c73f17f9ee3837a55024f78c71363275a75d75d86bab79f74782aa")     # y.c0
    two_g2 = ("0a4edef9c1ed7f729f520e47730a124fd70662a904ba1074728114d1031e1572c6c886f6b57ec72a6178288c47c33577",       # x.c1
              "1638533957d540a9d2370f17cc7ed5863bc0b995b8825e0ee1ea1e1e4d00dbae81f14b0bf3611b78c952aacab827a053",       # x.c0
              "0f6d4552fa65dd2638b361543f887136a43253d9c66c411697003f7a13c308f5422e1aa0a59c8967acdefd8b6e36ccf3",       # y.c1
              "0468fb440d82b0630aeb8dca2b5256789a66da69bf91009cbfe6bd221e47aa8ae88dece9764bf3bd999d95d71e4c9899")       # y.c0
    g1, g2 = O.g1_generator(), O.g2_generator()
    for pb, ob in ((P.g1_to_bytes(P.pt_neg(P.G1)), O.g1_mul(g1, frb(P.R - 1))),):
        assert pb == ob and pb[:48] == g1[:48] and pb[48:].hex() == neg_g1_y
    for pb, ob in ((P.g1_to_bytes(P.pt_mul(P.G1, 2)), O.g1_add(g1, g1)),):
        assert pb == ob and (pb[:48].hex(), pb[48:].hex()) == two_g1
    nb = P.g2_to_bytes(P.pt_neg(P.G2))
    assert nb == O.g2_mul(g2, frb(P.R - 1)) and nb[:96] == g2[:96] and (nb[96:144].hex(), nb[144:].hex()) == neg_g2_y
    db = P.g2_to_bytes(P.pt_mul(P.G2, 2))
    assert db == O.g2_add(g2, g2) and tuple(db[48 * i:48 * i + 48].hex() for i in range(4)) == two_g2
    # sign flag of the compressed form (curve.ml:199,208): -G carries 0x20, G does not
    assert O.g1_compress(P.g1_to_bytes(P.pt_neg(P.G1)))[0] == 0xb7 and O.g1_compress(g1)[0] == 0x97
    assert O.g2_compress(nb)[0] == 0xb3 and O.g2_compress(g2)[0] == 0x93


def test_field_vs_bigint():
    for _ in range(50):
        a, b = rnd.randrange(P.R), rnd.randrange(P.R)
        assert O.fr_mul(frb(a), frb(b)) == frb(a * b % P.R)
    for a in (1, 2, P.R - 1, rnd.randrange(P.R)):
        assert O.fr_inv(frb(a)) == frb(P.fr_inv(a))


def test_group_vs_bigint():
    g1, g2 = O.g1_generator(), O.g2_generator()
    for k in (0, 1, 2, P.R - 1, rnd.randrange(P.R), rnd.randrange(P.R)):
        p1, p2 = P.pt_mul(P.G1, k), P.pt_mul(P.G2, k)
        assert O.g1_mul(g1, frb(k)) == P.g1_to_bytes(p1)
        assert O.g2_mul(g2, frb(k)) == P.g2_to_bytes(p2)
        assert O.g1_compress(P.g1_to_bytes(p1)) == P.g1_compress(p1)
        assert O.g2_compress(P.g2_to_bytes(p2)) == P.g2_compress(p2)
    p = P.pt_mul(P.G1, 12345)
    q = P.pt_mul(P.G1, 999)
    pb, qb = P.g1_to_bytes(p), P.g1_to_bytes(q)
    assert O.g1_add(pb, qb) == P.g1_to_bytes(P.pt_add(p, q))
    assert O.g1_add(pb, pb) == P.g1_to_bytes(P.pt_add(p, p))                 # P + P
    assert O.g1_add(pb, P.g1_to_bytes(P.pt_neg(p))) == P.g1_to_bytes(None)   # P + (-P)
    assert O.g1_add(pb, P.g1_to_bytes(None)) == pb                            # P + O
    p2 = P.pt_mul(P.G2, 777)
    assert O.g2_add(P.g2_to_bytes(p2), P.g2_to_bytes(p2)) == P.g2_to_bytes(P.pt_add(p2, p2))


def test_curve_ml_homomorphism_selftest():
    """curve.ml:224-239: g*a = of_Fr a ; g*(ab+cd) = g*ab + g*cd for random ints < 10000."""
    a, b, c, d = (rnd.randrange(10000) for _ in range(4))
    g = O.g1_generator()
    lhs = O.g1_mul(g, frb(a * b + c * d))
    rhs = O.g1_add(O.g1_mul(g, frb(a * b)), O.g1_mul(g, frb(c * d)))
    assert lhs == rhs


def test_ntt_vs_definition():
    """FFT.ml:29-67: out[k] = sum_j a_j w_N^(jk), natural order; inverse divides by N."""
    for lg in range(0, 7):
        a = [rnd.randrange(P.R) for _ in range(1 << lg)]
        assert O.fr_ntt(frs(a), lg, False) == frs(P.ntt(a))
        assert O.fr_ntt(frs(a), lg, True) == frs(P.ntt(a, True))
    a = [rnd.randrange(P.R) for _ in range(1 << 10)]
    assert O.fr_ntt(O.fr_ntt(frs(a), 10, False), 10, True) == frs(a)   # FFT.ml:88-96 test_fft


def test_ntt_polynomial_mul_equals_naive():
    """FFT.ml:98-108 polynomial_mul == Polynomial.mul."""
    p1 = [rnd.randrange(P.R) for _ in range(13)]
    p2 = [rnd.randrange(P.R) for _ in range(20)]
    lg = 6
    f1 = RC.fr_ints(O.fr_ntt(frs(p1 + [0] * (64 - 13)), lg, False))
    f2 = RC.fr_ints(O.fr_ntt(frs(p2 + [0] * (64 - 20)), lg, False))
    prod = RC.fr_ints(O.fr_ntt(frs([x * y % P.R for x, y in zip(f1, f2)]), lg, True))
    assert P.poly_normalize(prod) == P.poly_mul(p1, p2)
    assert RC.fr_ints(O.poly_mul(frs(p1), frs(p2))) == P.poly_mul(p1, p2)


def test_polynomial_ml_kats():
    """polynomial.ml:94-97 apply KAT, :135-139 mul KAT, :180-209 div_rem identity, over Fr."""
    one = [1, 1, 1]
    assert RC.fr_ints(O.poly_mul(frs(one), frs([1, 1, 1, 1]))) == [1, 2, 3, 3, 2, 1]
    assert P.poly_eval([1, 2, 3, 4], 2) == 49
    for _ in range(50):
        a = [rnd.randrange(P.R) for _ in range(rnd.randrange(1, 20))]
        b = [rnd.randrange(P.R) for _ in range(rnd.randrange(1, 20))]
        q, r = O.poly_divrem(frs(a), frs(b))
        qi, ri = RC.fr_ints(q), RC.fr_ints(r)
        assert len(ri) < len(b)
        assert P.poly_add(P.poly_mul(qi, b), ri) == P.poly_normalize(a)
        pq, pr = P.poly_divrem(a, b)
        assert P.poly_normalize(qi) == pq and ri == pr


def test_polynomial_ml_interpolation_kats():
    """polynomial.ml:232-243 `test_interpolate`: the reference's three point sets -- two of them NOT contiguous integers -- over Fr instead of Q:
    the interpolant passes through every point (the reference's own assertion) and has the coefficients the rationals give."""
    third, half = P.fr_inv(3), P.fr_inv(2)
    for xys, coeffs in (([(0, 1), (1, 2)], [1, 1]),
                        ([(0, 10), (3, 9)], [10, (-third) % P.R]),
                        ([(1, 3), (2, 2), (3, 4)], [7, (-11 * half) % P.R, 3 * half % P.R])):
        f = P.interpolate(xys)
        assert all(P.poly_eval(f, x) == y % P.R for x, y in xys)
        assert P.poly_normalize(f) == coeffs
        basis = P.lagrange_basis([x for x, _ in xys])
        for j, (xj, _) in enumerate(xys):
            assert [P.poly_eval(basis[j], x) for x, _ in xys] == [1 if i == j else 0 for i in range(len(xys))]
    # on the QAP's domain 0..n-1 (QAP.ml:81-86) the general form is the integer-domain form the C oracle's QAP.build uses
    ys = [rnd.randrange(P.R) for _ in range(7)]
    assert P.poly_normalize(P.interpolate(list(enumerate(ys)))) == P.poly_normalize(P.interpolate_int_domain(ys))
    cs, _w = RC.iterated_cubic(6, 5)
    q = O.QAP(cs.n, cs.m, *csrs(cs))
    col = [0] * cs.n
    k = int(cs.O.col[1])
    for g in range(cs.n):
        for e in range(cs.O.ptr[g], cs.O.ptr[g + 1]):
            if cs.O.col[e] == k:
                col[g] = int.from_bytes(bytes(cs.O.val[32 * e:32 * e + 32]), "little")
    assert P.poly_normalize(RC.fr_ints(q.poly(2, k))) == P.poly_normalize(P.interpolate(list(enumerate(col))))
    assert P.poly_normalize(RC.fr_ints(q.poly(3))) == P.z_poly(cs.n)                       # polynomial.ml:248-251 `z`


def test_readme_circuit_fixture():
    d = json.load(open(GOLDEN))
    for case in d["cases"]:
        cs, w = RC.readme_circuit(case["x"])
        assert [hex(x) for x in w] == case["witness"]
        assert cs.check(w)
        q = O.QAP(cs.n, cs.m, *csrs(cs))
        assert [hex(x) for x in RC.fr_ints(q.poly(3))] == d["z"]
        rc, p, h = q.eval(frs(w))
        assert rc == 0
        assert [hex(x) for x in RC.fr_ints(h)] == case["h"]
        assert [hex(x) for x in RC.fr_ints(p)] == case["p"]
        v, ww, y = q.eval_vwy(frs(w))
        assert [hex(x) for x in P.poly_normalize(RC.fr_ints(v))] == case["v"]
        assert [hex(x) for x in P.poly_normalize(RC.fr_ints(ww))] == case["w"]
        assert [hex(x) for x in P.poly_normalize(RC.fr_ints(y))] == case["y"]
    # x = 3: h = -15 - 9 X
    assert [int(c, 16) for c in d["cases"][0]["h"]] == [P.R - 15, P.R - 9]
    # unsatisfied witness -> non-zero remainder (QAP.ml:134 assert)
    cs, w = RC.readme_circuit(3)
    w[4] += 1
    q = O.QAP(cs.n, cs.m, *csrs(cs))
    assert q.eval(frs(w))[0] == -3


def test_qap_build_interpolates():
    """QAP.ml:81-86: every variable polynomial takes the gate coefficient at X = gate id."""
    cs, w = RC.iterated_cubic(8, 5)
    q = O.QAP(cs.n, cs.m, *csrs(cs))
    for which, M in ((0, cs.L), (1, cs.R), (2, cs.O)):
        dense = [[0] * cs.n for _ in range(cs.m)]
        for g in range(cs.n):
            for e in range(M.ptr[g], M.ptr[g + 1]):
                dense[M.col[e]][g] = int.from_bytes(bytes(M.val[32 * e:32 * e + 32]), "little")
        for k in range(cs.m):
            poly = RC.fr_ints(q.poly(which, k))
            assert [P.poly_eval(poly, g) for g in range(cs.n)] == dense[k]
            assert poly == P.interpolate_int_domain(dense[k])


def _groth16_verify(cs, w, pk1, pk2, vk1, vk2, a, b, c):
    """groth16.ml:163-173: e(A,B) = e(alpha,beta) + e(sum_io w_k L_k/gamma, gamma) + e(C, delta)."""
    A, B, Cc = P.g1_from_bytes(a), P.g2_from_bytes(b), P.g1_from_bytes(c)
    alpha1, beta2 = P.g1_from_bytes(pk1[:96]), P.g2_from_bytes(pk2[:192])
    gm, dl = P.g2_from_bytes(vk2[192:384]), P.g2_from_bytes(vk2[384:576])
    io = [k for k in range(cs.m) if not cs.mid[k]]
    acc = None
    for j, k in enumerate(io):
        acc = P.pt_add(acc, P.pt_mul(P.g1_from_bytes(vk1[96 * (1 + j):96 * (2 + j)]), w[k]))
    return P.pairing_product_is_one([(A, B), (P.pt_neg(alpha1), beta2), (P.pt_neg(acc), gm), (P.pt_neg(Cc), dl)])


@pytest.mark.parametrize("maker", [lambda: RC.readme_circuit(3), lambda: RC.iterated_cubic(8, 0x1234567)])
def test_groth16_literal_equals_msm_form_equals_trapdoor_and_verifies(maker):
    cs, w = maker()
    assert cs.check(w)
    L, R_, Oo = csrs(cs)
    q = O.QAP(cs.n, cs.m, L, R_, Oo)
    st = P.fr_stream(0x5EED0002)
    tox = [next(st) for _ in range(7)]
    toxic, r, s = frs(tox[:5]), frb(tox[5]), frb(tox[6])
    pk1, pk2, vk1, vk2 = q.groth16_setup(toxic, cs.mid)
    sol = frs(w)
    rc1, a1, b1, c1 = q.groth16_prove(pk1, pk2, cs.mid, sol, r, s, 1)   # literal groth16.ml:116-161
    rc0, a0, b0, c0 = q.groth16_prove(pk1, pk2, cs.mid, sol, r, s, 0)
    a2, b2, c2 = O.groth16_prove_trapdoor(cs.n, cs.m, L, R_, Oo, cs.mid, sol, toxic, r, s)
    assert rc1 == 0 and rc0 == 0
    assert a1 == a0 == a2 and b1 == b0 == b2 and c1 == c0 == c2
    assert _groth16_verify(cs, w, pk1, pk2, vk1, vk2, a1, b1, c1)
    # a tampered proof must not verify
    assert not _groth16_verify(cs, w, pk1, pk2, vk1, vk2, O.g1_add(a1, O.g1_generator()), b1, c1)
    # setup exponents reproduce the key
    e1, e2, eio = O.groth16_setup_exponents(cs.n, cs.m, L, R_, Oo, cs.mid, toxic)
    g1, g2 = O.g1_generator(), O.g2_generator()
    for i in range(len(e1) // 32):
        assert O.g1_mul(g1, e1[32 * i:32 * i + 32]) == pk1[96 * i:96 * i + 96]
    for i in range(len(e2) // 32):
        assert O.g2_mul(g2, e2[32 * i:32 * i + 32]) == pk2[192 * i:192 * i + 192]
    for i in range(len(eio) // 32):
        assert O.g1_mul(g1, eio[32 * i:32 * i + 32]) == vk1[96 * (1 + i):96 * (2 + i)]


def test_msm_naive_matches_bigint_and_apply_powers_errors():
    n = 6
    ks = [rnd.randrange(P.R) for _ in range(n)]
    ss = [rnd.randrange(P.R) for _ in range(n)]
    bases1 = b"".join(O.g1_mul(O.g1_generator(), frb(k)) for k in ks)
    bases2 = b"".join(O.g2_mul(O.g2_generator(), frb(k)) for k in ks)
    rc, out = O.g1_msm_naive(bases1, frs(ss))
    exp = sum(k * s for k, s in zip(ks, ss)) % P.R
    assert rc == 0 and out == O.g1_mul(O.g1_generator(), frb(exp))
    assert out == P.g1_to_bytes(P.msm([P.g1_from_bytes(bases1[96 * i:96 * i + 96]) for i in range(n)], ss))
    rc, out = O.g2_msm_naive(bases2, frs(ss))
    assert rc == 0 and out == O.g2_mul(O.g2_generator(), frb(exp))
    assert O.fr_dot(frs(ks), frs(ss)) == frb(exp)
    # curve.ml:116 invalid_arg "apply_powers": fewer points than coefficients
    assert O.g1_msm_naive(bases1[:96 * 3], frs(ss))[0] == -2
    # curve.ml:115: coefficients may run out first
    rc, out = O.g1_msm_naive(bases1, frs(ss[:3]))
    assert rc == 0 and out == O.g1_mul(O.g1_generator(), frb(sum(k * s for k, s in zip(ks[:3], ss[:3])) % P.R))
    assert O.g1_msm_naive(b"", b"")[1] == P.g1_to_bytes(None)


@pytest.mark.parametrize("maker", [lambda: RC.readme_circuit(3), lambda: RC.iterated_cubic(6, 0x77)])
def test_pinocchio_literal_equals_trapdoor_and_verifies(maker):
    """pinocchio.ml: KeyGen.generate (:77-189), ZKCompute.f (:427-514), Verify.f (:254-420)."""
    cs, w = maker()
    L, R_, Oo = csrs(cs)
    q = O.QAP(cs.n, cs.m, L, R_, Oo)
    st = P.fr_stream(0x5EED0003)
    tox = [next(st) for _ in range(11)]
    toxic, (dv, dw, dy) = frs(tox[:8]), (frb(x) for x in tox[8:])
    lit = O.pinocchio_keygen_exponents(q, cs.n, cs.m, L, R_, Oo, cs.mid, toxic, True)      # Poly.apply on dense polys
    fast = O.pinocchio_keygen_exponents(None, cs.n, cs.m, L, R_, Oo, cs.mid, toxic, False)  # Lagrange basis
    assert lit == fast
    pk1, pk2 = O.points_of_exponents_g1(lit[0]), O.points_of_exponents_g2(lit[1])
    vk1, vk2 = O.points_of_exponents_g1(lit[2]), O.points_of_exponents_g2(lit[3])
    sol = frs(w)
    rc, proof = O.pinocchio_prove(q, pk1, pk2, cs.mid, sol, dv, dw, dy)
    assert rc == 0
    assert proof == O.pinocchio_prove_trapdoor(cs.n, cs.m, L, R_, Oo, cs.mid, sol, toxic, dv, dw, dy)
    io = [w[k] for k in range(cs.m) if not cs.mid[k]]
    assert O.pinocchio_verify(vk1, vk2, io, proof)
    # NonZK (Compute.f :210-248) = zero blinding; also verifies
    z = frb(0)
    rc, proof0 = O.pinocchio_prove(q, pk1, pk2, cs.mid, sol, z, z, z)
    assert rc == 0 and proof0 != proof and O.pinocchio_verify(vk1, vk2, io, proof0)
    # tampering breaks it
    bad = bytearray(proof)
    bad[384:480] = O.g1_add(bytes(proof[384:480]), O.g1_generator())
    assert not O.pinocchio_verify(vk1, vk2, io, bytes(bad))


def test_decoder_oracle_round_trips_and_public_vectors():
    """pyref.fp_sqrt / fp2_sqrt / g1,g2_decompress / g1,g2_decode / pt_mul_jac (the decoder oracle of tests/test_decoders.py): inverse of g1/g2_compress
    over both signs of y, the generators' public compressed strings, the EIP-2537 coordinates of -G1, 2 G1, -G2, 2 G2 used above, and the rules
    that make a string non-canonical."""
    for k in (1, 2, 3, 0xDEADBEEF, P.R - 1, P.R - 2):
        assert P.pt_mul_jac(P.G1, k) == P.pt_mul(P.G1, k) and P.pt_mul_jac(P.G2, k) == P.pt_mul(P.G2, k)
        for pt, comp, dec, enc, raw in ((P.pt_mul(P.G1, k), P.g1_compress, P.g1_decompress, P.g1_to_bytes, P.g1_decode),
                                        (P.pt_mul(P.G2, k), P.g2_compress, P.g2_decompress, P.g2_to_bytes, P.g2_decode)):
            signs = set()
            for q in (pt, P.pt_neg(pt)):
                c = comp(q)
                signs.add(c[0] & 0x20)
                assert dec(c) == (P.OK, q) and raw(enc(q)) == (P.OK, q)
            assert signs == {0, 0x20}
    assert P.pt_mul_jac(P.G1, P.R) is None and P.pt_mul_jac(P.G2, P.R) is None and P.pt_mul_jac(None, 5) is None
    for dec, comp, raw, enc in ((P.g1_decompress, P.g1_compress, P.g1_decode, P.g1_to_bytes), (P.g2_decompress, P.g2_compress, P.g2_decode, P.g2_to_bytes)):
        assert dec(comp(None)) == (P.OK, None) and raw(enc(None)) == (P.OK, None)
    d = json.load(open(GOLDEN))
    assert P.g1_decompress(bytes.fromhex(d["g1_generator_compressed"])) == (P.OK, P.G1)
    assert P.g2_decompress(bytes.fromhex(d["g2_generator_compressed"])) == (P.OK, P.G2)
    # the EIP-2537 coordinates: -G1 and 2 G1 uncompressed, 2 G2 from its compressed string
    neg_g1_y = "114d1d6855d545a8aa7d76c8cf2e21f267816aef1db507c96655b9d5caac42364e6f38ba0ecb751bad54dcd6b939c2ca"
    assert P.g1_decode(P.G1_X.to_bytes(48, "big") + bytes.fromhex(neg_g1_y)) == (P.OK, P.pt_neg(P.G1))
    two_g1_x = "0572cbea904d67468808c8eb50a9450c9721db309128012543902d0ac358a62ae28f75bb8f1c7c42c39a8c5529bf0f4e"
    two_g1_y = "166a9d8cabc673a322fda673779d8e3822ba3ecb8670e461f73bb9021d5fd76a4c56d9d4cd16bd1bba86881979749d28"
    assert P.g1_decompress(bytes.fromhex("a5" + two_g1_x[2:])) == (P.OK, (P.Fp1(int(two_g1_x, 16)), P.Fp1(int(two_g1_y, 16))))
    assert P.g2_decompress(P.g2_compress(P.pt_mul(P.G2, 2)))[1] == P.pt_mul(P.G2, 2)
    # square roots: the larger root, None for a non-square; Fp2 with a zero imaginary part on either side
    for a in (0, 1, 4, 9, P.P - 1, 2):
        r = P.fp_sqrt(a)
        assert (r is None) == (pow(a, (P.P - 1) // 2, P.P) == P.P - 1) and (r is None or (r * r % P.P == a and r >= (P.P - r) % P.P))
    assert P.fp_sqrt(P.P - 1) is None and P.fp_sqrt(4) == P.P - 2
    for a in (P.Fp2(4, 0), P.Fp2(-4, 0), P.Fp2(0, 2), P.Fp2(3, 4), P.Fp2(5, 7) * P.Fp2(5, 7), P.Fp2(0, 0)):
        r = P.fp2_sqrt(a)
        assert r * r == a and (r.b, r.a) >= ((-r).b, (-r).a), a
    assert P.fp2_sqrt(P.Fp2(4, 0)) == P.Fp2(-2, 0) and P.fp2_sqrt(P.Fp2(-4, 0)) == P.Fp2(0, -2)
    # what makes a string non-canonical
    g = P.g1_compress(P.G1)
    assert P.g1_decompress(bytes([g[0] & 0x7F]) + g[1:])[0] == P.BAD_ENCODING and P.g1_decompress(g[:47])[0] == P.BAD_ENCODING
    assert P.g1_decompress(bytes([0xE0]) + bytes(47))[0] == P.BAD_ENCODING and P.g1_decompress(bytes([0xC0]) + bytes(46) + b"\x01")[0] == P.BAD_ENCODING
    assert P.g1_decompress(bytes([0x80 | 0x1A]) + (P.P % (1 << 376)).to_bytes(47, "big"))[0] == P.BAD_ENCODING          # x = p
    assert P.g1_decode(bytes([0x60]) + bytes(95))[0] == P.BAD_ENCODING and P.g2_decode(bytes([0x40]) + bytes(190) + b"\x01")[0] == P.BAD_ENCODING
    e = bytearray(P.g1_to_bytes(P.G1)); e[0] |= 0x20
    assert P.g1_decode(bytes(e))[0] == P.BAD_ENCODING
