"""Pairings on the device (csrc/pairing_dev.hip, csrc/pairing_tower.cuh) against the oracle's Python Fp12 and the library's own host pairing.

Layer by layer, so that a failure names its layer: the Fp12 tower through zk_selftest_fp12 (every operation against oracle/pyref.py), then
zk_pairing_product_many against zk_pairing_product byte for byte -- every batch size that fills one group of lanes, part of a wave, a whole wave,
a wave and a bit, several workgroups -- then one call of products of different lengths with identities and cancelling pairs in it, then the
verdicts on bad points."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyref as P
from zukelang_amd import _lib
from zukelang_amd.curve import G1, G2, Pairing

pytestmark = pytest.mark.gpu

ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE = -1, -2
OPS = {"mul": 0, "sqr": 1, "inv": 2, "conj": 3, "frob": 4, "frob2": 5, "mul_line": 6, "final_exp": 7}
IDENT1, IDENT2 = b"\x40" + bytes(95), b"\x40" + bytes(191)


def gt_bytes(f):
    """oracle Fp12 -> the library's GT encoding: c0.c0.a, c0.c0.b, c0.c1.a, ... c1.c2.b, 48 B big-endian."""
    out = b""
    for six in (f.c0, f.c1):
        for c in (six.c0, six.c1, six.c2):
            out += c.a.to_bytes(48, "big") + c.b.to_bytes(48, "big")
    return out


def fp12_of(coeffs):
    c = [P.Fp2(coeffs[2 * i], coeffs[2 * i + 1]) for i in range(6)]
    return P.Fp12(P.Fp6(c[0], c[1], c[2]), P.Fp6(c[3], c[4], c[5]))


def selftest(op, a, b=None):
    n = len(a)
    out = np.zeros(576 * n, dtype=np.uint8)
    pa, ka = _lib.u8(b"".join(gt_bytes(x) for x in a))
    pb, kb = _lib.u8(b"".join(gt_bytes(x) for x in b)) if b is not None else (None, None)
    _lib.check(_lib.lib().zk_selftest_fp12(OPS[op], pa, pb, n, out.ctypes.data_as(_lib._P8)))
    raw = out.tobytes()
    return [raw[576 * i:576 * (i + 1)] for i in range(n)]


@pytest.fixture(scope="module")
def elements():
    """0, 1, p - 1 in every coefficient, a unitary element (a pairing value), 16 random elements -- and a second operand for each."""
    st = P.fr_stream(0xF12)
    rnd = lambda: ((next(st) << 256) | next(st)) % P.P
    unitary = P.pairing(P.pt_mul(P.G1, 0xABCDEF), P.pt_mul(P.G2, 0x123457))
    a = [fp12_of([0] * 12), P.FP12_ONE, fp12_of([P.P - 1] * 12), unitary] + [fp12_of([rnd() for _ in range(12)]) for _ in range(16)]
    b = [fp12_of([rnd() for _ in range(12)]) for _ in range(len(a) - 3)] + [unitary, fp12_of([P.P - 1] * 12), fp12_of([0] * 12)]
    return a, b


def test_fp12_product_square_inverse_conjugate(elements):
    a, b = elements
    assert selftest("mul", a, b) == [gt_bytes(x * y) for x, y in zip(a, b)]
    assert selftest("sqr", a) == [gt_bytes(x * x) for x in a]
    assert selftest("inv", a) == [gt_bytes(x.inv()) for x in a]          # 1 / 0 = 0 on both sides (the inversion's convention)
    assert selftest("conj", a) == [gt_bytes(x.conj()) for x in a]
    assert selftest("conj", a[3:4]) == selftest("inv", a[3:4])            # unitary: the conjugate is the inverse


def test_fp12_frobenius_maps(elements):
    a, _ = elements
    fr1 = [x.pow(P.P) for x in a]                                        # the definition, 381 squarings each
    assert selftest("frob", a) == [gt_bytes(x) for x in fr1]
    assert selftest("frob2", a) == [gt_bytes(x.pow(P.P)) for x in fr1]


def test_fp12_product_with_a_sparse_line(elements):
    a, b = elements
    z = P.Fp2(0)
    sparse = [P.Fp12(P.Fp6(y.c0.c0, z, z), P.Fp6(z, y.c1.c1, y.c1.c2)) for y in b]          # w^0, w^3 = v w, w^5 = v^2 w
    assert selftest("mul_line", a, sparse) == [gt_bytes(x * y) for x, y in zip(a, sparse)]
    assert selftest("mul_line", a, b) == [gt_bytes(x * y) for x, y in zip(a, sparse)]       # the other coefficients of b are not read


def test_fp12_final_exponentiation_special_elements(elements):
    a, _ = elements
    got = selftest("final_exp", a)
    assert got[0] == gt_bytes(fp12_of([0] * 12)) and got[1] == gt_bytes(P.FP12_ONE)
    assert got[2] == gt_bytes(P.final_exp(a[2])) and got[3] == gt_bytes(P.final_exp(a[3]))


def test_fp12_final_exponentiation_random_elements(elements):
    """x -> x^((p^12 - 1) / r) is a homomorphism, and the oracle's plain power costs a second per element in Python.  So the 16 random elements
    are held to it TOGETHER: with 64-bit weights c_i drawn here (the device never sees them) prod_i y_i^(c_i) must be the oracle's final
    exponentiation of prod_i x_i^(c_i) for the device's y_i.  A wrong y_i = (right value) * d_i survives only if prod_i d_i^(c_i) = 1 for
    these weights.  Two further elements are compared one by one, as the special ones are."""
    a, _ = elements
    x = a[4:]
    got = selftest("final_exp", x)
    y = [fp12_of([int.from_bytes(g[48 * k:48 * (k + 1)], "big") for k in range(12)]) for g in got]
    st = P.fr_stream(0xC0FFEE12)
    c = [next(st) >> 191 for _ in x]
    lhs, rhs = P.FP12_ONE, P.FP12_ONE
    for xi, yi, ci in zip(x, y, c):
        lhs, rhs = lhs * yi.pow(ci), rhs * xi.pow(ci)
    assert lhs == P.final_exp(rhs)
    for i in (0, 15):
        assert got[i] == gt_bytes(P.final_exp(x[i]))
    for yi in y[:4]:
        assert yi.pow(P.R) == P.FP12_ONE                                  # ... and they lie in GT


# ------------------------------------------------------------------------------------------------------------------ products against the host
def host_product(g1, g2):
    out = C.create_string_buffer(576)
    rc = _lib.lib().zk_pairing_product(g1, g2, C.c_size_t(len(g1) // 96), out)
    return rc, out.raw


@pytest.fixture(scope="module")
def pool():
    """129 pairs ([a] G1, [b] G2), scalars 1, r - 1, 2^200 among random ones, and the host's pairing of each (about 1.3 s, once)."""
    st = P.fr_stream(0x9A121)
    a = [1, P.R - 1, 1 << 200, 5] + [next(st) for _ in range(125)]
    b = [1, 1 << 200, P.R - 1, 11] + [next(st) for _ in range(125)]
    frs = lambda xs: b"".join(P.fr_to_bytes(x) for x in xs)
    g1, g2 = bytes(G1.of_Fr(frs(a))), bytes(G2.of_Fr(frs(b)))
    assert g1[:96] == P.g1_to_bytes(P.G1) and g2[192 * 3:192 * 4] == P.g2_to_bytes(P.pt_mul(P.G2, 11))
    host = []
    for i in range(129):
        rc, gt = host_product(g1[96 * i:96 * (i + 1)], g2[192 * i:192 * (i + 1)])
        assert rc == 0
        host.append(gt)
    return g1, g2, host


@pytest.mark.parametrize("n", list(range(1, 13)) + [63, 64, 65, 129])
def test_single_pair_products_match_the_host(pool, n):
    g1, g2, host = pool
    assert Pairing.product_many(g1[:96 * n], g2[:192 * n], [1] * n) == host[:n]


def test_one_call_of_products_of_different_lengths(pool):
    g1, g2, host = pool
    p1 = lambda i: g1[96 * i:96 * (i + 1)]
    p2 = lambda i: g2[192 * i:192 * (i + 1)]
    neg5 = P.g1_to_bytes(P.pt_neg(P.pt_mul(P.G1, 5)))
    lens = [0, 1, 2, 3, 4, 40, 1]
    prods = [[],
             [(p1(0), p2(0))],                                            # the generator pair
             [(IDENT1, p2(7)), (p1(8), p2(8))],                           # an identity in G1
             [(p1(9), IDENT2), (p1(10), p2(10)), (p1(11), p2(11))],       # an identity in G2
             [(p1(3), p2(3)), (neg5, p2(3)), (p1(12), p2(12)), (p1(13), p2(13))],          # (P, Q) next to (-P, Q)
             [(p1(20 + i), p2(20 + i)) for i in range(40)],
             [(p1(3), p2(3))]]
    assert [len(x) for x in prods] == lens
    got = Pairing.product_many(b"".join(a for pr in prods for a, _ in pr), b"".join(b for pr in prods for _, b in pr), lens)
    for k, pr in enumerate(prods):
        rc, want = host_product(b"".join(a for a, _ in pr), b"".join(b for _, b in pr))
        assert rc == 0 and got[k] == want, k
    assert got[0] == gt_bytes(P.FP12_ONE)
    assert got[6] == gt_bytes(P.pairing(P.pt_mul(P.G1, 5), P.pt_mul(P.G2, 11)))          # coefficient by coefficient against the oracle
    assert got[2] == host[8]


# ------------------------------------------------------------------------------------------------------------------ bad points
def _g1_outside_subgroup():
    x = 0
    while True:
        x += 1
        y2 = (x ** 3 + 4) % P.P
        y = pow(y2, (P.P + 1) // 4, P.P)
        if y * y % P.P == y2:
            pt = (P.Fp1(x), P.Fp1(y))
            if P.pt_mul(pt, P.R) is not None:
                return P.g1_to_bytes(pt)


def _g2_outside_subgroup():
    x = 0
    while True:
        x += 1
        y = P.fp2_sqrt(P.Fp2(x, 1) * P.Fp2(x, 1) * P.Fp2(x, 1) + P.B2)
        if y is not None:
            pt = (P.Fp2(x, 1), y)
            if P.pt_mul(pt, P.R) is not None:
                return P.g2_to_bytes(pt)


@pytest.fixture(scope="module")
def bad_points():
    good1, good2 = P.g1_to_bytes(P.pt_mul(P.G1, 7)), P.g2_to_bytes(P.pt_mul(P.G2, 9))
    y_changed = bytearray(good1); y_changed[95] ^= 1
    y2_changed = bytearray(good2); y2_changed[191] ^= 1
    comp = bytearray(good1); comp[0] |= 0x80
    comp2 = bytearray(good2); comp2[0] |= 0x80
    inf1 = bytearray(IDENT1); inf1[40] = 1
    inf2 = bytearray(IDENT2); inf2[0] |= 0x20
    return good1, good2, {
        "y changed (G1)": (bytes(y_changed), good2), "y changed (G2)": (good1, bytes(y2_changed)),
        "G1 outside the subgroup": (_g1_outside_subgroup(), good2), "G2 on the twist outside the subgroup": (good1, _g2_outside_subgroup()),
        "compression flag (G1)": (bytes(comp), good2), "compression flag (G2)": (good1, bytes(comp2)),
        "non-canonical infinity (G1)": (bytes(inf1), good2), "non-canonical infinity (G2)": (good1, bytes(inf2)),
        "(0, 0) without the infinity bit": (bytes(96), good2),
    }


def many_rc(g1, g2, lens):
    out = np.zeros(576 * len(lens), dtype=np.uint8)
    p1, k1 = _lib.u8(g1)
    p2, k2 = _lib.u8(g2)
    return _lib.lib().zk_pairing_product_many(p1, p2, (C.c_uint64 * len(lens))(*lens), len(lens), out.ctypes.data_as(_lib._P8))


def test_bad_points_fail_the_call_with_the_hosts_code(bad_points):
    good1, good2, bad = bad_points
    codes = {}
    for name, (b1, b2) in bad.items():
        host_rc, _ = host_product(b1, b2)
        assert host_rc in (ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE), name
        # alone, and as the last pair of the third product of a call whose other points are good
        assert many_rc(b1, b2, [1]) == host_rc, name
        assert many_rc(good1 * 4 + b1, good2 * 4 + b2, [2, 0, 3]) == host_rc, name
        codes[name] = host_rc
    assert codes["y changed (G1)"] == ZK_ERR_NOT_ON_CURVE and codes["compression flag (G2)"] == ZK_ERR_ARG          # the two codes differ: the next test needs both


def test_two_bad_points_report_the_first(bad_points):
    good1, good2, bad = bad_points
    off1, _ = bad["y changed (G1)"]                 # ZK_ERR_NOT_ON_CURVE
    _, flag2 = bad["compression flag (G2)"]         # ZK_ERR_ARG
    # the host's order: G1 of pair i, then G2 of pair i
    assert many_rc(good1 + off1 + good1, good2 + good2 + flag2, [3]) == ZK_ERR_NOT_ON_CURVE
    assert many_rc(good1 + good1 + off1, good2 + flag2 + good2, [1, 2]) == ZK_ERR_ARG
    assert many_rc(off1, flag2, [1]) == ZK_ERR_NOT_ON_CURVE           # the same pair: its G1 point comes first
    assert many_rc(good1 * 70 + off1, flag2 + good2 * 70, [71]) == ZK_ERR_ARG
