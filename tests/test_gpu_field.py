"""GPU parity of the base-field layer (14 x 29-bit limbs, lazy reduction, value bounds in the type):
zk_selftest_fp evaluates 23 expressions per operand pair through the same code paths the group law uses;
the expected values are Python big-integer arithmetic mod p.  Edge operands: 0, 1, p-1, values whose limbs are
all-ones at the 29-bit boundaries, a = b, a + b = p."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import pyref as P
from zukelang_amd import _lib

pytestmark = pytest.mark.gpu
p = P.P
NOUT = 23


def le48(x):
    return int(x).to_bytes(48, "little")


def operands():
    rnd = random.Random(0xF1E1D)
    edge = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 380, (1 << 381) - 1 - ((1 << 381) - 1 - (p - 1)),
            sum(0x1FFFFFFF << (29 * i) for i in range(13)) % p, sum(0x10000000 << (29 * i) for i in range(14)) % p,
            (1 << 29) - 1, 1 << 29, (1 << 58) - 1, p - (1 << 29), 3 * ((p - 1) // 7)]
    a, b = [], []
    for x in edge:
        for y in (edge[0], edge[1], edge[3], x, (p - x) % p, rnd.randrange(p)):
            a.append(x); b.append(y)
    for _ in range(4096 - len(a)):
        a.append(rnd.randrange(p)); b.append(rnd.randrange(p))
    if len(a) & 1:
        a.append(5); b.append(7)
    return a, b


def test_field_battery_matches_big_integers():
    a, b = operands()
    n = len(a)
    out = np.zeros(NOUT * 48 * n, dtype=np.uint8)
    _lib.check(_lib.lib().zk_selftest_fp(b"".join(le48(x) for x in a), b"".join(le48(x) for x in b), C.c_size_t(n),
                                         out.ctypes.data_as(C.POINTER(C.c_uint8))))
    raw = out.tobytes()
    get = lambda i, k: int.from_bytes(raw[48 * (NOUT * i + k):48 * (NOUT * i + k + 1)], "little")
    inv = lambda x: pow(x, p - 2, p)
    for i in range(n):
        x, y = a[i], b[i]
        d1 = (-x - 2 * y) % p
        exp = [(x + y) % p, (x - y) % p, x * y % p, x * x % p, (-x) % p, inv(x), 8 * x % p, d1, d1 * (y - x) % p,
               (x * y - (x + y) * (x - y)) % p]
        for k, e in enumerate(exp):
            assert get(i, k) == e, (i, k, hex(x), hex(y))
        flags = 1 | 2 | (4 if x == 0 else 0) | 8 | (16 if x == y else 0) | 32
        assert get(i, 10) == flags, (i, hex(x), hex(y), get(i, 10))
        assert get(i, 11) == 0
        assert get(i, 15) == x * y % p
        # lane pairs: (a_even + a_odd u) and (b_even + b_odd u) in Fp2 = Fp[u]/(u^2 + 1)
        e = i & ~1
        x0, x1, y0, y1 = a[e], a[e + 1], b[e], b[e + 1]
        mul = ((x0 * y0 - x1 * y1) % p, (x0 * y1 + x1 * y0) % p)
        sqr = ((x0 * x0 - x1 * x1) % p, 2 * x0 * x1 % p)
        s0, s1, t0, t1 = (x0 - y0) % p, (x1 - y1) % p, (x0 + y0) % p, (x1 + y1) % p
        dif = ((s0 * t0 - s1 * t1) % p, (s0 * t1 + s1 * t0) % p)
        c = i & 1
        assert (get(i, 12), get(i, 13), get(i, 14)) == (mul[c], sqr[c], dif[c]), (i, "fp2 lane pair")
        # lockstep inversion (csrc/fp_inv.cuh): base field, and Fp2 on the lane pair: 1 / (x0 + x1 u) = (x0 - x1 u) / (x0^2 + x1^2)
        assert get(i, 16) == inv(x), (i, "fe_inv_fast", hex(x))
        nrm = inv((x0 * x0 + x1 * x1) % p)
        assert get(i, 17) == ((x0 * nrm) % p, (-x1 * nrm) % p)[c], (i, "fp2 fe_inv_fast")
        # round 3: the fused a - b - 2 c (one carry pass), the lazily negated factor of the fused double product, the lazy negation inside the lane-pair product
        big = (16 * x - y) % p
        assert get(i, 18) == (x * x - x * y - 2 * y * (x + y)) % p, (i, "fe_sub_sub_dbl on products", hex(x), hex(y))
        assert get(i, 19) == (x - 3 * big) % p, (i, "fe_sub_sub_dbl at the at-rest bound", hex(x), hex(y))
        assert get(i, 20) == (x * y - big * y) % p, (i, "fe_mul_sub with a lazily negated factor", hex(x), hex(y))
        b0, b1 = (16 * x0 - y0) % p, (16 * x1 - y1) % p
        assert get(i, 21) == ((b0 * y0 - b1 * y1) % p, (b0 * y1 + b1 * y0) % p)[c], (i, "fp2 lane-pair product, lazily reduced left operand")
        assert get(i, 22) == ((b0 * b0 - b1 * b1) % p, 2 * b0 * b1 % p)[c], (i, "fp2 lane-pair square with the lazy difference")


def test_inversions_whose_montgomery_residue_is_the_edge():
    """Added rows for outputs 5, 16 and 17.  The hook takes canonical x and inverts the integer x * 2^406 mod p, so 0, 1, 2^380 above arrive as what are in
    effect random integers.  Here x = X * 2^-406 mod p for the X that matter to fp_inv29_call (tests/fp29_cases.py): those that keep it busy for all 27
    iterations, those of them a 26-iteration build gets wrong, the values on either side of its `exact` switch, the limb boundaries.  For output 17 the
    pair (x0, x1) is steered so that the norm x0^2 + x1^2 is such an x, where x - x1^2 has a square root."""
    import fp29_cases as Cs
    classes = Cs.full_length_montgomery_residues()
    assert all(classes.values()) and len(classes["needs_all_27"]) >= 32 and len(classes["wrong_after_26"]) >= 16
    rinv = pow(2, -406, p)
    rnd = random.Random(0xED6E)
    xs = [X * rinv % p for cl in classes.values() for X in cl]
    a, b, steered = [], [], 0
    for x in xs:                                    # lanes (2k, 2k+1): x itself beside a random partner
        a += [x, rnd.randrange(p)]
        b += [rnd.randrange(p), x]
    for x in xs:                                    # lanes (2k, 2k+1) = (x0, x1) with x0^2 + x1^2 = x
        for _ in range(64):
            x1 = rnd.randrange(p)
            x0 = pow((x - x1 * x1) % p, (p + 1) // 4, p)
            if (x0 * x0 + x1 * x1) % p == x:
                a += [x0, x1]
                b += [rnd.randrange(p), rnd.randrange(p)]
                steered += 1
                break
    assert steered >= len(xs) * 3 // 4
    n = len(a)
    out = np.zeros(NOUT * 48 * n, dtype=np.uint8)
    _lib.check(_lib.lib().zk_selftest_fp(b"".join(le48(x) for x in a), b"".join(le48(x) for x in b), C.c_size_t(n), out.ctypes.data_as(C.POINTER(C.c_uint8))))
    raw = out.tobytes()
    get = lambda i, k: int.from_bytes(raw[48 * (NOUT * i + k):48 * (NOUT * i + k + 1)], "little")
    inv = lambda x: pow(x, p - 2, p)
    for i in range(n):
        assert get(i, 5) == inv(a[i]), (i, "fe_inv", hex(a[i]))
        assert get(i, 16) == inv(a[i]), (i, "fe_inv_fast", hex(a[i]))
        e = i & ~1
        nrm = inv((a[e] * a[e] + a[e + 1] * a[e + 1]) % p)
        assert get(i, 17) == ((a[e] * nrm) % p, (-a[e + 1] * nrm) % p)[i & 1], (i, "fp2 fe_inv_fast", hex(a[e]), hex(a[e + 1]))


def be48(x):
    return int(x).to_bytes(48, "big")


def _selftest_sqrt(field, blobs):
    n, B = len(blobs), 96 if field else 48
    root = np.zeros(B * n, dtype=np.uint8)
    sq = np.zeros(n, dtype=np.uint8)
    _lib.check(_lib.lib().zk_selftest_sqrt(C.c_int(field), b"".join(blobs), C.c_size_t(n), root.ctypes.data_as(C.POINTER(C.c_uint8)),
                                           sq.ctypes.data_as(C.POINTER(C.c_uint8))))
    raw = root.tobytes()
    return [raw[B * i:B * (i + 1)] for i in range(n)], [int(x) for x in sq]


def test_square_roots_and_the_sign_rule_match_big_integers():
    """zk_selftest_sqrt: fp_sqrt_dev / fp2_sqrt_dev and the sign rule of k_decompress_g1/g2 (one device function for both) on bare field elements against
    pyref.fp_sqrt / fp2_sqrt, which return the lexicographically larger root.  Fp2 covers what no subgroup point the suite can construct reaches: a zero
    imaginary part of the ARGUMENT (root real or purely imaginary), a zero imaginary part of the ROOT (the sign then comes from the real part), and both
    candidates (a0 + s)/2, (a0 - s)/2 for the real part's square.  Exact bytes; every class of input is counted and must occur."""
    rnd = random.Random(0x5C207)
    # ---- Fp
    ts = [rnd.randrange(1, p) for _ in range(40)]
    fp = [0, 1, p - 1, 4, 2, 3, (p - 1) // 2, (p + 1) // 2] + [t * t % p for t in ts] + [(-t * t) % p for t in ts]
    fp += [rnd.randrange(p) for _ in range(4096 - len(fp))]
    roots, sq = _selftest_sqrt(0, [be48(a) for a in fp])
    seen = {"square": 0, "non-square": 0}
    for a, r, s in zip(fp, roots, sq):
        want = P.fp_sqrt(a)
        seen["square" if want is not None else "non-square"] += 1
        assert s == (want is not None) and r == be48(want or 0), ("Fp", hex(a), r.hex(), s)
    assert all(seen.values()), seen
    # ---- Fp2
    F = P.Fp2
    euler = lambda v: pow(v % p, (p - 1) // 2, p)
    el = []
    for t in ts[:24]:
        c = t * t % p
        el += [F(c, 0), F(-c, 0), F(0, c), F(0, -c), F(t, 0), F(0, t)]                        # (c, 0) with c a square / a non-square of Fp; (0, c); arbitrary ones
        el += [F(t, 0) * F(t, 0), F(0, t) * F(0, t), F(t, t) * F(t, t), F(t, -t) * F(t, -t)]      # squares of (t, 0), (0, t), (t, t), (t, -t)
    el += [F(0, 0), F(1, 0), F(0, 1), F(p - 1, 0), F(0, p - 1), F(4, 0), F(4, 4), F(p - 1, p - 1)]
    while len(el) < 4096:
        a = F(rnd.randrange(p), rnd.randrange(p))
        el.append(a * a if rnd.random() < 0.5 else a)
    roots, sq = _selftest_sqrt(1, [be48(a.b) + be48(a.a) for a in el])
    seen = {"real argument, real root": 0, "real argument, imaginary root": 0, "norm not a square": 0, "first candidate": 0, "second candidate": 0,
            "root with a zero imaginary part": 0, "root with a zero real part": 0}
    for a, r, s in zip(el, roots, sq):
        want = P.fp2_sqrt(a)
        assert s == (want is not None), ("Fp2", a, s)
        assert r == (be48(want.b) + be48(want.a) if want is not None else bytes(96)), ("Fp2", a, r.hex())
        if a.b == 0 and not a.is_zero():
            seen["real argument, real root" if want.b == 0 else "real argument, imaginary root"] += 1
        elif want is None:
            seen["norm not a square"] += 1
        elif not a.is_zero():
            s0 = pow((a.a * a.a + a.b * a.b) % p, (p + 1) // 4, p)                              # the root of the norm that a^((p+1)/4) gives
            seen["first candidate" if euler((a.a + s0) * P.fp_inv(2)) == 1 else "second candidate"] += 1
        if want is not None and not want.is_zero():
            if want.b == 0:
                seen["root with a zero imaginary part"] += 1
            if want.a == 0:
                seen["root with a zero real part"] += 1
    assert all(seen.values()), seen
    # an element >= p is refused
    assert _lib.lib().zk_selftest_sqrt(C.c_int(0), be48(p), C.c_size_t(1), C.create_string_buffer(48), C.create_string_buffer(1)) == -1
