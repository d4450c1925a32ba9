"""Two Fp2 products on a lane pair, one whole lazy-Karatsuba product per lane (csrc/ff.cuh: fe_mul2_lanewise, csrc/fp2_lane_gen.cuh), and the G2 bucket
accumulation rebuilt on them, against Python integers and the oracle.

The even lane of a pair gathers both components of a and b and runs a b, the odd lane those of c and d and runs c d; both results go back to the
component layout.  What can go wrong: a gather taking the wrong lane's half, a scatter swapping the two results or their components, the signed c0
chain at the largest limbs, the missing top limb of c0 + p:
  * zk_selftest_fp2_lanewise on 4096 quadruples (a, b, c, d) of Fp2 -- a b, c d and the fused a b - c d, exact against integers: random values lifted to
    the at-rest bound 64 p in weakly normalised limbs (all eight components different, so every wrong half shows), every limb at its maximum, 0 and
    p - 1 in each component alone, a = c with b = d (the two lanes must then agree), one product extreme beside one zero both ways round;
  * zk_msm_g2 at 65 and 1025 points with ZK_ACC_G2_INLINE = 0 and 1, against the oracle's naive fold: one base repeated 20 times under scalar 1 (equal
    x: the out-of-line doubling, then a run that crosses a chunk border), P, -P and Q in one bucket (the accumulator returns to the identity in mid-run),
    an identity base, and a last chunk of 7 entries; 43 and 1003 chunks leave the last wave partly filled.
No tolerances anywhere."""
import ctypes as C
import random
from functools import lru_cache

import numpy as np
import pytest

from oracle import pyref as P
from test_gpu_field import operands as field_operands
from test_gpu_fp_paired import L, W, exact_limbs, max_limbs, value, weak_limbs
from test_gpu_msm_collisions import CHUNK, borders, curve, runs
from test_gpu_options import options
from zukelang_amd import _lib
from zukelang_amd import r1cs as RC
from zukelang_amd.curve import G2

pytestmark = pytest.mark.gpu
p = P.P
WEAK = (1 << W) + 7
RINV = pow(1 << (W * L), -1, p)
NQUADS = 4096


@lru_cache(maxsize=None)
def quads():
    """[(a, b, c, d)], each an Fp2 value (c0 limbs, c1 limbs)"""
    rng = random.Random(0xF2A1E)
    fa, fb = field_operands()
    low = sum(WEAK << (W * i) for i in range(L - 1))
    top = low + ((64 * p - 1 - low) >> (W * (L - 1)) << (W * (L - 1)))          # the largest value below 64 p with every lower limb at 2^29 + 7
    mx, zero, pm1 = max_limbs(top), exact_limbs(0), exact_limbs(p - 1)
    MX, ZERO = (mx, mx), (zero, zero)
    out = [(MX, MX, MX, MX), (MX, MX, ZERO, ZERO), (ZERO, ZERO, MX, MX), (MX, ZERO, ZERO, MX), (ZERO, ZERO, ZERO, ZERO),
           ((zero, mx), (zero, mx), (mx, zero), (mx, zero)), ((mx, zero), (mx, zero), (zero, mx), (zero, mx))]          # c0 = -a1 b1: the most negative chain | the most positive
    some = lambda: exact_limbs(rng.randrange(p))
    for e in (zero, pm1):                                                       # 0 and p - 1 in each of the eight components alone
        for slot in range(8):
            comps = [some() for _ in range(8)]
            comps[slot] = e
            out.append(tuple((comps[2 * j], comps[2 * j + 1]) for j in range(4)))
    lift = lambda x: weak_limbs(x + rng.randrange(64) * p, rng)
    n = len(fa)
    for i in range(64):                                                         # a = c, b = d: both lanes of the pair must return the same product
        a, b = (lift(fa[i]), lift(fb[(i + 3) % n])), (lift(fb[i]), lift(fa[(i + 5) % n]))
        out.append((a, b, a, b))
    i = 0
    while len(out) < NQUADS:                                                    # eight different components per quadruple
        comps = [lift(x) for x in (fa[i], fb[(i + 3) % n], fb[i], fa[(i + 5) % n], fa[(i + 1) % n], fb[(i + 4) % n], fb[(i + 1) % n], fa[(i + 6) % n])]
        out.append(tuple((comps[2 * j], comps[2 * j + 1]) for j in range(4)))
        i += 1
    for q in out:
        for x in q:
            for l in x:
                assert all(v <= WEAK for v in l) and value(l) < 64 * p
    return out


def fp2_mont(x, y):
    return ((x[0] * y[0] - x[1] * y[1]) * RINV % p, (x[0] * y[1] + x[1] * y[0]) * RINV % p)


def test_lanewise_products_match_big_integers():
    qs = quads()
    n = len(qs)
    assert n == NQUADS
    vals = [tuple((value(x[0]), value(x[1])) for x in q) for q in qs]
    assert len(set(vals)) >= n - 8                                              # the cases are distinct (random components may repeat an edge row at most)
    unequal = [v for v in vals if v[0] != v[2] and v[1] != v[3] and len({c for x in v for c in x}) == 8]
    assert len(unequal) >= 3900                                                 # the two lanes of a pair hold unequal values, in every half
    assert sum(1 for v in vals if v[0] == v[2] and v[1] == v[3] and v[0][0] != v[0][1]) >= 64
    words = np.zeros((n, 4, 2, 16), dtype=np.uint32)
    for i, q in enumerate(qs):
        for j, x in enumerate(q):
            words[i, j, 0, :L], words[i, j, 1, :L] = x[0], x[1]
    out = np.zeros(3 * 96 * n, dtype=np.uint8)
    _lib.check(_lib.lib().zk_selftest_fp2_lanewise(words.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(n), out.ctypes.data_as(_lib._P8)))
    raw = out.tobytes()
    get = lambda i, k: tuple(int.from_bytes(raw[96 * (3 * i + k) + 48 * c:96 * (3 * i + k) + 48 * (c + 1)], "little") for c in (0, 1))
    bad = []
    for i, (a, b, c, d) in enumerate(vals):
        ab, cd = fp2_mont(a, b), fp2_mont(c, d)
        exp = [ab, cd, ((ab[0] - cd[0]) % p, (ab[1] - cd[1]) % p)]
        for k, e in enumerate(exp):
            if get(i, k) != e:
                bad.append((i, k))
    assert not bad, (len(bad), bad[:8])


def test_selftest_refuses_what_its_contract_excludes():
    lib = _lib.lib()
    out = (C.c_uint8 * (3 * 96))()
    ok = (C.c_uint32 * 128)()
    assert lib.zk_selftest_fp2_lanewise(None, 1, out) == -1 and lib.zk_selftest_fp2_lanewise(ok, 0, out) == -1 and lib.zk_selftest_fp2_lanewise(ok, 1, None) == -1
    bad = (C.c_uint32 * 128)()
    bad[16 * 5 + 3] = WEAK + 1
    assert lib.zk_selftest_fp2_lanewise(bad, 1, out) == -1
    bad = (C.c_uint32 * 128)()
    bad[16 * 7 + 13] = 64 * 13 + 1
    assert lib.zk_selftest_fp2_lanewise(bad, 1, out) == -1


# ---- a small G2 product through the public call
WINDOW = 16
REPEATS = 20


@lru_cache(maxsize=None)
def msm_case(n):
    cv = curve(1)
    rng = random.Random(0x165 + 16 * n)
    nrand = n - REPEATS - 3 - 1
    rand_pts = bytes(G2.of_Fr(RC.random_fr_bytes(nrand, 6100 + n)))
    rand_sc = [rng.randrange(1 << 200, 1 << 253) for _ in range(nrand)]
    bases = cv.p * REPEATS + cv.p1 + cv.neg(cv.p1) + cv.p2 + cv.inf + rand_pts
    scalars = [1] * REPEATS + [2, 2, 2] + [rng.randrange(1, 1 << 253)] + rand_sc
    ident = [False] * (REPEATS + 3) + [True] + [False] * nrand
    assert len(scalars) == n and len(bases) == n * G2.POINT_BYTES
    r = runs(scalars, WINDOW, False, ident)
    total = sum(cnt for _, cnt in r.values())
    assert r[0] == (0, REPEATS) and borders(r[0]) == 1          # the repeated base: one run from the first entry of a chunk across a chunk border
    assert r[1] == (REPEATS, 3)                                 # P, -P, Q: identity in mid-run, inside one chunk
    assert total % CHUNK == 7                                   # the last chunk holds an odd number of entries
    chunks = -(-total // CHUNK)
    assert chunks % 32 != 0 and (n < 1025 or chunks > 64)      # the last wave partly filled; at 1025 points more than one block of lane pairs
    sc = b"".join(P.fr_to_bytes(s) for s in scalars)
    rc, ref = cv.naive(bases, sc)
    assert rc == 0 and ref != cv.inf
    return bases, sc, ref


@pytest.mark.parametrize("inline", (0, 1))
@pytest.mark.parametrize("n", (65, 1025))
def test_small_g2_product_matches_the_naive_fold(n, inline):
    bases, sc, ref = msm_case(n)
    with options({"ZK_ACC_G2_INLINE": inline}):
        assert bytes(G2.apply_powers(sc, bases, WINDOW)) == ref
