"""The paired field products (csrc/fp_pair_gen.cuh) and the group law rebuilt on them, against Python integers and the oracle.

Where the base-field products are expanded in place, independent products of a group addition run side by side: the multiply-adds of two (at the end of
an addition, three) products alternate, one accumulator chain per column each.  What can go wrong is a carry or a quotient digit of one chain reaching
another, an operand register shared or overwritten between the chains, or a column bound missed at the largest limbs the forms admit:

  * zk_selftest_fp_paired on the 4096 operand pairs of tests/test_gpu_field.py, lifted to the at-rest bound 64 p in weakly normalised limbs, and on
    0, 1, p - 1 and 64 p - 1 with every limb at 2^29 + 7, one all-maximum product beside one all-zero product both ways round, shared operands
    (a = c, b = d, a = d) and outputs written over inputs -- exact, against integers;
  * the mixed additions with the products expanded in place on table entries and on affine points (zk_selftest_group forms 7 and 8, xyzz_madd_impl in
    msm_acc_g1.hip): the two forms that issue the pairs, in G1.  Beside them, as regression cover of code this change does not touch: the same two
    forms in G2, the 6-product addition in place (form 9), the mixed additions out of line, the general addition and its from-memory form.  Every
    form on P + Q, P + P, P + (-P), an identity on either side and 64 distinct random pairs, canonical and lifted;
  * zk_msm_g1 / zk_msm_g2 at 1, 17 and 33 points (a chunk's first, second and seventeenth step) and at 2^12 points with every scalar equal (runs cross
    chunk borders; the fix-up and the digit sums run), against the oracle's naive fold.
No tolerances anywhere."""
import ctypes as C
import random
from functools import lru_cache

import numpy as np
import pytest

import group_law_cases as GL
import oracle_lib as O
from oracle import pyref as P
from test_gpu_field import operands as field_operands
from zukelang_amd import _lib
from zukelang_amd import r1cs as RC
from zukelang_amd.curve import G1, G2

pytestmark = pytest.mark.gpu
p = P.P
W, L, NOUT = 29, 14, 13
WEAK = (1 << W) + 7
RINV = pow(1 << (W * L), -1, p)


def exact_limbs(v):
    return [(v >> (W * i)) & ((1 << W) - 1) for i in range(L - 1)] + [v >> (W * (L - 1))]


def weak_limbs(v, rng):
    """v < 64 p in a weakly normalised form that is not the exact one: limbs borrow 2^29 from the limb above where that keeps them <= 2^29 + 7"""
    l = exact_limbs(v)
    for i in range(L - 1):
        if l[i] <= 7 and l[i + 1] > 0 and rng.random() < 0.75:
            l[i] += 1 << W
            l[i + 1] -= 1
    return l


def max_limbs(v):
    """v with every limb below the top one at 2^29 + 7 (v large enough)"""
    low = sum(WEAK << (W * i) for i in range(L - 1))
    top, rest = divmod(v - low, 1 << (W * (L - 1)))
    assert v >= low and rest == 0
    return [WEAK] * (L - 1) + [top]


def value(l):
    return sum(x << (W * i) for i, x in enumerate(l))


@lru_cache(maxsize=None)
def lanes():
    rng = random.Random(0x2A12ED)
    a, b = field_operands()
    assert len(a) >= 4096
    lift = lambda x: weak_limbs(x + rng.randrange(64) * p, rng)
    quads = [[lift(a[i]), lift(b[i]), lift(a[(i + 1) % len(a)]), lift(b[(i + 1) % len(a)])] for i in range(len(a))]
    low = sum(WEAK << (W * i) for i in range(L - 1))
    top = low + ((64 * p - 1 - low) >> (W * (L - 1)) << (W * (L - 1)))          # the largest value below 64 p with every lower limb at 2^29 + 7
    assert 63 * p < top < 64 * p
    edge = [exact_limbs(0), exact_limbs(1), exact_limbs(p - 1), exact_limbs(64 * p - 1), max_limbs(top)]
    for x in edge:
        for y in edge:
            quads.append([x, y, y, x])
            quads.append([x, x, y, y])
    mx, zero = max_limbs(top), exact_limbs(0)
    quads += [[mx, mx, zero, zero], [zero, zero, mx, mx], [mx, mx, mx, mx], [mx, zero, zero, mx]]          # a leak between the chains shows here
    for q in quads:
        for l in q:
            assert all(x <= WEAK for x in l) and value(l) < 64 * p
    return quads


def test_paired_products_match_big_integers():
    quads = lanes()
    n = len(quads)
    words = np.zeros((n, 4, 16), dtype=np.uint32)
    for i, q in enumerate(quads):
        for j, l in enumerate(q):
            words[i, j, :L] = l
    out = np.zeros(NOUT * 48 * n, dtype=np.uint8)
    _lib.check(_lib.lib().zk_selftest_fp_paired(words.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(n), out.ctypes.data_as(_lib._P8)))
    raw = out.tobytes()
    get = lambda i, k: int.from_bytes(raw[48 * (NOUT * i + k):48 * (NOUT * i + k + 1)], "little")
    mont = lambda x: x * RINV % p
    for i, q in enumerate(quads):
        a, b, c, d = (value(l) for l in q)
        exp = [mont(a * b), mont(c * d), mont(a * a), mont(c * c), mont(a * b), mont(a * b), mont(a * b), mont(c * a), mont(a * b), mont(c * d),
               mont(a * b - c * d), mont(a * d), mont(c * b)]
        for k, e in enumerate(exp):
            assert get(i, k) == e, (i, k, [hex(x) for x in (a, b, c, d)])


def test_selftest_refuses_what_its_contract_excludes():
    lib = _lib.lib()
    out = (C.c_uint8 * (NOUT * 48))()
    ok = (C.c_uint32 * 64)()
    assert lib.zk_selftest_fp_paired(None, 1, out) == -1 and lib.zk_selftest_fp_paired(ok, 0, out) == -1 and lib.zk_selftest_fp_paired(ok, 1, None) == -1
    bad = (C.c_uint32 * 64)()
    bad[3] = WEAK + 1
    assert lib.zk_selftest_fp_paired(bad, 1, out) == -1
    bad = (C.c_uint32 * 64)()
    bad[16 + 13] = 64 * 13 + 1
    assert lib.zk_selftest_fp_paired(bad, 1, out) == -1


# ---- the group law: madd_inline and madd_table_inline issue the pairs in G1; every other row (and all of G2) runs code this change leaves as it was
PAIRED_FORMS = ["add", "add_raw_mem", "madd", "madd_table", "madd_inline", "madd_table_inline", "mmadd_inline"]
RANDOM_PAIRS = 64
# 64 points, generic case i = (pts[i], pts[(7 i + 3) mod 64]): 64 distinct pairs of distinct points, each in every representation of either side
battery = lru_cache(maxsize=None)(lambda group: GL.battery(group, seed=0x2A1D, points=RANDOM_PAIRS, generic=RANDOM_PAIRS, special=4))


def takes(form, pair):
    f = GL.FORMS[form]
    return not (f.second == "table" and pair.b_aff is None) and not (f.needs_affine_a and pair.a_rep not in ("one",) + GL.IDENTITIES)


@pytest.mark.parametrize("rep", (0, 1))
@pytest.mark.parametrize("form", PAIRED_FORMS)
@pytest.mark.parametrize("group", (0, 1))
def test_additions_on_paired_products_match_the_oracle(group, form, rep):
    f = GL.FORMS[form]
    g, pairs, _ = battery(group)
    mine = [x for x in pairs if takes(form, x)]
    seen = {x.cls for x in mine}
    assert {"generic", "P+P", "P-P", "O+P"} <= seen and (f.second == "table" or "P+O" in seen)
    generic = [x for x in mine if x.cls == "generic"]
    assert len({x.expected for x in generic}) >= RANDOM_PAIRS and len({(g.aff_bytes(x.b_aff), x.expected) for x in generic}) >= RANDOM_PAIRS          # distinct (P, Q)
    a = b"".join(g.xyzz_bytes(x.a) for x in mine)
    b = b"".join(g.xyzz_bytes(x.b_xyzz) if f.second == "xyzz" else g.aff_bytes(x.b_aff) for x in mine)
    size = 192 if group else 96
    out = C.create_string_buffer(size * len(mine))
    u8 = lambda x: C.cast(C.c_char_p(x), _lib._P8)
    _lib.check(_lib.lib().zk_selftest_group(group, f.number, rep, u8(a), u8(b), len(mine), C.cast(out, _lib._P8)))
    bad = [(i, x.cls, x.a_rep, x.b_rep) for i, x in enumerate(mine) if out.raw[size * i:size * (i + 1)] != x.expected]
    assert not bad, (form, group, rep, len(bad), bad[:8])


# ---- the MSMs whose kernels issue the pairs
@pytest.mark.parametrize("n", (1, 17, 33))
@pytest.mark.parametrize("G,naive", [(G1, O.g1_msm_naive), (G2, O.g2_msm_naive)])
def test_short_msm_matches_the_naive_fold(G, naive, n):
    bases = G.of_Fr(RC.random_fr_bytes(n, 5100 + n))
    scalars = RC.random_fr_bytes(n, 5200 + n)
    rc, ref = naive(bytes(bases), bytes(scalars))
    assert rc == 0 and bytes(G.apply_powers(scalars, bases)) == ref


@pytest.mark.parametrize("G,naive", [(G1, O.g1_msm_naive), (G2, O.g2_msm_naive)])
def test_msm_with_every_scalar_equal_matches_the_naive_fold(G, naive):
    """2^12 points, one scalar: every window files all 4096 points into ONE bucket, so a run spans every chunk of the window -- heads, tails, the fix-up
    that joins them and the digit sums all run"""
    n = 1 << 12
    bases = G.of_Fr(RC.random_fr_bytes(n, 5300))
    scalars = bytes(RC.random_fr_bytes(1, 5301)) * n
    rc, ref = naive(bytes(bases), scalars)
    assert rc == 0 and bytes(G.apply_powers(scalars, bases)) == ref
