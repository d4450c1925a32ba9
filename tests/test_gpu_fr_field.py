"""GPU parity of the scalar field, both layers, against Python integers mod r.

zk_selftest_fr: the 8 x 32-bit Fe<FrParams> of csrc/ff.cuh -- the generated Montgomery product, add / sub / neg / cond_sub, the binary-Euclid inverse,
fe_from_u32, fe_is_canonical: the arithmetic of zk_fr_spmv, the R1CS check, the tables and every to/from-Montgomery pass -- on the operands where a
borrow or a carry decides: r - 1, a + b = r, words of all ones.
zk_selftest_fr29: the lazily reduced 9 x 29-bit integers of csrc/fr29.cuh on raw limbs, placed at the bounds of the stage schedule of csrc/ntt_lds.cuh
(24 r against K = 32 r, 38 r and 42 r in the inverse butterfly, operand bounds A * B = 64, both branches of the quotient estimate, a carry rippling
through all nine limbs), which no input of zk_fr_ntt reaches.  Every output is held to its value congruence, its documented value bound, exact limbs
where the header says so, and limb for limb to the integer model tests/fr29_model.py; tests/fr29_cases.py builds the classes, each counted."""
import ctypes as C
import random

import numpy as np
import pytest

import fr29_cases as K
import fr29_model as F
from zukelang_amd import _lib

pytestmark = pytest.mark.gpu
r = F.R
NOUT = 14
P32 = C.POINTER(C.c_uint32)


def le32(x):
    return int(x).to_bytes(32, "little")


def blob(values):
    """32-byte little-endian integers back to back, as an array the call can take a pointer to"""
    return np.frombuffer(b"".join(le32(x) for x in values), dtype=np.uint8)


def operands():
    rnd = random.Random(0xF2E1D)
    top = r >> 224
    edge = [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2,
            (1 << 32) - 1, 1 << 32, (1 << 64) - 1, (1 << 255) % r,
            (1 << 256) % r, (1 << 512) % r, (1 << 768) % r,
            r - (1 << 32), r - (1 << 224),
            (1 << 224) - 1, ((top - 1) << 224) | ((1 << 224) - 1), (top << 224) | ((1 << 64) - 1),          # all-ones words below r's top word
            (0x12345678 << 224) | 0x9ABCDEF0, (1 << 192) + 1, (0x7FFFFFFF << 192) | (0xFFFFFFFF << 64) | 1,          # zero words in the middle
            (1 << 232) - 1, ((1 << 261) - 1) % r, sum(F.M << (58 * i) for i in range(4)), F.M, 1 << 29, (1 << 58) - 1]          # 29-bit limbs of all ones
    assert all(0 <= x < r for x in edge)
    a, b = [], []
    for x in edge:
        for y in (0, 1, r - 1, x, (r - x) % r, rnd.randrange(r)):
            a.append(x); b.append(y)
    for _ in range(4096 - len(a)):
        a.append(rnd.randrange(r)); b.append(rnd.randrange(r))
    return a, b


def test_word_field_battery_matches_big_integers():
    a, b = operands()
    n = len(a)
    assert n == 4096
    out = np.zeros(NOUT * 32 * n, dtype=np.uint8)
    ab, bb = blob(a), blob(b)
    _lib.check(_lib.lib().zk_selftest_fr(0, ab.ctypes.data_as(_lib._P8), bb.ctypes.data_as(_lib._P8), n, out.ctypes.data_as(_lib._P8)))
    raw = out.tobytes()
    get = lambda i, k: int.from_bytes(raw[32 * (NOUT * i + k):32 * (NOUT * i + k + 1)], "little")
    seen = {"a = b": 0, "a + b = r": 0, "a = 0": 0, "a - b borrows": 0, "a + b >= r": 0}
    for i in range(n):
        x, y = a[i], b[i]
        exp = [(x + y) % r, (x - y) % r, (y - x) % r, x * y % r, x * x % r, (-x) % r, 2 * x % r, pow(x, r - 2, r),
               x, (x & 0xFFFFFFFF) % r, (x * y % r + x * x % r + y * y % r) % r, (1 if x == 0 else 0) | (2 if x == y else 0), x, x * y % r]
        assert len(exp) == NOUT
        for k, e in enumerate(exp):
            assert get(i, k) == e, (i, k, hex(x), hex(y), hex(get(i, k)))
        seen["a = b"] += x == y
        seen["a + b = r"] += x + y == r
        seen["a = 0"] += x == 0
        seen["a - b borrows"] += x < y
        seen["a + b >= r"] += x + y >= r
    assert all(seen.values()), seen


def test_inverses_whose_montgomery_residue_is_the_edge():
    """Added rows for output 7.  fe_inv runs words_inv on the Montgomery residue a * 2^256 mod r, so the edge operands above arrive as what are in effect
    random integers.  Here a = A * 2^-256 mod r for A in 1, 2, r - 1, 2^k, r - 2^k and the A that drive the outer loop of words_inv longest in its
    integer restatement (fp29_model.words_inv; tests/fp29_cases.py searches with a fixed seed).  The largest count found is 203, against the guard
    4 * 32 * 8 = 1024."""
    import fp29_cases as Cs
    import fp29_model as FP
    table = Cs.fr_words_inv_operands()
    assert {1, 2, r - 1, 1 << 252, r - (1 << 7)} <= set(table) and len(table) >= 64
    assert 200 <= max(table.values()) < Cs.FR_GUARD // 4, max(table.values())
    rinv = pow(2, -256, r)
    a = [A * rinv % r for A in table]
    b = [1] * len(a)
    out = np.zeros(NOUT * 32 * len(a), dtype=np.uint8)
    ab, bb = blob(a), blob(b)
    _lib.check(_lib.lib().zk_selftest_fr(0, ab.ctypes.data_as(_lib._P8), bb.ctypes.data_as(_lib._P8), len(a), out.ctypes.data_as(_lib._P8)))
    raw = out.tobytes()
    for i, (A, x) in enumerate(zip(table, a)):
        assert x * (1 << 256) % r == A and FP.words_inv(A, r)[0] == pow(A, -1, r)
        got = int.from_bytes(raw[32 * (NOUT * i + 7):32 * (NOUT * i + 8)], "little")
        assert got == pow(x, r - 2, r), (hex(A), table[A])


def test_is_canonical_decides_the_borrow_chain_at_every_word():
    word = lambda k: 1 << (32 * k)
    vals = [r - 1, r, r + 1, (1 << 256) - 1, 0]
    for k in range(8):
        if (r >> (32 * k)) & 0xFFFFFFFF:
            vals.append(r - word(k))                     # word k decremented: below r whatever the words under it hold
        if (r >> (32 * k)) & 0xFFFFFFFF != 0xFFFFFFFF and r + word(k) < 1 << 256:
            vals.append(r + word(k))                     # word k incremented
        vals.append((r >> (32 * k) << (32 * k)) | (word(k) - 1))          # r's words from k up, all ones below: >= r
        vals.append((r >> (32 * k) << (32 * k)))                            # r's words from k up, zeros below: < r (r's word 0 is 1), = r for k = 0
    vals = [v for v in vals if 0 <= v < 1 << 256]
    out = np.full(len(vals), 9, dtype=np.uint8)
    vb = blob(vals)
    _lib.check(_lib.lib().zk_selftest_fr(1, vb.ctypes.data_as(_lib._P8), None, len(vals), out.ctypes.data_as(_lib._P8)))
    assert [int(x) for x in out] == [1 if v < r else 0 for v in vals], [hex(v) for v, x in zip(vals, out) if int(x) != (v < r)]
    assert sum(v < r for v in vals) >= 8 and sum(v >= r for v in vals) >= 8


# ---------------------------------------------------------------------------------------------- raw limbs
OUT_WORDS = {0: 8, 1: 9, 2: 9, 3: 45, 4: 27, 5: 8}
ZERO = [0] * F.L


def run29(op, lanes):
    """lanes: [(u, v, w)] as lists of 9 limbs -> one list of output words per lane"""
    flat = np.array([x for u, v, w in lanes for l in (u, v, w) for x in l], dtype=np.uint32)
    assert flat.size == 27 * len(lanes)
    out = np.zeros(OUT_WORDS[op] * len(lanes), dtype=np.uint32)
    _lib.check(_lib.lib().zk_selftest_fr29(op, flat.ctypes.data_as(P32), len(lanes), out.ctypes.data_as(P32)))
    return [[int(x) for x in row] for row in out.reshape(len(lanes), OUT_WORDS[op])]


def test_canonical_pack_and_weak_reduction_on_both_branches_of_the_quotient_estimate():
    cases = K.reduce_cases()
    lanes = [(l, ZERO, ZERO) for _, l in cases]
    packed, weak = run29(0, lanes), run29(1, lanes)
    seen = {}
    for (kind, l), p, w in zip(cases, packed, weak):
        v = F.val(l)
        assert v < 64 * r
        cls = K.reduce_class(l)
        for c in (kind, cls):
            seen[c] = seen.get(c, 0) + 1
        assert p == F.words8(v % r), (kind, cls, [hex(x) for x in l])                                   # the value, fully reduced, as 8 words
        assert F.val(w) % r == v % r and F.val(w) < 2 * r and K.is_exact(w), (kind, cls, [hex(x) for x in l])
        assert (F.val(w) >= r) == (cls == "estimate short by one, subtraction taken")
        assert w == F.reduce_weak(l) and p == F.canon_pack(l), (kind, cls)                              # limb for limb what the model computes
    assert set(seen) == {"exact", "pending", "ripple", "largest", "top limb k D", "estimate exact, no subtraction", "estimate short by one, subtraction taken"}, seen
    assert min(seen.values()) >= 2 and seen["pending"] >= 64, seen


def test_products_at_the_top_of_every_bound_pair():
    cases = K.product_cases()
    got = run29(2, [(u, v, ZERO) for *_, u, v in cases])
    kinds = set()
    for (label, ku, kv, A, B, u, v), p in zip(cases, got):
        assert A * B <= 64 and F.val(u) < A * r and F.val(v) < B * r
        assert (F.val(p) * F.RP - F.val(u) * F.val(v)) % r == 0, (label, A, B)          # p = u v / 2^261
        assert F.val(p) < 2 * r and K.is_exact(p), (label, A, B)
        assert p == F.mul(u, v), (label, A, B)
        kinds.add((label, ku, kv, A))
    for A in K.PRODUCT_BOUNDS:
        assert {(lab, "exact", "exact", A) for lab in ("top", "mixed", "random")} <= kinds
        assert any(k[3] == A and "pending" in k[1:3] for k in kinds), A


def test_forward_butterfly_at_24_r_against_32_r():
    cases = K.forward_cases()
    got = run29(3, [(u, v, w) for _, u, v, w in cases])
    seen = {}
    for (label, u, v, w), o in zip(cases, got):
        x, xs, y, yc, y2 = (o[9 * k:9 * k + 9] for k in range(5))
        K.check_forward(u, v, w, x, xs, y, yc, y2)
        mx = F.add(u, v)
        assert [x, xs, y, yc, y2] == [mx, F.reduce_weak(mx), F.mul(F.sub_raw(u, v, 5), w), F.mul(F.sub(u, v, 5), w), F.sub(u, v, 5)], label
        seen[label] = seen.get(label, 0) + 1
    assert {"v at the bound", "both at the bound", "u = v", "u at the bound", "v above u + 16 r", "random"} <= set(seen), seen
    assert any("pending" in s for s in seen), seen


def test_inverse_butterfly_at_38_r_and_42_r():
    cases = K.inverse_cases()
    got = run29(4, [(u, v, w) for _, u, v, w in cases])
    seen = {}
    for (label, u, v, w), o in zip(cases, got):
        t, x, y = (o[9 * k:9 * k + 9] for k in range(3))
        K.check_inverse(u, v, w, t, x, y)
        mt = F.mul(v, w)
        assert [t, x, y] == [mt, F.add(u, mt), F.sub(u, mt, 2)], label
        seen[label] = seen.get(label, 0) + 1
    assert {"at the bounds", "zero", "random"} <= set(seen) and any("pending" in s for s in seen), seen


def test_unpack_then_pack_is_the_identity_on_any_256_bits():
    vals = K.word_cases()
    got = run29(5, [(F.words8(v) + [0xFFFFFFFF], ZERO, ZERO) for v in vals])          # the ninth word of the slot is not read
    for v, o in zip(vals, got):
        assert o == F.words8(v), hex(v)
        assert o == F.pack_exact(F.unpack_words(F.words8(v)))
