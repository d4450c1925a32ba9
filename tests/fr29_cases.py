"""Operand classes of zk_selftest_fr29 (tests/test_gpu_fr_field.py), built so that the precondition of every output holds by construction, and what each
output must be, on Python integers only.  tests/test_fr29_model.py runs the same classes through the integer model without a GPU, so that the
expectations are checked before a device is."""
import random

import fr29_model as F

R, L, W, M, WEAK = F.R, F.L, F.W, F.M, F.WEAK
OMEGA_1024 = pow(7, (R - 1) >> 10, R)          # a primitive 2^10-th root of unity of Fr (7 generates the multiplicative group)


def with_small_limb(v, i, e):
    """v with limb i < 8 replaced by e in 0..7, so that a carry can be left pending there inside the weak range"""
    return v - ((((v >> (W * i)) & M) - e) << (W * i))


def representations(v, rnd, bound):
    """exact limbs, and -- where a value below bound * r can be had by giving one limb a value of 0..7 -- that value with a carry pending out of that
    limb: the limb + 2^29, the next limb - 1.  Returns [(kind, limbs)]."""
    out = [("exact", F.unpack(v))]
    l = F.unpack(v)
    for i in range(L - 1):          # the value itself, wherever one of its limbs is small enough
        p = F.pending(l, i)
        if p is not None:
            out.append(("pending", p))
    i, e = rnd.randrange(L - 1), rnd.randrange(8)
    v2 = with_small_limb(v, i, e)
    if 0 <= v2 < bound * R:
        p = F.pending(F.unpack(v2), i)
        if p is not None:
            out.append(("pending", p))
    return out


def reduce_cases(seed=0xF29):
    """[(label, limbs)] of values below 64 r for fr9_canon_pack / fr9_reduce_weak"""
    rnd = random.Random(seed)
    out = []
    for k in range(64):
        small = rnd.randrange(1, 1 << rnd.randrange(1, 200))
        for d in (0, 1, 2, R - 2, R - 1, R // 2, rnd.randrange(R), small, R - small):
            for kind, l in representations(k * R + d, rnd, k + 1):
                out.append((kind, l))
    for top in (0, 1, F.MOD[L - 1], 5 * F.MOD[L - 1] + 3, F.TOP_64R - 1):          # a carry that ripples through all nine limbs
        l = [WEAK] + [M] * (L - 2) + [top]
        assert F.val(l) < 64 * R
        out.append(("ripple", l))
    # a top limb that is an exact multiple k D of the estimate's divisor D = (r >> 232) + 1: top * QMUL >> 50 lands on k by the margin of the rounding
    # of QMUL alone (a multiplier one smaller gives k - 1 here, and only here)
    D = (R >> (W * (L - 1))) + 1
    for k in range(1, 64):
        for low in (0, (1 << (W * (L - 1))) - 1, rnd.randrange(1 << (W * (L - 1)))):
            v = ((k * D) << (W * (L - 1))) + low
            assert v < 64 * R and v // R == k
            out.append(("top limb k D", F.unpack(v)))
    out.append(("largest", F.unpack(64 * R - 1)))
    for kind, l in representations(64 * R - 1 - rnd.randrange(1 << 60), rnd, 64):
        out.append((kind if kind == "pending" else "largest", l))
    return out


def reduce_class(l):
    """which way the quotient estimate went"""
    _, q = F.reduce_weak_q(l)
    Q = F.val(l) // R
    assert q in (Q, Q - 1)
    return "estimate exact, no subtraction" if q == Q else "estimate short by one, subtraction taken"


PRODUCT_BOUNDS = (1, 2, 3, 8, 16, 48, 56, 64)


def _at_bound(rnd, bound, top):
    return bound * R - 1 - rnd.randrange(1 << rnd.randrange(1, 200)) if top else rnd.randrange(bound * R)


def product_cases(seed=0xF2A, per_pair=6):
    """[(label, A, B, u, v)]: u < A r, v < B r, A * B <= 64, at the top of the bounds and at random, in both limb representations"""
    rnd = random.Random(seed)
    out = []
    for A in PRODUCT_BOUNDS:
        B = 64 // A
        for top_u, top_v in ((True, True), (True, False), (False, True), (False, False)):
            for _ in range(per_pair):
                us = representations(_at_bound(rnd, A, top_u), rnd, A)
                vs = representations(_at_bound(rnd, B, top_v), rnd, B)
                for ku, u in (us[0], us[-1]):
                    for kv, v in (vs[0], vs[-1]):
                        out.append(("top" if top_u and top_v else "mixed" if top_u or top_v else "random", ku, kv, A, B, u, v))
        out.append(("top", "exact", "exact", A, B, F.unpack(A * R - 1), F.unpack(B * R - 1)))
    return out


def factors(rnd):
    """canonical factors as memory holds them: exact limbs, below r"""
    j = rnd.randrange(512)
    return [0, 1, R - 1, pow(OMEGA_1024, j, R) * F.RP % R, F.RP % R, rnd.randrange(R), rnd.randrange(R)]


def forward_cases(seed=0xF2B, count=40):
    """[(label, u, v, w)]: u, v < 24 r (the bound before the fourth stage of a DIF group), K = 32 r"""
    rnd = random.Random(seed)
    top = 24 * R - 1
    pairs = [("v at the bound", 0, top), ("v at the bound", 1, top), ("v at the bound", rnd.randrange(R), top), ("both at the bound", top, top),
             ("u = v", 0, 0), ("u at the bound", top, 0), ("u at the bound", top, 1)]
    for _ in range(count):
        x = _at_bound(rnd, 24, rnd.random() < 0.5)
        pairs.append(("u = v", x, x))
        pairs.append(("v above u + 16 r", rnd.randrange(7 * R), 24 * R - 1 - rnd.randrange(R)))
        pairs.append(("random", rnd.randrange(24 * R), rnd.randrange(24 * R)))
    out = []
    for label, u, v in pairs:
        ws = factors(rnd)
        for w in ws if label != "random" else ws[3:5]:
            ur, vr = representations(u, rnd, 24), representations(v, rnd, 24)
            out.append((label, ur[0][1], vr[0][1], F.unpack(w)))
            if ur[-1][0] == "pending" or vr[-1][0] == "pending":
                out.append((label + ", pending carry", ur[-1][1], vr[-1][1], F.unpack(w)))
    return out


def inverse_cases(seed=0xF2C, count=60):
    """[(label, u, v, w)]: u < 38 r, v < 42 r (the last DIT stage of ten)"""
    rnd = random.Random(seed)
    pairs = [("at the bounds", 38 * R - 1, 42 * R - 1), ("at the bounds", 0, 42 * R - 1), ("at the bounds", 38 * R - 1, 0), ("zero", 0, 0)]
    for _ in range(count):
        pairs.append(("random", _at_bound(rnd, 38, rnd.random() < 0.3), _at_bound(rnd, 42, rnd.random() < 0.3)))
    out = []
    for label, u, v in pairs:
        ws = factors(rnd)
        for w in ws if label != "random" else ws[3:5]:
            ur, vr = representations(u, rnd, 38), representations(v, rnd, 42)
            out.append((label, ur[0][1], vr[0][1], F.unpack(w)))
            if ur[-1][0] == "pending" or vr[-1][0] == "pending":
                out.append((label + ", pending carry", ur[-1][1], vr[-1][1], F.unpack(w)))
    return out


def word_cases(seed=0xF2D):
    """8-word values for the pack / unpack round trip: any 256-bit pattern"""
    rnd = random.Random(seed)
    out = [0, (1 << 256) - 1, R, R - 1, (1 << 255), 1]
    out += [1 << (W * i) for i in range(L)] + [(1 << (W * i)) - 1 for i in range(1, L)] + [1 << (32 * j) for j in range(8)]
    out += [((1 << 256) - 1) ^ (M << (W * i)) for i in range(L - 1)]
    out += [rnd.getrandbits(256) for _ in range(64)]
    return out


def is_exact(l):
    return all(0 <= x <= M for x in l[:L - 1])


def is_weak(l):
    return all(0 <= x <= WEAK for x in l[:L - 1])


def check_forward(u, v, w, x, xs, y, y_carried, y2):
    """what the five outputs of op 3 must be, by integers alone"""
    U, V, Wv = F.val(u), F.val(v), F.val(w)
    assert F.val(x) == U + V and F.val(x) < 48 * R and is_weak(x)
    assert F.val(xs) % R == (U + V) % R and F.val(xs) < 2 * R and is_exact(xs)
    assert (F.val(y) * F.RP - (U - V) * Wv) % R == 0 and F.val(y) < 2 * R and is_exact(y)
    assert list(y_carried) == list(y), "sub_raw then mul differs from sub then mul"
    assert F.val(y2) == U - V + 32 * R and F.val(y2) < 56 * R and is_weak(y2)


def check_inverse(u, v, w, t, x, y):
    U, V, Wv = F.val(u), F.val(v), F.val(w)
    assert (F.val(t) * F.RP - V * Wv) % R == 0 and F.val(t) < 2 * R and is_exact(t)
    assert F.val(x) == U + F.val(t) and F.val(x) < 40 * R and is_weak(x)
    assert F.val(y) == U - F.val(t) + 4 * R and F.val(y) < 42 * R and is_weak(y)
