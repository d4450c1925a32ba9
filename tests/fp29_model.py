"""Integer model of the base-field layer of zukelang_amd/csrc/ff.cuh and fp_inv.cuh (Fp on 14 limbs of 29 bits, Montgomery R = 2^406), importable and
without side effects.

  * the constants of fp29_consts.cuh, parsed from the header (MOD, NINV, PINV, R1-R3, KP, KPN, KPW, FP29_PTOP_INV);
  * fp_carry, fe_add, fe_sub, fe_neg, fe_neg_lazy, fe_sub_sub_dbl, fe_dbl, fp_canon_call, fe_is_zero (both slow paths), fp_pack / fp_unpack and
    fp_inv29_call restated limb for limb on lists of 14 integers.  Each asserts what the device code relies on without checking: no limb reaches 2^32
    before a carry pass, no limb of a subtraction borrows, results are weakly normalised, the quotient estimate is within two of the quotient, every
    int64 accumulator of the inversion stays inside 63 bits and every signed limb inside int32, a = 0 and b = 1 after the last iteration.  Where those
    hold the lists are what the device computes, limb for limb (tests/test_gpu_fp29.py compares them with zk_selftest_fp29).

fp_canon_call's quotient estimate is IEEE single precision on the device: (float)t13 and (float)t12 round to nearest-even (v_cvt_f32_u32), the product by
2^29 is exact, the sum and the product by FP29_PTOP_INV round to nearest-even, the conversion to uint32 truncates.  numpy.float32 does the same.

inv29() takes the iteration count and the `exact` threshold as arguments so that tests/test_fp29_model.py can show what a build with other values
would do; the defaults are the header's."""
import os
import re

import numpy as np

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
W, L, M = 29, 14, (1 << 29) - 1
U32 = 0xFFFFFFFF
WEAK = (1 << W) + 7                    # a weakly normalised limb: at most this
RBITS = W * L                          # 406
TOPSHIFT = W * (L - 1)                 # 377
FP_MAX_BOUND = 8192
FP_REST = 64
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zukelang_amd", "csrc")
CONSTS_PATH = os.path.join(CSRC, "fp29_consts.cuh")


def parse_consts(path=CONSTS_PATH):
    src = open(path).read()

    def arr(name):
        body = re.search(name + r"(?:\[\d+\])+ = \{(.*?)\};", src, re.S).group(1)
        return [int(x, 16) for x in re.findall(r"0x([0-9a-f]+)u", body)]

    def rows(name):
        flat = arr(name)
        return [flat[L * k:L * k + L] for k in range(len(flat) // L)]

    def scalar(name):
        return int(re.search(name + r" = 0x([0-9a-f]+)u", src).group(1), 16)
    return {"MOD": arr("FP29_MOD"), "R1": arr("FP29_R1"), "R2": arr("FP29_R2"), "R3": arr("FP29_R3"), "KP": rows("FP29_KP"), "KPN": rows("FP29_KPN"),
            "KPW": rows("FP29_KPW"), "NINV": scalar("FP29_NINV"), "PINV": scalar("FP29_PINV"), "NK": int(re.search(r"FP29_NK = (\d+)", src).group(1)),
            "PTOP_INV": re.search(r"FP29_PTOP_INV = ([0-9.e+-]+)f;", src).group(1)}


_C = parse_consts()
MOD, R1, R2, R3, KP, KPN, KPW, NINV, PINV, NK = (_C[k] for k in ("MOD", "R1", "R2", "R3", "KP", "KPN", "KPW", "NINV", "PINV", "NK"))
PTOP_INV = np.float32(_C["PTOP_INV"])
# what the comments of fp29_consts.cuh and ff.cuh state about limbs 0..12 of each table: [lo, hi]
# (the upper end of KP and KPW is what keeps a limb of a + (K p - b) below 2^32 for a weakly normalised a)
SPREAD = {"KP": ((1 << 30) - 2, U32 - WEAK), "KPN": ((1 << 29) + 8, (1 << 30) - 2), "KPW": ((1 << 31) - 4, U32 - WEAK)}
TABLES = {"KP": KP, "KPN": KPN, "KPW": KPW}


def fp_ks(b):
    k = 2
    while k < b + 1:
        k <<= 1
    return k


def fp_ki(k):
    i = 0
    while (2 << i) < k:
        i += 1
    return i


def val(l):
    return sum(x << (W * i) for i, x in enumerate(l))


def unpack(v):
    """exact limbs of a non-negative integer below 2^(377 + 32)"""
    assert 0 <= v < 1 << (TOPSHIFT + 32)
    return [(v >> (W * i)) & M for i in range(L - 1)] + [v >> TOPSHIFT]


def top_limb_of(bound):
    """the largest top limb of an exact-limb value below bound * p"""
    return (bound * P - 1) >> TOPSHIFT


def pending(l, i):
    """the same value with a carry pending out of limb i < 13: limb i + 2^29, limb i + 1 - 1 (None where limb i + 1 is zero or limb i leaves the weak range)"""
    if l[i + 1] == 0 or l[i] + (1 << W) > WEAK:
        return None
    r = list(l)
    r[i] += 1 << W
    r[i + 1] -= 1
    return r


def weak_form(v, seed):
    """a weakly normalised form of v that is not the exact one, or None: the first limb from `seed` on that can hold a pending carry"""
    l = unpack(v)
    for d in range(L - 1):
        r = pending(l, (seed + d) % (L - 1))
        if r is not None:
            return r
    return None


def all_weak(top):
    """limbs 0..12 at 2^29 + 7, the top limb as given"""
    return [WEAK] * (L - 1) + [top]


def is_weak(l):
    return all(0 <= x <= WEAK for x in l[:L - 1]) and 0 <= l[L - 1] <= U32


def check_tables():
    """every row of every table is 2^(k+1) p with limbs 0..12 inside the stated spread and a non-negative top limb; KPW row 0 is unused (all zero)"""
    for name, t in TABLES.items():
        lo, hi = SPREAD[name]
        assert len(t) == NK == 13
        for k, row in enumerate(t):
            if name == "KPW" and k == 0:
                assert row == [0] * L
                continue
            assert val(row) == (2 << k) * P, (name, k)
            assert all(lo <= x <= hi for x in row[:L - 1]), (name, k)
            assert 0 <= row[L - 1] <= U32


# ---------------------------------------------------------------- the additive forms
def carry(t):
    """fp_carry: limbs 0..12 below 2^32 in (the top limb is taken modulo 2^32, as the device's register is), weakly normalised out"""
    assert all(0 <= x <= U32 for x in t[:L - 1]), "a limb reaches 2^32 before the carry pass"
    c = [x >> W for x in t[:L - 1]]
    r = [t[0] & M] + [(t[i] & M) + c[i - 1] for i in range(1, L - 1)] + [(t[L - 1] + c[L - 2]) & U32]
    assert is_weak(r)
    return r


def _exact(r, want):
    assert want >= 0 and val(r) == want, "the carry pass did not leave the exact value (top limb wrapped)"
    return r


def fe_add(a, b):
    assert is_weak(a) and is_weak(b)
    assert a[L - 1] + b[L - 1] <= U32
    return _exact(carry([x + y for x, y in zip(a, b)]), val(a) + val(b))


def fe_dbl(a):
    assert is_weak(a) and 2 * a[L - 1] <= U32
    return _exact(carry([x << 1 for x in a]), 2 * val(a))


def _row(table, bound, lo=0):
    ki = fp_ki(fp_ks(bound))
    assert lo <= ki < NK, "subtrahend bound out of range"
    return ki, TABLES[table][ki]


def fe_sub(a, b, bb):
    """fe_sub<A, B = bb>: a - b + fp_ks(bb) p; the caller's part is val(b) < bb p"""
    assert is_weak(a) and is_weak(b) and val(b) < bb * P
    _, k = _row("KP", bb)
    t = []
    for i in range(L):
        d = k[i] - b[i]
        if i < L - 1:
            assert d >= 0, "a limb of the subtraction borrows"
        t.append(a[i] + d if i < L - 1 else (a[i] + d) & U32)
    return _exact(carry(t), val(a) - val(b) + fp_ks(bb) * P)


def fe_neg(a, ab):
    assert is_weak(a) and val(a) < ab * P
    _, k = _row("KP", ab)
    t = []
    for i in range(L):
        d = k[i] - a[i]
        if i < L - 1:
            assert d >= 0, "a limb of the negation borrows"
        t.append(d & U32)
    return _exact(carry(t), fp_ks(ab) * P - val(a))


def fe_neg_lazy(a, ab):
    """K p - a with NO carry pass: limbs in [1, 2^30], the top limb non-negative"""
    assert is_weak(a) and val(a) < ab * P
    _, k = _row("KPN", ab)
    r = [k[i] - a[i] for i in range(L)]
    assert all(1 <= x <= 1 << 30 for x in r[:L - 1]), "a lazily negated limb leaves [1, 2^30]"
    assert 0 <= r[L - 1] <= U32, "the top limb of the lazy negation borrows"
    assert val(r) == fp_ks(ab) * P - val(a)
    return r


def fe_sub_sub_dbl(a, b, c, bb, cb):
    """fe_sub_sub_dbl<A, bb, cb>: a - b - 2 c + fp_ks(bb + 2 cb) p"""
    assert is_weak(a) and is_weak(b) and is_weak(c) and val(b) < bb * P and val(c) < cb * P
    _, k = _row("KPW", bb + 2 * cb, lo=1)
    t = []
    for i in range(L):
        d = k[i] - b[i] - (c[i] << 1)
        if i < L - 1:
            assert d >= 0, "a limb of the double subtraction borrows"
        t.append(a[i] + d if i < L - 1 else (a[i] + d) & U32)
    return _exact(carry(t), val(a) - val(b) - 2 * val(c) + fp_ks(bb + 2 * cb) * P)


# ---------------------------------------------------------------- full reduction and the zero test
def _exact_limbs_u32(a):
    """the serial pass at the head of fp_canon_call and fp_is_zero_mod_p_inline, on 32-bit registers"""
    t = list(a)
    for i in range(L - 1):
        t[i + 1] += t[i] >> W
        assert t[i + 1] <= U32, "a limb overflows in the exact-limb pass"
        t[i] &= M
    return t


def canon_estimate(t13, t12):
    """the float quotient estimate, before the decrement"""
    xf = np.float32(np.float32(t13) * np.float32(536870912.0)) + np.float32(t12)
    return int(np.float32(xf) * PTOP_INV)


def canon(a, stats=None, dec=True, reps=2):
    """fp_canon_call: any weakly normalised value below 8192 p -> exact limbs of the representative below p.  stats, if given, collects Q - q.
    dec / reps restate the header's `q = q ? q - 1 : 0` and its two conditional subtractions (other values: what a build without them would do)."""
    assert is_weak(a)
    x = val(a)
    assert x < FP_MAX_BOUND * P
    t = _exact_limbs_u32(a)
    q = canon_estimate(t[13], t[12])
    if dec:
        q = q - 1 if q else 0
    big_q = x // P
    if dec and reps == 2:
        assert 0 <= big_q - q <= 2, "the quotient estimate is outside {Q-2, Q-1, Q}"
    if stats is not None:
        stats[big_q - q] = stats.get(big_q - q, 0) + 1
    cy = 0
    for i in range(L):
        cur = t[i] - q * MOD[i] + cy
        assert -(1 << 63) <= cur < 1 << 63
        t[i] = cur & M if i < L - 1 else cur & U32
        cy = cur >> W
    if dec and reps == 2:
        assert t[L - 1] < 1 << 31 and val(t) == x - q * P and val(t) < 3 * P, "the remainder is not below 3 p with a non-negative top limb"
    for _ in range(reps):
        u, bw = [], 0
        for i in range(L):
            ti = t[i] - (1 << 32) if (i == L - 1 and t[i] >> 31) else t[i]          # (int32_t)t[i]
            d = ti - MOD[i] - bw
            assert -(1 << 31) <= d < 1 << 31
            bw = 1 if d < 0 else 0
            u.append(d & M if i < L - 1 else d & U32)
        if not bw:
            t = u
    if dec and reps == 2:
        assert val(t) == x % P and all(v <= M for v in t)
    return t


def is_zero_mod_p_inline(a):
    """fp_is_zero_mod_p_inline"""
    assert is_weak(a)
    t = _exact_limbs_u32(a)
    k = (t[0] * PINV) & M
    cy, o = 0, 0
    for i in range(L):
        cur = t[i] - k * MOD[i] + cy
        assert -(1 << 63) <= cur < 1 << 63
        o |= cur & M if i < L - 1 else cur & U32
        cy = cur >> W
    r = o == 0 and cy == 0
    assert r == (val(a) == k * P)
    return r


def is_zero(a, b, form):
    """fe_is_zero<b>; form 'call' (fp_canon) or 'inline' (fp_is_zero_mod_p_inline).  Returns (verdict, path): path 'zero' | 'b1' | 'fast' | 'slow'"""
    assert is_weak(a) and val(a) < b * P
    if not any(a):
        return True, "zero"
    if b == 1:
        return False, "b1"
    k = (a[0] * PINV) & U32 & M
    if k >= b:
        return False, "fast"
    r = is_zero_mod_p_inline(a) if form == "inline" else not any(canon(a))
    return r, "slow"


# ---------------------------------------------------------------- the dense memory format
def pack(a):
    """fp_pack: exact limbs, value < p -> 12 words"""
    assert all(0 <= x <= M for x in a) and val(a) < P
    r = []
    for j in range(12):
        bit = 32 * j
        k, s = bit // W, bit % W
        x = a[k] >> s
        x |= a[k + 1] << (W - s)
        if 2 * W - s < 32 and k + 2 < L:
            x |= a[k + 2] << (2 * W - s)
        r.append(x & U32)
    return r


def unpack_words(w):
    """fp_unpack: 12 words -> 14 limbs, every limb masked to 29 bits"""
    r = []
    for i in range(L):
        bit = W * i
        k, s = bit // 32, bit % 32
        x = w[k] >> s
        if k + 1 < 12:
            x |= w[k + 1] << (32 - s)
        r.append(x & M)
    return r


def words12(v):
    return [(v >> (32 * j)) & U32 for j in range(12)]


# ---------------------------------------------------------------- the lockstep inversion
FP_INV_ITERS = 27
EXACT_ELL = 6


def _i32(x):
    assert -(1 << 31) <= x < 1 << 31, "a signed value leaves int32"
    return x


def _i64(x):
    assert -(1 << 62) <= x < 1 << 62, "an accumulator leaves 63 bits"
    return x


def inv29(x, iters=FP_INV_ITERS, exact_ell=EXACT_ELL, info=None, strict=True):
    """fp_inv29_call: exact limbs of a canonical X < p -> weakly normalised limbs of X^-1 mod p, value in (4p, 60p); 0 -> 0.
    info, if given, receives zero_at (the iteration count after which a first was 0; None if never), max_uv (largest |u|, |v| seen, as an integer) and
    max_fg.  strict = False drops the assertions on the END state (a = 0, b = 1, the value) for runs with other iteration counts."""
    assert all(0 <= v <= M for v in x) and val(x) < P
    big_x = val(x)
    a, b = list(x), list(MOD)
    u, v = [1] + [0] * (L - 1), [0] * L
    any_ = any(x)
    zero_at, max_uv, max_fg = None, 0, 0
    for it in range(iters):
        # 1: approximations
        j = max([i for i in range(3, L) if a[i] | b[i]] + [2])
        small = j == 2
        ha, ma, la, hb, mb, lb = a[j], a[j - 1], a[j - 2], b[j], b[j - 1], b[j - 2]
        top = ha | hb
        ell = top.bit_length()
        exact = small and ell <= exact_ell
        ta = (ha << 35) | (ma << 6) | (la >> 23)
        tb = (hb << 35) | (mb << 6) | (lb >> 23)
        assert ta < 1 << 64 and tb < 1 << 64
        if exact:
            xa = (a[0] | (a[1] << 29) | (a[2] << 58)) & ((1 << 64) - 1)
            xb = (b[0] | (b[1] << 29) | (b[2] << 58)) & ((1 << 64) - 1)
            if exact_ell == EXACT_ELL:
                assert xa == val(a) and xb == val(b), "`exact` was chosen for values that do not fit 64 bits"
        else:
            xa = (((ta >> ell) << 29) | a[0]) & ((1 << 64) - 1)
            xb = (((tb >> ell) << 29) | b[0]) & ((1 << 64) - 1)
            assert (ta >> ell) < 1 << 35 and (tb >> ell) < 1 << 35
        # 2: 29 binary-GCD steps
        f0, g0, f1, g1 = 1, 0, 0, 1
        for _ in range(W):
            odd = xa & 1
            sw = odd and xa < xb
            na, nb = (xb, xa) if sw else (xa, xb)
            nf0, ng0, nf1, ng1 = (f1, g1, f0, g0) if sw else (f0, g0, f1, g1)
            xa = ((na - (nb if odd else 0)) & ((1 << 64) - 1)) >> 1
            xb = nb
            f0 = _i32(nf0 - (nf1 if odd else 0))
            g0 = _i32(ng0 - (ng1 if odd else 0))
            f1 = _i32(nf1 << 1)
            g1 = _i32(ng1 << 1)
            assert abs(f0) + abs(g0) <= 1 << W and abs(f1) + abs(g1) <= 1 << W, "|f| + |g| exceeds 2^29"
        max_fg = max(max_fg, abs(f0) + abs(g0), abs(f1) + abs(g1))
        # 3a: (a, b) <- (f0 a + g0 b, f1 a + g1 b) / 2^29, made non-negative
        va, vb = val(a), val(b)
        assert all(l < 1 << 31 for l in a + b)

        def lin(f, g):
            c, r = 0, [0] * L
            for i in range(L):
                c = _i64(c + f * a[i] + g * b[i])
                if i == 0:
                    assert c & M == 0, "the division by 2^29 is not exact"
                else:
                    r[i - 1] = c & M
                c >>= W
            r[L - 1] = c & U32
            s = U32 if c < 0 else 0
            cy = s & 1
            o = []
            for i in range(L - 1):
                t = (r[i] ^ (s & M)) + cy
                o.append(t & M)
                cy = t >> W
            o.append(((r[L - 1] ^ s) + cy) & U32)
            want = abs(f * va + g * vb) >> W
            assert val(o) == want, "a or b is not |f a + g b| / 2^29 after the sign fix-up"
            return o, (-f if s else f), (-g if s else g)
        na_, f0, g0 = lin(f0, g0)
        nb_, f1, g1 = lin(f1, g1)
        a, b = na_, nb_
        _i32(f0), _i32(g0), _i32(f1), _i32(g1)
        # 3b: (u, v) <- (f u + g v + q p) / 2^29, signed limbs
        vu, vv = val(u), val(v)

        def mont(f, g):
            lo = (f * u[0] + g * v[0]) & U32
            q = (lo * NINV) & U32 & M
            c, r = 0, [0] * L
            for i in range(L):
                c = _i64(c + f * u[i] + g * v[i] + q * MOD[i])
                if i == 0:
                    assert c & M == 0
                else:
                    r[i - 1] = c & M
                c >>= W
            r[L - 1] = _i32(c)
            assert val(r) << W == f * vu + g * vv + q * P
            return r
        u, v = mont(f0, g0), mont(f1, g1)
        assert all(_i32(l) == l for l in u + v)
        max_uv = max(max_uv, abs(val(u)), abs(val(v)))
        assert (val(u) * big_x - val(a)) % P == 0 and (val(v) * big_x - val(b)) % P == 0, "a = u X, b = v X (mod p) is broken"
        if zero_at is None and not any(a):
            zero_at = it + 1
    if info is not None:
        info.update(zero_at=zero_at, max_uv=max_uv, max_fg=max_fg, a=val(a), b=val(b), v=val(v))
    if strict and any_:
        assert val(a) == 0 and val(b) == 1, "a = 0, b = 1 does not hold after the last iteration"
        assert max_uv < 28 * P
    ki = fp_ki(32)
    t = []
    for i in range(L):
        s = (v[i] + KP[ki][i]) if any_ else 0
        if i < L - 1:
            assert 0 <= s <= U32
        t.append(s & U32)
    r = carry(t)
    if any_:
        if strict:
            assert val(r) == val(v) + 32 * P
            assert 4 * P < val(r) < 60 * P and val(r) * big_x % P == 1, "the result is not X^-1 in (4p, 60p)"
    else:
        assert r == [0] * L
    return r


def inv_fast(x):
    """what fe_inv_fast adds to fp_inv29_call on a canonical integer X: the Montgomery product by R^3, fully reduced: X^-1 * 2^812 mod p"""
    return pow(val(x), -1, P) * pow(2, 2 * RBITS, P) % P if any(x) else 0


# ---------------------------------------------------------------- the binary Euclid of ff.cuh on dense words (words_inv<P>, any odd modulus)
def words_inv(a, mod):
    """words_inv<P>: x -> x^-1 mod `mod` with no Montgomery correction, inv(0) = 0.  Returns (inverse, outer-loop count); the device's guard stops the
    loop at 4 * 32 * N iterations (1024 for Fr, 1536 for the 12 words of Fp)"""
    assert 0 <= a < mod and mod & 1
    if a == 0:
        return 0, 0
    u, v, x1, x2, loops = a, mod, 1, 0, 0

    def halve(x):
        return (x + mod if x & 1 else x) >> 1
    while u != 1 and v != 1:
        loops += 1
        while not u & 1:
            u >>= 1
            x1 = halve(x1)
        while not v & 1:
            v >>= 1
            x2 = halve(x2)
        if u >= v:
            u -= v
            x1 = (x1 - x2) % mod
        else:
            v -= u
            x2 = (x2 - x1) % mod
    r = x1 if u == 1 else x2
    assert r * a % mod == 1
    return r, loops
