"""Integer model of zukelang_amd/csrc/fr29.cuh (Fr on 9 limbs of 29 bits, Montgomery R' = 2^261), importable and without side effects.

Three layers, all on Python integers:
  * the constants of fr29_consts.cuh, parsed from the header (MOD, KR, C32, QMUL);
  * the fr9_* functions restated limb for limb on lists of 9 integers.  Each asserts what the device code relies on without checking: no product
    column reaches 2^64, no limb leaves 32 bits, no limb of a subtraction borrows, the quotient estimate fits.  Where those hold the lists are what
    the device computes, limb for limb (tests/test_gpu_fr_field.py compares them with zk_selftest_fr29);
  * the same functions on worst-case intervals (Iv: value < bound * r, a maximum per limb), which is how tests/test_fr29_model.py walks the stage
    schedule of ntt_lds.cuh;
  * sampled_checks(): random and extreme operands through single steps, with a fixed seed."""
import os
import random
import re

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
W, L, M = 29, 9, (1 << 29) - 1
U32 = 0xFFFFFFFF
WEAK = (1 << W) + 7                    # a weakly normalised limb: at most this
RP = 1 << 261                          # the Montgomery radix of the 9-limb form
TOP_64R = (64 * R) >> (W * (L - 1))    # the largest top limb of an exact-limb value below 64 r
CONSTS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zukelang_amd", "csrc", "fr29_consts.cuh")


def parse_consts(path=CONSTS_PATH):
    src = open(path).read()

    def arr(name):
        body = re.search(name + r"(?:\[\d+\])+ = \{(.*?)\};", src, re.S).group(1)
        return [int(x, 16) for x in re.findall(r"0x([0-9a-f]+)u", body)]
    kr = arr("FR29_KR")
    return {"MOD": arr("FR29_MOD"), "KR": [kr[L * k:L * k + L] for k in range(len(kr) // L)], "C32": arr("FR29_C32"),
            "QMUL": int(re.search(r"FR29_QMUL = (\d+)u", src).group(1)), "NK": int(re.search(r"FR29_NK = (\d+)", src).group(1))}


_C = parse_consts()
MOD, KR, C32, QMUL, NK = _C["MOD"], _C["KR"], _C["C32"], _C["QMUL"], _C["NK"]


def val(l):
    return sum(x << (W * i) for i, x in enumerate(l))


def unpack(v):
    """exact limbs of a non-negative integer below 2^(261 + 3)"""
    return [(v >> (W * i)) & M for i in range(L - 1)] + [v >> (W * (L - 1))]


def pending(l, i):
    """the same value with a carry pending out of limb i < 8: limb i + 2^29, limb i + 1 - 1 (None where limb i + 1 is zero or limb i leaves the weak range)"""
    if l[i + 1] == 0 or l[i] + (1 << W) > WEAK:
        return None
    r = list(l)
    r[i] += 1 << W
    r[i + 1] -= 1
    return r


def words8(v):
    return [(v >> (32 * j)) & U32 for j in range(8)]


def unpack_words(w):
    """fr9_unpack: 8 words of 32 bits -> 9 limbs"""
    r = []
    for i in range(L):
        bit = W * i
        k, s = bit // 32, bit % 32
        x = w[k] >> s
        if k + 1 < 8:
            x |= w[k + 1] << (32 - s)
        r.append(x & M if i < L - 1 else x & U32)
    return r


def pack_exact(a):
    """fr9_pack_exact: exact limbs, value < 2^256 -> 8 words"""
    r = []
    for j in range(8):
        bit = 32 * j
        k, s = bit // W, bit % W
        x = a[k] >> s
        if k + 1 < L:
            x |= a[k + 1] << (W - s)
        if 2 * W - s < 32 and k + 2 < L:
            x |= a[k + 2] << (2 * W - s)
        r.append(x & U32)
    return r


def carry(t):
    assert all(0 <= x <= U32 for x in t), "a limb outside 32 bits before the carry pass"
    c = [t[i] >> W for i in range(L - 1)]
    r = [t[0] & M] + [(t[i] & M) + c[i - 1] for i in range(1, L - 1)] + [t[L - 1] + c[L - 2]]
    assert all(0 <= x <= U32 for x in r), "a limb outside 32 bits after the carry pass"
    return r


def add(a, b):
    return carry([x + y for x, y in zip(a, b)])


def sub(a, b, ki):
    assert all(k >= y for k, y in zip(KR[ki][:L - 1], b[:L - 1])), "limb borrow"
    t = [x + (k - y) for x, y, k in zip(a, b, KR[ki])]
    assert all(0 <= x <= U32 for x in t[:L - 1]), "a limb outside 32 bits before the carry pass"
    c = [t[i] >> W for i in range(L - 1)]
    # the top limb may wrap below zero before the carry pass (32-bit arithmetic); it is exact after it because the value is >= r
    r = [t[0] & M] + [(t[i] & M) + c[i - 1] for i in range(1, L - 1)] + [(t[L - 1] + c[L - 2]) & U32]
    assert val(r) == val(a) + (R << ki) - val(b), "the top limb did not come back"
    return r


def sub_raw(a, b, ki):
    r = [x + (k - y) for x, y, k in zip(a, b, KR[ki])]
    assert all(0 <= x <= U32 for x in r), "sub_raw: a limb borrows or leaves 32 bits"
    return r


def mul(a, b):
    acc, m, r = 0, [], [0] * L
    for k in range(L):
        acc += sum(a[i] * b[k - i] for i in range(k + 1)) + sum(m[i] * MOD[k - i] for i in range(k))
        assert acc < 1 << 64, "product column overflow"
        m.append((-acc) & M)
        acc += m[k]
        assert acc < 1 << 64 and acc & M == 0
        acc >>= W
    for k in range(L, 2 * L - 1):
        acc += sum(a[i] * b[k - i] for i in range(k - L + 1, L)) + sum(m[i] * MOD[k - i] for i in range(k - L + 1, L))
        assert acc < 1 << 64, "product column overflow"
        r[k - L] = acc & M
        acc >>= W
    assert acc <= U32
    r[L - 1] = acc
    return r


def reduce_weak_q(a):
    """fr9_reduce_weak and the quotient it estimated"""
    t = list(a)
    for i in range(L - 1):
        t[i + 1] += t[i] >> W
        t[i] &= M
        assert t[i + 1] <= U32
    assert t[L - 1] * QMUL < 1 << 64
    q = (t[L - 1] * QMUL) >> 50
    r, cy = [], 0
    for i in range(L):
        cur = t[i] - q * MOD[i] + cy
        assert -(1 << 63) <= cur < 1 << 63
        r.append(cur & M if i < L - 1 else cur)
        cy = cur >> W
    assert 0 <= r[L - 1] <= U32 and val(r) == val(a) - q * R, "the quotient estimate exceeds the quotient"
    return r, q


def reduce_weak(a):
    return reduce_weak_q(a)[0]


def canon_limbs(a):
    """the limbs fr9_canon_pack hands to fr9_pack_exact, and whether the conditional subtraction was taken"""
    t = reduce_weak(a)
    u, bw = [], 0
    for i in range(L):
        d = t[i] - MOD[i] - bw
        assert -(1 << 31) <= d < 1 << 31
        bw = 1 if d < 0 else 0
        u.append(d & M if i < L - 1 else d & U32)
    return (t, False) if bw else (u, True)


def canon_pack(a):
    return pack_exact(canon_limbs(a)[0])


def canon(a):
    """the value fr9_canon_pack stores (its words: canon_pack)"""
    return val(canon_limbs(a)[0])


# ---------------------------------------------------------------------------------------------- worst-case intervals
class Iv:
    """every value v with v < bound * r whose limb i is at most limbs[i] (limbs 0..7; the top limb holds the rest)"""

    def __init__(self, bound, limbs, exact=False):
        self.bound, self.limbs, self.exact = bound, list(limbs), exact

    def top(self):
        return (self.bound * R - 1) >> (W * (L - 1))          # the lower limbs are non-negative: the top limb never exceeds value >> 232

    def all_limbs(self):
        return self.limbs + [self.top()]

    def __repr__(self):
        return "Iv(< %d r, limbs <= %s)" % (self.bound, [hex(x) for x in self.limbs])


def iv_exact(bound):
    return Iv(bound, [M] * (L - 1), True)


def iv_weak(bound):
    return Iv(bound, [WEAK] * (L - 1))


def iv_join(a, b):
    return Iv(max(a.bound, b.bound), [max(x, y) for x, y in zip(a.limbs, b.limbs)], a.exact and b.exact)


def _iv_carried(bound, pre):
    assert all(x <= U32 for x in pre), "a limb outside 32 bits before the carry pass"
    out = [M] + [M + (pre[i - 1] >> W) for i in range(1, L - 1)]
    assert all(x <= WEAK for x in out), "the carry pass does not leave weakly normalised limbs"
    return Iv(bound, out)


def iv_add(a, b):
    return _iv_carried(a.bound + b.bound, [x + y for x, y in zip(a.all_limbs(), b.all_limbs())])


def _iv_sub_pre(a, b, ki):
    assert 0 <= ki < NK, "no such multiple of r"
    assert (1 << ki) >= b.bound + 1, "2^KI below the subtrahend's bound + 1"
    assert all(k >= y for k, y in zip(KR[ki][:L - 1], b.limbs)), "limb borrow"
    return [x + k for x, k in zip(a.all_limbs(), KR[ki])]          # the subtrahend's limbs at zero


def iv_sub(a, b, ki):
    return _iv_carried(a.bound + (1 << ki), _iv_sub_pre(a, b, ki))


def iv_sub_raw(a, b, ki):
    pre = _iv_sub_pre(a, b, ki)
    assert KR[ki][L - 1] >= b.top(), "sub_raw: the top limb would wrap and no carry pass follows"
    assert all(x <= U32 for x in pre), "a limb outside 32 bits"
    r = Iv(a.bound + (1 << ki), pre[:L - 1])
    r.raw_top = pre[L - 1]
    return r


def iv_mul(a, b):
    """returns the result interval; peak column value in iv_mul.peak"""
    assert a.bound * b.bound <= 64, "operand bounds exceed the Montgomery headroom: %d * %d" % (a.bound, b.bound)
    la = a.limbs + [getattr(a, "raw_top", a.top())]
    lb = b.limbs + [getattr(b, "raw_top", b.top())]
    acc, peak = 0, 0
    for k in range(2 * L - 1):
        lo, hi = max(0, k - L + 1), min(k, L - 1)
        acc += sum(la[i] * lb[k - i] for i in range(lo, hi + 1))
        acc += sum(M * MOD[k - i] for i in range(lo, hi + 1) if k - i > 0 or k >= L)          # m_i <= 2^29 - 1; m_k * r_0 = m_k is the next line
        if k < L:
            acc += M
        assert acc < 1 << 64, "product column %d reaches 2^64 at the interval maxima" % k
        peak = max(peak, acc)
        acc >>= W
    assert acc <= U32
    iv_mul.peak = peak
    return iv_exact(2)


def iv_reduce_weak(a):
    assert a.bound <= 64, "reduce_weak above 64 r"
    t = a.all_limbs()
    for i in range(L - 1):
        t[i + 1] += t[i] >> W
        assert t[i + 1] <= U32, "a limb outside 32 bits"
    assert a.top() * QMUL < 1 << 64 and ((a.top() * QMUL) >> 50) * max(MOD) < 1 << 62
    return iv_exact(2)


def iv_canon_store(a):
    iv_reduce_weak(a)          # fr9_canon_pack = reduce_weak, one conditional subtraction, pack


# ---------------------------------------------------------------------------------------------- sampled single steps
def lazy(rnd, bound):
    """a lazily reduced representative below bound * r: random, or at the top of the bound"""
    v = rnd.randrange(bound * R) if rnd.random() < 0.8 else bound * R - 1 - rnd.randrange(1 << rnd.randrange(1, 200))
    return unpack(v)


def sampled_checks(seed=1, products=20000, butterflies=3000):
    rnd = random.Random(seed)
    for it in range(products):
        A = rnd.choice([1, 2, 3, 8, 16, 48, 56, 64])
        a, b = lazy(rnd, A), lazy(rnd, 64 // A)
        p = mul(a, b)
        assert val(p) < 2 * R and (val(p) * RP - val(a) * val(b)) % R == 0
        x = lazy(rnd, rnd.choice([1, 2, 24, 42, 63, 64]))
        assert canon(x) == val(x) % R
        k = rnd.randrange(1, 64)          # extreme tops for the quotient estimate
        for d in (-1, 0, 1):
            v = k * R + d * rnd.randrange(1, 1 << rnd.randrange(1, 240))
            if 0 <= v < 64 * R:
                assert canon(unpack(v)) == v % R
    for it in range(butterflies):
        # DIF stage chain: bounds 3 -> 6 -> 12 -> 24 -> (reduce) 2
        u, v, w = lazy(rnd, 24), lazy(rnd, 24), lazy(rnd, 1)
        x = add(u, v)
        y = mul(sub(u, v, 5), w)
        assert mul(sub_raw(u, v, 5), w) == y          # no carry pass before a product by a factor with exact limbs
        assert val(x) < 48 * R and val(reduce_weak(x)) < 2 * R and val(y) < 2 * R
        assert (val(y) * RP - (val(u) - val(v)) * val(w)) % R == 0
        # DIT: u below 38 r, v below 42 r
        u, v = lazy(rnd, 38), lazy(rnd, 42)
        t = mul(v, w)
        x = add(u, t)
        y = sub(u, t, 2)
        assert val(x) < 40 * R and val(y) < 42 * R and (val(y) - val(u) + val(t)) % R == 0
    return products, butterflies
