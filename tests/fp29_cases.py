"""The operand classes of the base-field limb layer (tests/fp29_model.py), built so that each function's precondition holds by construction.  Shared by
tests/test_fp29_model.py (the model over the table) and tests/test_gpu_fp29.py (the same table through zk_selftest_fp29).  Every table is a dict
class name -> list, so that a test can count each class and fail on an empty one; every table is computed once per process."""
import functools
import random

import fp29_model as F

P, W, L, M, WEAK = F.P, F.W, F.L, F.M, F.WEAK
CANON_BOUND = F.FP_MAX_BOUND          # the largest value bound zk_selftest_fp29 admits: fp_canon_call's own, 8192 p
ZERO_BOUNDS = (2, F.FP_REST, 192)     # fe_is_zero<B>: the smallest, the at-rest bound, the largest any call site instantiates (DESIGN: how it was found)
SEARCH_BUDGET = 1200                  # model runs the seeded search may spend
SEARCH_ITERS = 30                     # the search runs the model this long, so that an operand that needs a 28th iteration shows
RANDOM_TAIL = 256


def max_weak(bound):
    """limbs 0..12 at 2^29 + 7 and the largest top limb that keeps the value below bound * p (None if there is none)"""
    t = (bound * P - F.val(F.all_weak(0)) - 1) >> F.TOPSHIFT
    return F.all_weak(t) if t >= 0 and F.val(F.all_weak(t)) < bound * P else None


def pending_chains(v, i):
    """v is a multiple of 2^(29 i) with a non-zero limb i: its forms with a carry pending out of limb i - 1 that was handed down from limb j <= i - 1:
    limb j = 2^29, limbs j+1 .. i-1 = 2^29 - 1, limb i one less"""
    e = F.unpack(v)
    assert not any(e[:i]) and e[i]
    out = []
    for j in range(i):
        l = list(e)
        l[j] = 1 << W
        for t in range(j + 1, i):
            l[t] = M
        l[i] -= 1
        assert F.val(l) == v and F.is_weak(l) and l != e
        out.append(l)
    return out


def no_second_weak_form(v):
    """True if the exact limbs are the only weakly normalised form of v: a carry can be left pending out of limb i only if limb i is at most 8"""
    return min(F.unpack(v)[:L - 1]) > 8


# ---------------------------------------------------------------- reduction
@functools.lru_cache(None)
def reduction_cases():
    exact, weak = [], []
    for k in range(CANON_BOUND):
        for v in ([k * P - 1] if k else []) + [k * P, k * P + 1, k * P + (P - 1)]:
            exact.append(F.unpack(v))
        # k p, k p - 1 and (k + 1) p - 1 have one weak form only (no_second_weak_form), so the forms with pending carries are those of the values
        # beside them that have them: k p rounded up to a multiple of 2^(29 i), and of that every chain of pending carries below limb i
        i = 1 + k % (L - 1)
        v = -(-(k * P + 1) >> (W * i)) << (W * i)
        if v < CANON_BOUND * P:
            ch = pending_chains(v, i)
            weak += [ch[0]] + ([ch[-1]] if len(ch) > 1 else []) + ([ch[k % len(ch)]] if len(ch) > 2 else [])
    tops = sorted(set([0, 1, 2, 12, 13, 14, 26, 27] + [13 * k + d for k in (64, 192, 1000, 4096, 8191) for d in (0, 1)] + [max_weak(CANON_BOUND)[L - 1]]))
    allweak = [F.all_weak(t) for t in tops if F.val(F.all_weak(t)) < CANON_BOUND * P]
    return {"exact": exact, "weak": weak, "all_weak": allweak}


# ---------------------------------------------------------------- zero test
@functools.lru_cache(None)
def zero_cases():
    """B -> class -> list of limb lists, every value below B p"""
    out = {}
    for b in ZERO_BOUNDS:
        rnd = random.Random(0xF290 + b)
        mult, small_k, big_k = [], [], []
        # a true multiple k p, 0 < k < 8192, has no weak form but the exact one (no_second_weak_form; tests/test_fp29_model.py checks every k), so
        # the class of multiples holds exact limbs
        for k in range(1, b):
            mult.append(F.unpack(k * P))
        for k in range(b):
            for i in range(1, L):
                for j in (1, 2, 3):
                    for v in (k * P + (j << (W * i)), k * P - (j << (W * i))):
                        if 0 < v < b * P:
                            l = F.unpack(v)
                            assert (l[0] * F.PINV) & M == k % (1 << W)
                            small_k.append(l if (i + j) & 1 else (F.weak_form(v, i) or l))
            for d in (1, -1, 2, P - 1):
                v = k * P + d
                if 0 < v < b * P and (F.unpack(v)[0] * F.PINV) & M >= b:
                    big_k.append(F.unpack(v))
        for _ in range(64):
            l = F.unpack(rnd.randrange(1, b * P))
            (big_k if (l[0] * F.PINV) & M >= b else small_k).append(l)
        mw = max_weak(b)
        ((big_k if (mw[0] * F.PINV) & M >= b else small_k).append(mw))
        out[b] = {"multiples": mult, "non_multiples_small_k": small_k, "k_at_least_B": big_k, "exact_zero": [[0] * L]}
    return out


# ---------------------------------------------------------------- additive rows
A_BOUND = F.FP_REST                        # the minuend of every row instantiation
SUB_ROWS = list(range(0, 12))              # fe_sub<64, B>: B = row_bound(row), fp_ks(B) + 64 <= 8192
NEG_ROWS = list(range(0, 13))              # fe_neg<A>, fe_neg_lazy<A>: A = row_bound(row)
SSD_ROWS = list(range(1, 12))              # fe_sub_sub_dbl<64, B, B>: B = row_bound(row - 1), fp_ks(3 B) = 2^(row + 1)


def row_bound(row):
    """the operand bound the hook instantiates for a table row: fp_ki(fp_ks(row_bound(row))) == row"""
    return 1 if row == 0 else 1 << row


def _extremes(bound, rnd):
    r = [[0] * L, F.unpack(bound * P - 1), F.unpack(rnd.randrange(bound * P))]
    mw = max_weak(bound)
    if mw is not None:
        r.append(mw)
    w = F.weak_form(bound * P - 1, 3)
    if w is not None:
        r.append(w)
    return r


@functools.lru_cache(None)
def additive_cases():
    """function -> row -> list of operand tuples"""
    rnd = random.Random(0xADD29)
    out = {"fe_sub": {}, "fe_neg": {}, "fe_neg_lazy": {}, "fe_sub_sub_dbl": {}}
    for row in SUB_ROWS:
        b = row_bound(row)
        assert F.fp_ki(F.fp_ks(b)) == row
        out["fe_sub"][row] = [(x, y) for x in _extremes(A_BOUND, rnd) for y in _extremes(b, rnd)]
    for row in NEG_ROWS:
        b = row_bound(row)
        assert F.fp_ki(F.fp_ks(b)) == row
        out["fe_neg"][row] = [(x,) for x in _extremes(b, rnd)]
        out["fe_neg_lazy"][row] = [(x,) for x in _extremes(b, rnd)]
    for row in SSD_ROWS:
        b = row_bound(row - 1)
        assert F.fp_ki(F.fp_ks(3 * b)) == row
        ex = _extremes(b, rnd)
        out["fe_sub_sub_dbl"][row] = [(x, y, z) for x in (_extremes(A_BOUND, rnd)[0], max_weak(A_BOUND), F.unpack(A_BOUND * P - 1)) for y in ex for z in ex]
    return out


@functools.lru_cache(None)
def add_cases():
    rnd = random.Random(0xADD)
    ex = _extremes(A_BOUND, rnd)
    return {"fe_add": [(x, y) for x in ex for y in ex], "fe_dbl": [(x,) for x in ex],
            "fp_carry": [([F.U32] * (L - 1) + [0],), ([F.U32] * L,), ([0] * L,), ([1 << W] * L,), ([M] * L,), (F.all_weak(5),)]
            + [([rnd.getrandbits(32) for _ in range(L)],) for _ in range(58)]}


@functools.lru_cache(None)
def pack_cases():
    rnd = random.Random(0x9AC)
    vals = [0, 1, P - 1, P - 2, P >> 1] + [1 << k for k in range(381)] + [(1 << k) - 1 for k in range(1, 381)] + [P - (1 << k) for k in range(380)]
    vals += [rnd.randrange(P) for _ in range(128)]
    return {"below_p": [v for v in vals if 0 <= v < P]}


# ---------------------------------------------------------------- inversion
def _families():
    fam = {}
    power = []
    for c in (1, 3, 5, 7):
        k = 0
        while c << k < P:
            for base in (c << k, P - (c << k)):
                power += [base - 1, base, base + 1]
            k += 1
    fam["c_2k"] = power
    half = P >> 1
    fam["small_and_ends"] = list(range(1, 200)) + [P - s for s in range(1, 200)] + [half + s for s in range(-100, 101)]
    fam["limb_boundaries"] = [1 << (W * j) for j in range(L)] + [(1 << (W * j)) - 1 for j in range(1, L)]
    fam["exact_switch"] = [1 << 58, 1 << 63, (1 << 64) - 1, 1 << 64, 1 << 87, (1 << 58) - 1, (1 << 63) + 1, (1 << 64) + 1, (1 << 87) - 1]
    rnd = random.Random(0x35B175)
    fam["shared_top_35_bits"] = [P - (1 << 300), P - (1 << 345) - 1, P - (1 << 345) + 1, P - 1 - (1 << 200)] + [P - rnd.getrandbits(rnd.randrange(30, 346)) for _ in range(60)]
    fam["zero"] = [0]
    rnd = random.Random(0x7A11)
    fam["random"] = [rnd.randrange(1, P) for _ in range(RANDOM_TAIL)]
    return {k: [x for x in dict.fromkeys(v) if 0 <= x < P] for k, v in fam.items()}


@functools.lru_cache(None)
def _run(x, iters=F.FP_INV_ITERS):
    info = {}
    limbs = F.inv29(F.unpack(x), iters=iters, info=info, strict=iters == F.FP_INV_ITERS)
    return tuple(limbs), info["zero_at"], info["max_uv"]


def _neighbours(x, rnd):
    c = [x + 1, x - 1, x ^ (1 << rnd.randrange(381)), x ^ (1 << rnd.randrange(64)), (x * 2) % P, (x * pow(2, -1, P)) % P, P - x,
         x + (1 << rnd.randrange(381)), x - (1 << rnd.randrange(381)), pow(x, -1, P) if x else 0]
    return [v for v in c if 0 < v < P]


@functools.lru_cache(None)
def inversion_search():
    """A seeded walk from the full-length operands through their neighbours, looking for the operand on which the APPROXIMATED loop reaches a = 0
    latest.  The model runs SEARCH_ITERS iterations here (no end-state assertions), so an operand that needs more than 27 would show as zero_at > 27.
    Returns (found: list of (x, zero_at), runs spent)."""
    rnd = random.Random(0x5EA2C4)
    seen = {}

    def score(x):
        if x not in seen:
            seen[x] = _run(x, SEARCH_ITERS)[1]
        return seen[x]
    fam = _families()
    front = [x for x in fam["c_2k"] + fam["limb_boundaries"] if x and _run(x)[1] == F.FP_INV_ITERS][:24]
    runs = 0
    best = []
    while runs < SEARCH_BUDGET and front:
        x = front[rnd.randrange(len(front))]
        for y in _neighbours(x, rnd):
            if y in seen or runs >= SEARCH_BUDGET:
                continue
            runs += 1
            s = score(y)
            if s is not None and s >= F.FP_INV_ITERS:
                front.append(y)
                best.append((y, s))
    return best, runs


@functools.lru_cache(None)
def inversion_cases():
    """class -> list of X.  'needs_all_27' is every operand of the families and of the search whose a first becomes 0 in the last iteration."""
    fam = _families()
    found, _ = inversion_search()
    fam["search"] = [x for x, _ in found][:128]
    full = [x for v in fam.values() for x in v if x and _run(x)[1] == F.FP_INV_ITERS]
    fam["needs_all_27"] = list(dict.fromkeys(full))
    # b = 1 (and with it the final v) can be reached long before a = 0: 2^380 has it after 14 iterations.  The operands whose result after 26
    # iterations is NOT the inverse are the ones that hold FP_INV_ITERS = 27 on the device
    fam["wrong_after_26"] = [x for x in fam["needs_all_27"] if F.val(F.inv29(F.unpack(x), iters=F.FP_INV_ITERS - 1, strict=False)) * x % P != 1]
    return fam


def inversion_expected(x):
    """(raw limbs of fp_inv29_call, zero_at) from the model, computed once per operand"""
    r = _run(x)
    return list(r[0]), r[1]


@functools.lru_cache(None)
def full_length_montgomery_residues():
    """a quick pick for the canonical-input batteries (tests/test_gpu_field.py): residues X that keep fp_inv29_call busy for all 27 iterations, those of
    them a 26-iteration build gets wrong, and the values on either side of the `exact` switch"""
    cand = [c << k for c in (1, 3, 5, 7) for k in range(366, 381) if c << k < P]
    cand += [P - x for x in cand]
    full = [x for x in cand if _run(x)[1] == F.FP_INV_ITERS]
    late = [x for x in full if F.val(F.inv29(F.unpack(x), iters=F.FP_INV_ITERS - 1, strict=False)) * x % P != 1]
    return {"needs_all_27": full, "wrong_after_26": late, "exact_switch": _families()["exact_switch"], "limb_boundaries": _families()["limb_boundaries"]}


# ---------------------------------------------------------------- words_inv<FrParams>: the operands that drive its outer loop longest
FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FR_GUARD = 4 * 32 * 8


@functools.lru_cache(None)
def fr_words_inv_operands():
    """A -> outer-loop count of words_inv on the integer A (what the device inverts is the Montgomery residue a * 2^256 mod r): 1, 2, r - 1, 2^k, r - 2^k,
    and the longest runs of a seeded walk through their neighbours"""
    rnd = random.Random(0xF2199)
    xs = [1, 2, FR - 1, FR - 2] + [1 << k for k in range(255) if 1 << k < FR] + [FR - (1 << k) for k in range(255)] + [rnd.randrange(1, FR) for _ in range(64)]
    seen = {x: F.words_inv(x, FR)[1] for x in xs if 0 < x < FR}
    front = sorted(seen, key=seen.get)[-16:]
    for _ in range(3000):
        x = front[rnd.randrange(len(front))]
        y = rnd.choice([x ^ (1 << rnd.randrange(255)), (x * 3) % FR, (x + (1 << rnd.randrange(255))) % FR, FR - x, pow(x, -1, FR), (x * pow(2, -1, FR)) % FR])
        if 0 < y < FR and y not in seen:
            seen[y] = F.words_inv(y, FR)[1]
            if seen[y] >= seen[front[0]]:
                front = sorted(front + [y], key=seen.get)[-16:]
    longest = sorted(seen, key=seen.get)[-32:]
    return {x: seen[x] for x in dict.fromkeys([1, 2, FR - 1] + [1 << k for k in range(0, 255, 7)] + [FR - (1 << k) for k in range(0, 255, 7)] + longest)}
