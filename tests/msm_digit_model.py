"""The signed-digit recoding of a Pippenger product as plain integers (csrc/msm.cuh: msm_fold, msm_windows; csrc/msm_digits.cuh: digit_constant,
digits_prepare, digit_at; csrc/msm_tail.cuh: digit_plan), and the scalars that sit at its ends.

A scalar s < r becomes nw digits d_j in [-(2^(c-1) - 1), 2^(c-1)]: d_j = ((s' + K) >> cj & mask) - bias with bias = 2^(c-1) - 1, K = sum_j bias 2^(cj) and
s' = s -- or, where the digits fold (one bucket set, checked points, c | 255), s' = min(s, r - s) with every sign turned round when r - s < s.  Digit d
goes to bucket |d| - 1; bucket k has weight w = k + 1 = hi 2^lb + lo, and the top bucket (digit +2^(c-1), weight nbw) is the only member of the last
high-digit value nd1 - 1.

families(c, fold) names the scalars that reach the ends of that plan: the top and the bottom digit in every window, carries out of a bottom digit, a
lone digit in the last window, the neighbours of r / 2 where the fold decides, and pairs s, r - s.  check_coverage() says what a family list must
contain; the CPU test holds it for every width and form, every GPU case asserts it before it runs a product (tests/test_msm_digit_model.py,
tests/test_gpu_msm_digit_ends.py), so a change of the plan fails there instead of hollowing the cases out."""
from collections import namedtuple

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
HALF = (R - 1) // 2                  # r is odd: r - s < s exactly when s > (r - 1) / 2
WIDTHS = range(2, 23)                # msm_points.hip: bases_setup refuses anything else
SHORT_C = 5                          # msm_resident.hip: the narrow table of the short products


# ---- csrc/msm_tail.cuh: digit_plan
def digit_plan(c):
    nbw = 1 << (c - 1)
    lb = (c + 1) // 2
    return dict(nbw=nbw, lb=lb, nd0=1 << lb, nd1=(nbw >> lb) + 1)


# ---- csrc/msm.cuh
def msm_fold(c, precomp, in_subgroup):
    return bool(precomp and in_subgroup and 255 % c == 0)


def msm_windows(c, fold=False):
    return 255 // c if fold and 255 % c == 0 else 255 // c + 1


def forms(c):
    """the forms a width can take: 0 plain, 1 folded"""
    return (0, 1) if 255 % c == 0 else (0,)


# ---- csrc/msm_digits.cuh
def bias(c):
    return (1 << (c - 1)) - 1


def digit_constant(c, nw):
    return sum(bias(c) << (c * j) for j in range(nw))


def flips(s, fold):
    """digits_prepare: t = r - s, the digits are taken from t when t < s"""
    return bool(fold) and s > HALF


def digits_prepare(s, c, fold):
    """(s' + K, flipped) of a non-zero scalar; the device keeps `flipped` in bit 31 of the ninth word"""
    flipped = flips(s, fold)
    return (R - s if flipped else s) + digit_constant(c, msm_windows(c, fold)), flipped


def digit_at(x, j, c):
    """window j of a prepared scalar: the digit before the fold's sign is applied"""
    return ((x >> (c * j)) & ((1 << c) - 1)) - bias(c)


Recoded = namedtuple("Recoded", "raw digits flipped keys_precomp keys_classic")


def recode(s, c, fold=0):
    """raw: the digits of s' = min(s, r - s) (of s itself in the plain form); digits: as they are filed, the fold's sign applied; keys_*: (global bucket,
    negative, window) of every non-zero digit in the one bucket set of a window table and in the nw sets of the classic layout"""
    nw, nbw = msm_windows(c, fold), 1 << (c - 1)
    if s == 0:
        return Recoded([0] * nw, [0] * nw, False, [], [])
    x, flipped = digits_prepare(s, c, fold)
    raw = [digit_at(x, j, c) for j in range(nw)]
    digits = [-d if flipped else d for d in raw]
    kp = [(abs(d) - 1, d < 0, j) for j, d in enumerate(digits) if d]
    kc = [(j * nbw + abs(d) - 1, d < 0, j) for j, d in enumerate(digits) if d]
    return Recoded(raw, digits, flipped, kp, kc)


def bucket_keys(scalars, c, precomp, identity, fold=0):
    """the global bucket of every non-zero digit of every scalar whose base is not the identity, as the sort files them"""
    keys = []
    for s, ident in zip(scalars, identity):
        if s == 0 or ident:
            continue
        rc = recode(s, c, fold)
        keys += [k for k, _, _ in (rc.keys_precomp if precomp else rc.keys_classic)]
    return keys


def bound(fold):
    """the largest value whose digits are ever taken"""
    return HALF if fold else R - 1


def largest_sum(c, fold):
    """every digit at its top value"""
    return sum((1 << (c - 1)) << (c * j) for j in range(msm_windows(c, fold)))


# ---- the scalars at the ends of the plan
def all_top(c, fold):
    """(J, sum_{j<J} 2^(c-1) 2^(cj)) with the largest J that stays within the bound"""
    top, s, J = 1 << (c - 1), 0, 0
    while J < msm_windows(c, fold) and s + (top << (c * J)) <= bound(fold):
        s += top << (c * J)
        J += 1
    return J, s


def all_bottom(c, fold):
    """(J, 2^(cJ) - sum_{j<J} (2^(c-1) - 1) 2^(cj)) with the largest J that fits: window J exists and the value stays within the bound"""
    best = None
    for J in range(1, msm_windows(c, fold)):
        s = (1 << (c * J)) - sum(bias(c) << (c * j) for j in range(J))
        if s <= bound(fold):
            best = (J, s)
    return best


def top_in_last(c, fold):
    """the smallest value with the top digit in the LAST window (every window below at the bottom digit), or None where no canonical scalar has one"""
    nw = msm_windows(c, fold)
    s = ((1 << (c - 1)) << (c * (nw - 1))) - sum(bias(c) << (c * j) for j in range(nw - 1))
    return s if 1 <= s <= bound(fold) else None


FIXED = (("r-1", R - 1), ("r-2", R - 2), ("(r-1)/2", (R - 1) // 2), ("(r+1)/2", (R + 1) // 2), ("(r-3)/2", (R - 3) // 2), ("(r+3)/2", (R + 3) // 2),
         ("2^254", 1 << 254), ("2^254-1", (1 << 254) - 1), ("1", 1), ("2", 2))
MIRRORED = ("all top", "all bottom", "(r-3)/2")


def families(c, fold=0):
    """[(name, scalar)], every scalar canonical and none zero"""
    nw, top = msm_windows(c, fold), 1 << (c - 1)
    out = [("all top", all_top(c, fold)[1]), ("all bottom", all_bottom(c, fold)[1])]
    out += [("top@%d" % j, top << (c * j)) for j in range(nw) if top << (c * j) <= bound(fold)]
    if top_in_last(c, fold) is not None and top << (c * (nw - 1)) > bound(fold):
        out.append(("top@%d,least" % (nw - 1), top_in_last(c, fold)))
    out += [("carry@%d" % j, (top + 1) << (c * j)) for j in range(nw - 1) if (top + 1) << (c * j) <= bound(fold)]
    out += list(FIXED)
    if fold:
        named = dict(out)
        for name in MIRRORED:
            out += [("mirror+ %s" % name, named[name]), ("mirror- %s" % name, R - named[name])]
    assert all(0 < s < R for _, s in out)
    return out


def mirror_pairs(c):
    """[(name, s, r - s)] of the folded families"""
    named = dict(families(c, 1))
    return [(name, named["mirror+ %s" % name], named["mirror- %s" % name]) for name in MIRRORED]


def coverage(c, fold, scalars):
    """what a scalar list reaches, by the digits of s' (bucket and sign before the fold turns it): the windows holding the top digit +2^(c-1) and the
    bottom digit -(2^(c-1) - 1), the scalars with a non-zero digit in the last window, the flipped and the unflipped ones"""
    nw, top = msm_windows(c, fold), 1 << (c - 1)
    tops, bottoms, last, flipped, plain = set(), set(), 0, 0, 0
    for s in scalars:
        rc = recode(s, c, fold)
        tops |= {j for j, d in enumerate(rc.raw) if d == top}
        bottoms |= {j for j, d in enumerate(rc.raw) if d == -bias(c) and d != 0}
        last += rc.raw[nw - 1] != 0
        flipped += rc.flipped
        plain += not rc.flipped
    return dict(tops=tops, bottoms=bottoms, last=last, flipped=flipped, plain=plain)


def check_coverage(c, fold, scalars):
    """the ends a family list must reach (the scalars on bases that are not the identity); returns coverage()"""
    nw, p = msm_windows(c, fold), digit_plan(c)
    # the plan has a place for the top bucket: weight nbw is the lone member of the last high-digit value, and no low digit is lost
    assert p["nbw"] >> p["lb"] == p["nd1"] - 1 and p["nbw"] & (p["nd0"] - 1) == 0 and (p["nd1"] - 1) << p["lb"] == p["nbw"], p
    got = coverage(c, fold, scalars)
    want_tops = set(range(nw - 1)) | ({nw - 1} if top_in_last(c, fold) is not None else set())
    assert got["tops"] == want_tops, (c, fold, "top digit", sorted(want_tops - got["tops"]))
    # a bottom digit in the last window would make s' negative; at c = 2 it is -1, as small a digit as there is, and still has a window to carry into
    assert got["bottoms"] == set(range(nw - 1)), (c, fold, "bottom digit", sorted(set(range(nw - 1)) - got["bottoms"]))
    assert got["last"] >= 4, (c, fold, "last window", got["last"])
    if fold:
        assert got["flipped"] >= 1 and got["plain"] >= 1, (c, fold, got)
        assert not flips(HALF, fold) and flips(HALF + 1, fold) and HALF in scalars and HALF + 1 in scalars
    else:
        assert got["flipped"] == 0
    return got
