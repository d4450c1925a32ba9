"""Equal and opposite sums meeting INSIDE the bucket reduction, in every kernel form that owns one of its steps (zk_msm_g1 / zk_msm_g2 against the
oracle's naive fold, classic and through the resident-key machinery).

With honest keys no two bucket sums are ever equal or opposite, so the P + P, P + (-P) and identity branches of the fix-up, the digit sums and the
trees never run in tests/test_gpu_options.py; the duplicated bases of tests/test_gpu_msm.py reach them at narrow windows and in the default forms only.
Here P3 = P1 + P2 (or its negative) sits in one bucket as a copied base while another bucket ACCUMULATES P1 + P2 -- the same group element with
ZZ != 1 and other limbs -- and the two buckets are placed, from a restatement of the digit plan, on one lane of a digit value's sum or on the two lanes
that meet in its tree; runs of one point cut by chunk borders do the same to the fix-up.  The restated plan is held to csrc/msm_tail.cuh by text, and
every case asserts from it that its points land where it needs them: a change of the plan fails here instead of hollowing the cases out."""
import os
import random
import re
from collections import Counter

import pytest

import oracle_lib as O
from msm_digit_model import bucket_keys, digit_plan, msm_windows as windows
from oracle import pyref as P
from test_gpu_options import options
from zukelang_amd.curve import G1, G2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16                       # msm.hip: chunk_min (ZK_MSM_CHUNK_MIN unset), what a small product gets
FIXUP_SERIAL_MAX = 16            # msm_tail.cuh
DW_POINTS = 256
GROUP_SIZES = (16, 32, 64)       # points per digit value: narrow G1 / narrow G2 and ZK_DS_WIDE_GROUP / wide

SETTINGS = [
    {},
    {"ZK_TAIL_SLOTS": 0}, {"ZK_TAIL_SLOTS": 1},
    {"ZK_TAIL_FIXUP_SLOTS": 1},
    {"ZK_FIXUP_BY_CHUNK": 0}, {"ZK_FIXUP_BY_CHUNK": 1},
    {"ZK_DS_WIDE_GROUP": 16, "ZK_TAIL_SLOTS": 0}, {"ZK_DS_WIDE_GROUP": 32, "ZK_TAIL_SLOTS": 0}, {"ZK_DS_WIDE_GROUP": 64, "ZK_TAIL_SLOTS": 0},
    {"ZK_RED_WAVES": 1, "ZK_TAIL_SLOTS": 0}, {"ZK_RED_WAVES": 2, "ZK_TAIL_SLOTS": 0},
    {"ZK_ACC_G1_GLDS": 0},
    {"ZK_ACC_G1_MMADD": 1},
    {"ZK_ACC_G2_INLINE": 0}, {"ZK_ACC_G2_INLINE": 1},
]


# ---- the plan, restated (csrc/msm_tail.cuh: digit_plan; csrc/msm_digits.cuh: the recoding, shared with tests/test_gpu_msm_digit_ends.py in
# tests/msm_digit_model.py and held to the sources there and below; csrc/msm.hip: the chunks)
def runs(scalars, c, precomp, identity):
    """{bucket: (first sorted position, entries)} of a product"""
    counts = Counter(bucket_keys(scalars, c, precomp, identity))
    out, pos = {}, 0
    for k in sorted(counts):
        out[k] = (pos, counts[k])
        pos += counts[k]
    return out


def borders(run):
    """chunk borders a run crosses: t1 - t0 of the fix-up kernels"""
    s, n = run
    return (s + n - 1) // CHUNK - s // CHUNK


def test_the_restated_plan_is_the_librarys():
    tail = open(os.path.join(ROOT, "zukelang_amd", "csrc", "msm_tail.cuh")).read()
    for line in ("p.nbw = 1u << (c - 1);", "p.lb = (c + 1) / 2;", "p.nd0 = 1u << p.lb;", "p.nd1 = (p.nbw >> p.lb) + 1;",
                 "FIXUP_SERIAL_MAX = %d;" % FIXUP_SERIAL_MAX, "DW_POINTS = %d;" % DW_POINTS):
        assert line in tail, line
    msm = open(os.path.join(ROOT, "zukelang_amd", "csrc", "msm.hip")).read()
    assert "chunk_min = (uint32_t)opt_int(OPT_MSM_CHUNK_MIN, %d);" % CHUNK in msm and "ZK_MSM_CHUNK_MIN" not in os.environ
    assert "const bool wide = dp.nd0 > DW_POINTS;" in msm
    red = open(os.path.join(ROOT, "zukelang_amd", "csrc", "msm_red.hip")).read()
    tl = open(os.path.join(ROOT, "zukelang_amd", "csrc", "msm_tail.hip")).read()
    for text in (red, tl):          # a lane's serial part strides the other digit by the group size; bucket w holds scalar w
        assert "const uint32_t w = low ? (e << p.lb) + d : (d << p.lb) + e;" in text
    assert "for (uint32_t e = lane; e < cnt; e += DS_GROUP)" in red and "for (uint32_t e = lane; e < cnt; e += DS)" in tl
    assert digit_plan(16) == dict(nbw=32768, lb=8, nd0=256, nd1=129) and digit_plan(17) == dict(nbw=65536, lb=9, nd0=512, nd1=129)
    assert digit_plan(16)["nd0"] <= DW_POINTS < digit_plan(17)["nd0"]          # c = 16: the narrow digit sums, c = 17: the wide ones


# ---- the points
class Curve:
    def __init__(self, G, naive, mul, add, gen, seed):
        self.G, self.naive, self.mul, self.add = G, naive, mul, add
        rng = random.Random(seed)
        k = lambda: P.fr_to_bytes(rng.randrange(1, P.R))
        self.neg = lambda p: mul(p, P.fr_to_bytes(P.R - 1))
        self.inf = bytes([0x40]) + bytes(G.POINT_BYTES - 1)
        self.p1, self.p2, self.p = mul(gen(), k()), mul(gen(), k()), mul(gen(), k())
        self.p3 = add(self.p1, self.p2)
        self.m3 = self.neg(self.p3)
        self.randoms = [mul(gen(), k()) for _ in range(12)]
        self.random_scalars = [rng.randrange(1, 1 << 253) for _ in range(12)]          # below 2^254: no carry into a top window that holds nothing else (digit 1 = bucket 0 of a resident set at c = 17)
        assert len({self.p1, self.p2, self.p3, self.m3, self.p}) == 5 and self.add(self.p3, self.m3) == self.inf


_curves = {}


def curve(group):
    if group not in _curves:
        _curves[group] = (Curve(G2, O.g2_msm_naive, O.g2_mul, O.g2_add, O.g2_generator, 0xC011) if group
                          else Curve(G1, O.g1_msm_naive, O.g1_mul, O.g1_add, O.g1_generator, 0xC010))
    return _curves[group]


# ---- the cases: (bases, scalars) and what the model must say about them
def digit_sum_cases(cv, c):
    """{name: (bases, scalars)}: two buckets holding the same (or opposite) group element in different representations, on one lane of a digit value's
    sum (serial part) or on the two lanes that meet last in its tree, for the low digit and, mirrored, for the high digit"""
    p = digit_plan(c)
    lb = p["lb"]
    d, h = 5, 3
    spots = {"low, serial": (d, d + (64 << lb)), "low, tree": (d, d + (1 << lb)), "high, serial": ((h << lb) + 1, (h << lb) + 65), "high, tree": (h << lb, (h << lb) + 1)}
    out = {}
    for name, (s1, s2) in spots.items():
        assert 1 <= s1 < s2 <= p["nbw"]
        lo, hi = (s1 & (p["nd0"] - 1), s2 & (p["nd0"] - 1)), (s1 >> lb, s2 >> lb)
        same, other = (lo, hi) if name.startswith("low") else (hi, lo)
        assert same[0] == same[1] != 0 and other[1] < (p["nd1"] if name.startswith("low") else p["nd0"])          # one digit value, weight not 0
        if name.endswith("serial"):
            assert all((other[1] - other[0]) % g == 0 for g in GROUP_SIZES) and other[0] != other[1]              # one lane, whatever the group size
        else:
            assert other[0] % 2 == 0 and other[1] == other[0] + 1 and other[1] < min(GROUP_SIZES)                  # lanes 2k, 2k + 1: the tree's last level
        for kind, third in (("doubling", cv.p3), ("cancelling", cv.m3)):
            scalars = [s1, s1, s2]
            for precomp in (False, True):
                r = runs(scalars, c, precomp, [False] * 3)
                assert r == {s1 - 1: (0, 2), s2 - 1: (2, 1)}                                                      # window 0 only: P1, P2 accumulate, P3 is copied
            out["%s, %s" % (name, kind)] = (cv.p1 + cv.p2 + third, scalars)
    return out


def fixup_cases(cv, c):
    """{name: (bases, scalars)}: one bucket whose run the chunk borders cut into equal, or opposite, partial sums"""
    out = {}
    for name, copies, neg, serial in (("32 P", 32, 0, True), ("48 P", 48, 0, True), ("16 P, 16 -P", 16, 16, True), ("320 P", 320, 0, False),
                                      ("160 P, 160 -P", 160, 160, False)):
        n = copies + neg
        for precomp in (False, True):
            r = runs([1] * n, c, precomp, [False] * n)
            assert r == {0: (0, n)} and n * windows(c) < CHUNK * 32768                    # few chunks: the fix-up goes by chunk border unless told otherwise
            assert (borders(r[0]) <= FIXUP_SERIAL_MAX) == serial and borders(r[0]) == n // CHUNK - 1 >= 1
        out[name] = (cv.p * copies + cv.neg(cv.p) * neg, [1] * n)
    return out


def mixed_case(cv, c):
    """one product holding all of the above under distinct digit values, random points and identity bases: the neighbours of a special case are ordinary"""
    bases, scalars, ident, want = [], [], [], {}
    p = digit_plan(c)
    lb = p["lb"]
    shift = 0
    for i, (name, (b, s)) in enumerate(digit_sum_cases(cv, c).items()):
        d = 7 + 2 * i                                        # another low digit (or, mirrored, another high digit) per case
        move = (d - 5) if name.startswith("low") else ((d - 3) << lb)
        s = [x + move for x in s]
        assert max(s) <= p["nbw"]
        want[s[0] - 1], want[s[2] - 1] = 2, 1
        bases.append(b)
        scalars += s
        ident += [False] * 3
    for k, (copies, neg) in enumerate(((32, 0), (48, 0), (16, 16), (320, 0), (160, 160))):
        bases.append(cv.p * copies + cv.neg(cv.p) * neg)
        scalars += [k + 1] * (copies + neg)
        ident += [False] * (copies + neg)
        want[k] = copies + neg
    for q, s in zip(cv.randoms, cv.random_scalars):
        bases += [q, cv.inf]
        scalars += [s, s ^ 0x5A5A]
        ident += [False, True]
    for precomp in (False, True):
        r = runs(scalars, c, precomp, ident)
        for k, n in want.items():
            assert r[k][1] == n, (k, n, r[k])                # nothing else fell into a special bucket
        for k, serial in ((0, True), (1, True), (2, True), (3, False), (4, False)):
            assert borders(r[k]) >= 1 and (borders(r[k]) <= FIXUP_SERIAL_MAX) == serial
    return b"".join(bases), scalars


_cases = {}


def cases(group, c):
    """[(name, bases, scalar bytes, expected)] of a curve and a window width, built once: the oracle's naive fold is the reference"""
    if (group, c) not in _cases:
        cv = curve(group)
        todo = dict(digit_sum_cases(cv, c))
        if c == 16:                                          # the fix-up does not depend on the width; 2^16 buckets per window only cost time
            todo.update(fixup_cases(cv, c))
        todo["mixed"] = mixed_case(cv, c)
        out = []
        for name, (bases, scalars) in todo.items():
            sc = b"".join(P.fr_to_bytes(s) for s in scalars)
            rc, ref = cv.naive(bases, sc)
            assert rc == 0
            out.append((name, bases, sc, ref))
        # the cancelling fix-up buckets are the identity (the cancelling digit sums leave s1 (P1 + P2) - s2 (P1 + P2), the oracle's business)
        named = {n: r for n, _, _, r in out}
        for n in ("16 P, 16 -P", "160 P, 160 -P"):
            assert n not in named or named[n] == cv.inf
        _cases[(group, c)] = out
    return _cases[(group, c)]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join("%s=%s" % (k.replace("ZK_", ""), v) for k, v in s.items()) or "defaults")
def test_equal_and_opposite_sums_meet_in_the_reduction(setting):
    bad = []
    for precomp in (0, 1):
        with options(dict(setting, **({"ZK_MSM_API_PRECOMP": 1} if precomp else {}))):
            for group in (0, 1):
                cv = curve(group)
                for c in (16, 17):
                    for name, bases, sc, ref in cases(group, c):
                        got = bytes(cv.G.apply_powers(sc, bases, c))
                        print("%-40s group %d c %d precomp %d: %s" % (name, group, c, precomp, "ok" if got == ref else "DIFFERS"))
                        if got != ref:
                            bad.append((name, group, c, precomp))
    assert not bad, (setting, bad)
