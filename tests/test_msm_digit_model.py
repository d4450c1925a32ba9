"""The integer model of the signed-digit recoding (tests/msm_digit_model.py) against the arithmetic it restates: the digits of every family member and of
seeded random scalars add up to the scalar at every width and in both forms, stay in range and never leave the c nw bits the device keeps; a bound
over ALL scalars; the model's lines pinned to the sources by text; and the ends every family list must reach.  No GPU."""
import os
import random

import pytest

import msm_digit_model as M
from oracle import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(c, fold) for c in M.WIDTHS for fold in M.forms(c)]
IDS = ["c%d%s" % (c, "-folded" if fold else "") for c, fold in CASES]


def source(name):
    return open(os.path.join(ROOT, "zukelang_amd", "csrc", name)).read()


def test_the_model_is_pinned_to_the_sources():
    assert M.R == P.R and M.HALF * 2 + 1 == M.R
    msm = source("msm.cuh")
    for line in ("static inline bool msm_fold(uint32_t c, bool precomp, bool in_subgroup) { return precomp && in_subgroup && 255 % c == 0; }",
                 "static inline uint32_t msm_windows(uint32_t c, bool fold = false) { return fold && 255 % c == 0 ? 255 / c : 255 / c + 1; }"):
        assert line in msm, line
    dig = source("msm_digits.cuh")
    for line in ("const uint32_t e = (uint32_t)(x >> b) & ((1u << a.c) - 1);",
                 "const uint32_t bias = (1u << (a.c - 1)) - 1;",
                 "if (e == bias) return false;",
                 "const uint32_t below = e < bias ? 1u : 0u;",
                 "const uint32_t d = below ? bias - e : e - bias;",
                 "const uint32_t neg = below ^ (s[8] >> 31);",
                 "key = (a.precomp ? 0u : j * a.nb_per_window) + (d - 1);",
                 "val = (uint32_t)(a.precomp ? (uint64_t)j * a.n + i : i) | (neg << 31);",
                 # the flip rule: t = r - s word by word, compared from the top word down, taken when t < s
                 "bw += (int64_t)FR_MOD[k] - (int64_t)s[k];",
                 "if (!decided && t[k] != s[k]) { less = t[k] < s[k]; decided = true; }",
                 "if (less) {",
                 "flip = 0x80000000u;",
                 "for (int k = 0; k < 8; k++) s[k] = t[k];",
                 "cy += (uint64_t)s[k] + a.K[k];",
                 "s[8] |= flip;",
                 "if ((int)w + 1 == k) x1 = k == 8 ? s[k] & 0x7fffffffu : s[k];",
                 # digit_constant
                 "uint64_t v = ((uint64_t)1 << (c - 1)) - 1;",
                 "uint32_t off = j * c, wd = off >> 5, sh = off & 31;"):
        assert line in dig, line
    tail = source("msm_tail.cuh")
    for line in ("p.nbw = 1u << (c - 1);", "p.lb = (c + 1) / 2;", "p.nd0 = 1u << p.lb;", "p.nd1 = (p.nbw >> p.lb) + 1;"):
        assert line in tail, line
    res = source("msm_resident.hip")
    assert "static constexpr uint32_t SHORT_C = %d;" % M.SHORT_C in res and 255 % M.SHORT_C == 0
    assert "static constexpr uint32_t SHORT_BUCKETS = 1u << (SHORT_C - 1);" in res
    assert "!digit_at(s, i, j, da, key, val) || key != bucket) continue;" in res
    assert M.msm_windows(M.SHORT_C, 1) == 51 and M.msm_windows(M.SHORT_C, 0) == 52
    # who folds: the entry points zk_msm_g1 / zk_msm_g2 never test the subgroup, so they never fold, whatever ZK_MSM_API_PRECOMP says; a resident handle
    # and a proving key fold when their upload ran the test
    api = source("msm.hip")
    assert "ZKCHK(msm_bases_from_bytes(b, curve, bases, nscalars, window_bits, precomp, c.stream));" in api
    assert "hipStream_t s, bool check_subgroup = false);" in msm
    points = source("msm_points.hip")
    assert "b.fold = msm_fold(c, precomp, in_subgroup); b.nw = msm_windows(c, b.fold);" in points
    assert 'if (c < 2 || c > 22) ZK_FAIL(ZK_ERR_ARG, "msm: window_bits must be in [2, 22]");' in points and list(M.WIDTHS) == list(range(2, 23))
    assert [c for c in M.WIDTHS if 255 % c == 0] == [3, 5, 15, 17]


def check_scalar(s, c, fold):
    nw, top = M.msm_windows(c, fold), 1 << (c - 1)
    rc = M.recode(s, c, fold)
    assert len(rc.raw) == nw
    assert sum(d << (c * j) for j, d in enumerate(rc.digits)) == (s - M.R if rc.flipped else s), (s, c, fold)
    assert all(-(top - 1) <= d <= top for d in rc.raw), (s, c, fold)
    p = M.digit_plan(c)
    for w in (abs(d) for d in rc.raw if d):                                  # the bucket's weight w = hi 2^lb + lo has a place among the plan's digit values
        assert w >> p["lb"] < p["nd1"] and w & (p["nd0"] - 1) < p["nd0"] and ((w >> p["lb"]) << p["lb"]) + (w & (p["nd0"] - 1)) == w <= p["nbw"], (s, c, fold, w)
    x, flipped = M.digits_prepare(s, c, fold)
    assert x >> (c * nw) == 0, (s, c, fold)                                  # s' + K never leaves the c nw bits of the windows
    assert flipped == rc.flipped == (bool(fold) and M.R - s < s)
    assert [k for k, _, _ in rc.keys_precomp] == [abs(d) - 1 for d in rc.digits if d]
    assert [k for k, _, _ in rc.keys_classic] == [j * top + abs(d) - 1 for j, d in enumerate(rc.digits) if d]
    assert all(0 <= k < top for k, _, _ in rc.keys_precomp) and all(0 <= k < nw * top for k, _, _ in rc.keys_classic)
    return rc


@pytest.mark.parametrize("c,fold", CASES, ids=IDS)
def test_the_digits_add_up_to_the_scalar(c, fold):
    nw = M.msm_windows(c, fold)
    assert c * nw - 256 <= 20 and c * (nw - 1) <= 255                        # the top window's field never meets the flip bit (bit 31 of word 8) and starts below word 8
    assert all(((c * j) & 31) + c <= 64 for j in range(nw))                  # a window never spans more than the two words digit_at reads
    assert M.digit_constant(c, nw) < 1 << (c * nw - 1)
    rng = random.Random(0xD161 + 64 * c + fold)
    for _, s in M.families(c, fold):
        check_scalar(s, c, fold)
    for _ in range(2000):
        check_scalar(rng.randrange(1, M.R), c, fold)
    assert M.recode(0, c, fold).keys_precomp == []


@pytest.mark.parametrize("c,fold", CASES, ids=IDS)
def test_every_scalar_fits_the_windows(c, fold):
    """Not a sample: the digit vectors of nw windows are in bijection with the integers of [-K, largest_sum] (s + K runs through every value of
    c nw bits), so every s' in [0, bound] has digits as soon as largest_sum >= bound"""
    nw = M.msm_windows(c, fold)
    K = M.digit_constant(c, nw)
    assert M.largest_sum(c, fold) + K == (1 << (c * nw)) - 1
    assert M.largest_sum(c, fold) >= M.bound(fold)
    assert M.bound(0) == M.R - 1 and M.bound(1) == (M.R - 1) // 2
    if fold:
        assert M.largest_sum(c, 0) >= M.R - 1 and M.msm_windows(c, 0) == nw + 1     # the same width unfolded: one window more
        assert M.largest_sum(c, 1) < M.R - 1                                        # and the folded windows do NOT hold every canonical scalar: the flip is needed
    assert M.digits_prepare(M.bound(fold), c, fold)[0] >> (c * nw) == 0


@pytest.mark.parametrize("c,fold", CASES, ids=IDS)
def test_the_families_are_what_their_names_say(c, fold):
    nw, top, low = M.msm_windows(c, fold), 1 << (c - 1), -((1 << (c - 1)) - 1)
    fam = M.families(c, fold)
    named = dict(fam)
    assert len(named) == len(fam) <= 300                                     # names are unique; a list fits one product of the GPU tests
    J, s = M.all_top(c, fold)
    assert J == nw - 1 and M.recode(s, c, fold).raw == [top] * J + [0] and not M.recode(s, c, fold).flipped
    J, s = M.all_bottom(c, fold)
    assert J == nw - 1 and M.recode(s, c, fold).raw == [low] * J + [1] and not M.recode(s, c, fold).flipped
    for name, s in fam:
        rc = M.recode(s, c, fold)
        kind, _, at = name.partition("@")
        if kind == "top" and "," not in at:
            j = int(at)
            assert rc.raw == [0] * j + [top] + [0] * (nw - 1 - j) and rc.keys_precomp == [(top - 1, False, j)] and rc.keys_classic == [(j * top + top - 1, False, j)]
        elif kind == "top":
            assert rc.raw == [low] * (nw - 1) + [top] and s == M.top_in_last(c, fold)
        elif kind == "carry":
            j = int(at)
            assert rc.raw == [0] * j + [low, 1] + [0] * (nw - 2 - j)
    if M.top_in_last(c, fold) is not None:
        assert M.top_in_last(c, fold) - 1 < M.top_in_last(c, fold) and M.recode(M.top_in_last(c, fold) - 1, c, fold).raw[nw - 1] != top      # it is the least such value
    else:
        assert M.recode(M.bound(fold), c, fold).raw[nw - 1] < top
    if fold:
        for name, s, t in M.mirror_pairs(c):
            a, b = M.recode(s, c, fold), M.recode(t, c, fold)
            assert s + t == M.R and a.flipped != b.flipped and a.raw == b.raw and a.digits == [-d for d in b.digits]
            assert [(k, j) for k, _, j in a.keys_precomp] == [(k, j) for k, _, j in b.keys_precomp]
            assert [n for _, n, _ in a.keys_precomp] == [not n for _, n, _ in b.keys_precomp]
    else:
        assert not any(name.startswith("mirror") for name in named)


@pytest.mark.parametrize("c,fold", CASES, ids=IDS)
def test_the_families_reach_every_end(c, fold):
    scalars = [s for _, s in M.families(c, fold)]
    got = M.check_coverage(c, fold, scalars)
    print("c %2d fold %d: %3d scalars, top digit in windows 0..%d%s, %d with a digit in the last window, %d flipped" % (
        c, fold, len(scalars), max(got["tops"]), "" if M.top_in_last(c, fold) is None else " (the last one)", got["last"], got["flipped"]))
    # the checks bite: an emptied family fails them
    without = [s for n, s in M.families(c, fold) if not n.startswith("top@") and not n.endswith("all top")]
    with pytest.raises(AssertionError):
        M.check_coverage(c, fold, without)
    # "all top" and "all bottom" alone reach windows 0 .. J - 1 = nw - 2, which check_coverage demands; with J shrunk by one they lose window J - 1
    nw = M.msm_windows(c, fold)
    (J, t), (Jb, b) = M.all_top(c, fold), M.all_bottom(c, fold)
    whole = M.coverage(c, fold, [t, b])
    assert whole["tops"] == whole["bottoms"] == set(range(nw - 1)) and J == Jb == nw - 1
    t1 = sum((1 << (c - 1)) << (c * j) for j in range(J - 1))
    b1 = (1 << (c * (J - 1))) - sum(M.bias(c) << (c * j) for j in range(J - 1))
    less = M.coverage(c, fold, [t1, b1])
    assert less["tops"] == less["bottoms"] == set(range(nw - 2))


def test_the_short_path_is_the_folded_five_bit_plan():
    assert M.msm_fold(M.SHORT_C, True, True) and not M.msm_fold(M.SHORT_C, True, False) and not M.msm_fold(M.SHORT_C, False, True)
    assert M.digit_plan(M.SHORT_C)["nbw"] == 16
    for fold in (0, 1):
        keys = {k for _, s in M.families(M.SHORT_C, fold) for k, _, _ in M.recode(s, M.SHORT_C, fold).keys_precomp}
        assert keys >= {0, 14, 15}                                           # digit 1, the bottom digit's bucket and the top bucket of the sixteen
