"""The bound discipline of the scalar field of the NTT kernels (csrc/fr29.cuh, csrc/ntt_lds.cuh), without a GPU: the constants are what they are
defined to be; no product column, quotient estimate or limb overflows at the worst-case intervals; the stage schedule of lds_ntt_stages, restated here,
keeps every operation's precondition at every one of its three call sites for s = 1 .. 10; the source lines the restatement mirrors are pinned, so that
an edit of the schedule fails here and sends its author to the model (tests/fr29_model.py).  What the device computes: tests/test_gpu_fr_field.py."""
import os
import re

import pytest

import fr29_cases as K
import fr29_model as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zukelang_amd", "csrc")
R, L, W, M, U32 = F.R, F.L, F.W, F.M, F.U32
TOP_SHIFT = W * (L - 1)


def code_of(name):
    """a source file without its // comments"""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


# ---------------------------------------------------------------------------------------------- constants
def test_every_constant_equals_its_definition():
    assert (L, W, F.NK) == (9, 29, 7) and R % (1 << W) == 1          # r = 1 mod 2^29: the quotient digit is a negation
    assert F.val(F.MOD) == R and all(0 <= x <= M for x in F.MOD)
    assert len(F.KR) == F.NK and 1 << (F.NK - 1) == 64
    for k, kr in enumerate(F.KR):
        assert F.val(kr) == R << k and len(kr) == L
        # spread form: no limb of 0..7 borrows against a weakly normalised subtrahend, and minuend + spread limb stays inside 32 bits (below 2^31)
        assert min(kr[:L - 1]) >= F.WEAK and max(kr[:L - 1]) + F.WEAK < 1 << 31 and 0 <= kr[L - 1] <= U32
        if k:          # the top limb covers that of any subtrahend of value <= (2^k - 1) r: a - b + 2^k r needs no carry pass to have a top limb >= 0
            assert kr[L - 1] >= (((1 << k) - 1) * R) >> TOP_SHIFT
    assert sum(x << (32 * i) for i, x in enumerate(F.C32)) == 32 * (1 << 256) % R and len(F.C32) == 8
    d = (R >> TOP_SHIFT) + 1
    assert F.QMUL == -(-(1 << 50) // d) == ((1 << 50) + d - 1) // d
    assert F.TOP_64R == 0x1CFB69D4          # what csrc/fr_selftest.hip admits as a top limb
    hook = open(os.path.join(CSRC, "fr_selftest.hip")).read()
    assert "FR29_TOP_64R = 0x%08xu" % F.TOP_64R in hook
    assert "{%s}" % ", ".join("0x%08xu" % x for x in F.MOD) in hook          # the host's copy of r for the argument checks, in limbs
    assert "{%s}" % ", ".join("0x%08xu" % ((R >> (32 * j)) & U32) for j in range(8)) in hook          # and in words


def test_the_quotient_estimate_is_the_quotient_or_one_less_at_every_multiple_of_r():
    """q = (top * QMUL) >> 50 against every value that has that top limb, around each multiple k r, k = 0 .. 64: never above the quotient, at most one below"""
    for k in range(65):
        for top in range(max(0, ((k * R) >> TOP_SHIFT) - 2), min(F.TOP_64R, ((k * R) >> TOP_SHIFT) + 2) + 1):
            q = (top * F.QMUL) >> 50
            lo, hi = top << TOP_SHIFT, min(((top + 1) << TOP_SHIFT) - 1, 64 * R - 1)
            assert q <= lo // R and q >= hi // R - 1, (k, top)
    # and it is monotone in between: the extremes above decide every top limb
    assert all(((t + 1) * F.QMUL) >> 50 >= (t * F.QMUL) >> 50 for t in range(0, F.TOP_64R, 0x10001))
    assert F.TOP_64R * F.QMUL < 1 << 64


# ---------------------------------------------------------------------------------------------- worst-case intervals
@pytest.mark.parametrize("A", K.PRODUCT_BOUNDS)
def test_no_product_column_reaches_2_64_at_the_interval_maxima(A):
    B = 64 // A
    p = F.iv_mul(F.iv_weak(A), F.iv_weak(B))          # every limb of both operands at 2^29 + 7, the m r terms at 2^29 - 1, carries included
    assert F.iv_mul.peak < 1 << 64 and (p.bound, p.exact) == (2, True)
    with pytest.raises(AssertionError, match="Montgomery headroom"):
        F.iv_mul(F.iv_weak(A), F.iv_weak(B + 1 if A * (B + 1) > 64 else 65))


def test_the_raw_difference_fits_a_product_by_an_exact_factor_only():
    """fr9_sub_raw<5>: limbs up to 2^31 as the FIRST operand against a factor with exact limbs -- 9 * 2^31 * 2^29 + 9 * 2^58 < 2^64"""
    assert 9 * (1 << 31) * (1 << 29) + 9 * (1 << 58) + (1 << 36) < 1 << 64
    for b in (1, 3, 24, 31):
        d = F.iv_sub_raw(F.iv_weak(24), F.iv_weak(b), 5)
        assert max(d.limbs) < 1 << 31 and d.raw_top <= U32
        F.iv_mul(d, F.iv_exact(1))
        assert F.iv_mul.peak < 1 << 64
    with pytest.raises(AssertionError, match="subtrahend"):
        F.iv_sub_raw(F.iv_weak(24), F.iv_weak(32), 5)          # 2^5 < 32 + 1
    with pytest.raises(AssertionError, match="Montgomery headroom"):
        F.iv_mul(F.iv_sub_raw(F.iv_weak(33), F.iv_weak(24), 5), F.iv_exact(1))          # 65 r
    # the carried difference and the sum are weakly normalised again, whatever the operands' limbs were
    for ki in range(1, F.NK):
        s = F.iv_sub(F.iv_weak(64 - (1 << ki)), F.iv_weak((1 << ki) - 1), ki)
        assert max(s.limbs) <= F.WEAK
    assert max(F.iv_add(F.iv_weak(32), F.iv_weak(32)).limbs) <= F.WEAK


def test_reduce_weak_takes_anything_below_64_r():
    assert F.iv_reduce_weak(F.iv_weak(64)).bound == 2
    with pytest.raises(AssertionError):
        F.iv_reduce_weak(F.iv_weak(65))


# ---------------------------------------------------------------------------------------------- the stage schedule
# The restatement.  Each step quotes the line of ntt_lds.cuh it mirrors; test_the_source_lines_the_restatement_mirrors_are_pinned holds the quotes to
# the file.
FACTOR = F.iv_exact(1)          # `const Fr9 w = fr9_load(tw + 8 * (h + j));` -- a factor read from memory: canonical, exact limbs
MIRRORED = {          # the line, and how often the file has it
    "const bool shrink = !INVERSE && (st & 3) == 3;": 1,
    "if (log_hl + log_L == 0) {": 1,
    "Fr9 x = fr9_add(u, v);": 1,
    "if (shrink) x = fr9_reduce_weak(x);": 2,          # in the span-2 stage and in the general one
    "fr9_lds_put(lds, e + hs, INVERSE ? fr9_sub<2>(u, v) : fr9_sub<5>(u, v));": 1,
    "const Fr9 t = fr9_mul(v, w);": 1,
    "x = fr9_add(u, t);": 1,
    "y = fr9_sub<2>(u, t);": 1,
    "x = fr9_add(u, v);": 1,
    "y = fr9_mul(fr9_sub_raw<5>(u, v), w);": 1,
    "const uint32_t log_hl = INVERSE ? st : s - 1 - st;": 1,
}


def dif(cur, s, contiguous):
    """lds_ntt_stages<false>: `s` stages on values inside `cur`; the last stage of a contiguous pass has span 2"""
    for st in range(s):
        shrink = (st & 3) == 3                                   # const bool shrink = !INVERSE && (st & 3) == 3;
        u = v = cur
        x = F.iv_add(u, v)                                       # x = fr9_add(u, v);
        if shrink:
            x = F.iv_reduce_weak(x)                              # if (shrink) x = fr9_reduce_weak(x);
        if contiguous and s - 1 - st == 0:                       # if (log_hl + log_L == 0) {   with log_hl = s - 1 - st
            y = F.iv_sub(u, v, 5)                                # INVERSE ? fr9_sub<2>(u, v) : fr9_sub<5>(u, v)
        else:
            y = F.iv_mul(F.iv_sub_raw(u, v, 5), FACTOR)          # y = fr9_mul(fr9_sub_raw<5>(u, v), w);
        cur = F.iv_join(x, y)
    return cur


def dit(cur, s, contiguous):
    """lds_ntt_stages<true>: the first stage of a contiguous pass has span 2"""
    for st in range(s):
        u = v = cur
        if contiguous and st == 0:                               # if (log_hl + log_L == 0) {   with log_hl = st
            x = F.iv_add(u, v)                                   # Fr9 x = fr9_add(u, v);
            y = F.iv_sub(u, v, 2)                                # INVERSE ? fr9_sub<2>(u, v) : fr9_sub<5>(u, v)
        else:
            t = F.iv_mul(v, FACTOR)                              # const Fr9 t = fr9_mul(v, w);
            x = F.iv_add(u, t)                                   # x = fr9_add(u, t);
            y = F.iv_sub(u, t, 2)                                # y = fr9_sub<2>(u, t);
        cur = F.iv_join(x, y)
    return cur


STAGES = list(range(1, 11))


@pytest.mark.parametrize("s", STAGES)
def test_forward_stages_keep_every_precondition_and_the_commented_bounds(s):
    """DIF (forward): inputs < 3r ... the outputs are < 48 r (< 56 r after the product-free last stage of a contiguous pass)"""
    for start in (F.iv_exact(1), F.iv_exact(2), F.iv_weak(3)):          # canonical from memory | cur < 2r in the fused tree | the comment's own input bound
        assert dif(start, s, False).bound <= 48
        assert dif(start, s, True).bound <= 56
    # the growth the comment states: 3, 6, 12, 24 -> 48 -> 2
    assert [dif(F.iv_weak(3), k, False).bound for k in (1, 2, 3, 4)] == [6, 12, 24, 2]
    if s >= 4:
        with pytest.raises(AssertionError):
            dif(F.iv_weak(4), s, False)          # one more r at the input and the fourth stage's u - v + 32 r no longer covers v: the model has teeth


@pytest.mark.parametrize("s", STAGES)
def test_inverse_stages_keep_every_precondition_and_the_commented_bounds(s):
    """DIT (inverse): inputs < 2r; x = u + v w < (B + 2) r, y = u - v w + 4r < (B + 4) r: after s <= 10 stages B <= 42"""
    for contiguous in (False, True):
        assert dit(F.iv_exact(1), s, contiguous).bound == 1 + 4 * s
        assert dit(F.iv_exact(2), s, contiguous).bound == 2 + 4 * s <= 42
    if s == 10:
        with pytest.raises(AssertionError):
            dit(F.iv_exact(2), 17, True)          # 2 + 4 * 16 = 66 r into a product


@pytest.mark.parametrize("s", STAGES)
def test_every_call_site_hands_over_and_takes_back_what_the_schedule_needs(s):
    canonical = F.iv_exact(1)                                    # fr9_load: unpack of a fully reduced element
    # ---- k_ntt_pass (ntt.hip): load, stages, optional scale product, optional + low half, canonical store
    for contiguous in (False, True):
        for inverse in (False, True):
            x = (dit if inverse else dif)(canonical, s, contiguous)          # Fr9 x = fr9_lds_get(lds, e);  // < 56 r
            assert x.bound <= 56
            for scale in (False, True):
                y = F.iv_mul(x, FACTOR) if scale else x                      # if (scale) x = fr9_mul(x, sc);
                F.iv_canon_store(y)                                          # fr9_store(dst + 8 * g, x);
                F.iv_canon_store(F.iv_add(y, canonical))                     # if (io.add_low ...) x = fr9_add(x, fr9_load(io.lo + 8 * g));
    # ---- k_ntt_mid (ntt.hip): forward stages, pointwise product, inverse stages on one tile
    x = dif(canonical, s, True)
    x = F.iv_mul(x, FACTOR)                                                  # fr9_mul(fr9_lds_get(lds, e), fr9_load(tab + ...)): < 2r
    assert x.bound == 2
    x = dit(x, s, True)
    assert x.bound <= 42
    F.iv_canon_store(x)
    F.iv_canon_store(F.iv_mul(x, FACTOR))
    # ---- k_tree_levels_fused (frstage.hip): levels 1 .. s on one tile, `cur` < 2r between the levels
    cur = canonical
    for lv in range(1, s + 1):
        x = dif(F.iv_join(cur, F.iv_exact(1)), lv, True)                     # lds[l][e] = low ? cur[l][e + half] : 0u;
        x = F.iv_mul(x, FACTOR)
        x = dit(x, lv, True)                                                 # Fr9 x = fr9_lds_get(lds, e);  // < 42 r
        assert x.bound <= 42
        summed = F.iv_add(x, cur)                                            # if ((e & lm) < half) x = fr9_add(x, fr9_lds_get(cur, e));
        assert summed.bound <= 44
        cur = F.iv_join(F.iv_reduce_weak(summed), F.iv_reduce_weak(x))       # fr9_lds_put(cur, e, fr9_reduce_weak(x));
        assert (cur.bound, cur.exact) == (2, True)
    F.iv_canon_store(cur)


def test_the_source_lines_the_restatement_mirrors_are_pinned():
    lds = code_of("ntt_lds.cuh")
    lines = [" ".join(x.split()) for x in lds.splitlines()]
    for quote, times in MIRRORED.items():
        assert lines.count(quote) == times, quote
    # text counts, as tests/test_fp_pair_model.py and tests/test_fp2_lane_model.py pin their schedules
    assert lds.count("(st & 3) == 3") == 1 and lds.count("fr9_sub<2>") == 2 and lds.count("fr9_sub<5>") == 1 and lds.count("fr9_sub_raw<5>") == 1
    assert lds.count("fr9_reduce_weak") == 2 and lds.count("fr9_mul(") == 2 and lds.count("fr9_add(") == 3
    assert re.search(r"static constexpr int NTT_LOG_T = 10;", lds)
    # the three call sites and what surrounds the stages there
    ntt, frs = code_of("ntt.hip"), code_of("frstage.hip")
    assert ntt.count("lds_ntt_stages<") == 3 and frs.count("lds_ntt_stages<") == 2
    assert ntt.count("lds_ntt_stages<false>(lds, tw_fwd, T, s, 0, 0, 0, false);") == 1 and ntt.count("lds_ntt_stages<true>(lds, tw_inv, T, s, 0, 0, 0, false);") == 1
    assert ntt.count("lds_ntt_stages<INVERSE>(lds, tw, T, a.s, a.log_RS, log_L, c0, a.strided != 0);") == 1
    assert frs.count("lds_ntt_stages<false>(lds, tw_fwd, T, lv, 0, 0, 0, false);") == 1 and frs.count("lds_ntt_stages<true>(lds, tw_inv, T, lv, 0, 0, 0, false);") == 1
    assert frs.count("fr9_lds_put(cur, e, fr9_reduce_weak(x));") == 1 and frs.count("if ((e & lm) < half) x = fr9_add(x, fr9_lds_get(cur, e));") == 1
    assert ntt.count("if (scale) x = fr9_mul(x, sc);") == 2 and ntt.count("x = fr9_add(x, fr9_load(io.lo + 8 * g));") == 1
    # the stage counts the plan can ask for: a tile of at most 2^NTT_LOG_T elements, strided passes of at most NTT_LOG_T - 2 stages
    assert "const uint32_t smax = log_T - 2;" in ntt and "uint32_t s_last = log_len < log_T ? log_len : log_T;" in ntt
    # the header names this model
    assert "tests/fr29_model.py" in open(os.path.join(CSRC, "fr29.cuh")).read()
    assert not os.path.exists(os.path.join(ROOT, "scripts", "proto", "fr29_model.py")) or len(open(os.path.join(ROOT, "scripts", "proto", "fr29_model.py")).read().splitlines()) <= 3


# ---------------------------------------------------------------------------------------------- the functions on integers
def test_sampled_single_steps():
    assert F.sampled_checks(seed=1) == (20000, 3000)


def test_the_operand_classes_of_the_gpu_test_hold_on_the_model():
    """tests/fr29_cases.py through the integer model: every class occurs, every precondition holds (the model asserts them), every expectation is met"""
    seen = {}
    for kind, l in K.reduce_cases():
        assert K.is_weak(l) and l[L - 1] <= F.TOP_64R and F.val(l) < 64 * R
        r = F.reduce_weak(l)
        assert F.val(r) % R == F.val(l) % R and F.val(r) < 2 * R and K.is_exact(r)
        assert F.canon(l) == F.val(l) % R
        for c in (kind, K.reduce_class(l)):
            seen[c] = seen.get(c, 0) + 1
        assert F.canon_limbs(l)[1] == (K.reduce_class(l) == "estimate short by one, subtraction taken")
    assert set(seen) == {"exact", "pending", "ripple", "largest", "top limb k D", "estimate exact, no subtraction", "estimate short by one, subtraction taken"}
    assert min(seen.values()) >= 2 and seen["pending"] >= 64, seen
    kinds = set()
    for label, ku, kv, A, B, u, v in K.product_cases():
        assert F.val(u) < A * R and F.val(v) < B * R and A * B <= 64 and K.is_weak(u) and K.is_weak(v)
        p = F.mul(u, v)
        assert (F.val(p) * F.RP - F.val(u) * F.val(v)) % R == 0 and F.val(p) < 2 * R and K.is_exact(p)
        kinds.add((label, ku, kv, A))
    for A in K.PRODUCT_BOUNDS:
        assert {(lab, "exact", "exact", A) for lab in ("top", "mixed", "random")} <= kinds
        assert any(k[3] == A and "pending" in k[1:3] for k in kinds), A
    labels = {}
    for label, u, v, w in K.forward_cases():
        assert F.val(u) < 24 * R and F.val(v) < 24 * R and F.val(w) < R and K.is_exact(w)
        x = F.add(u, v)
        K.check_forward(u, v, w, x, F.reduce_weak(x), F.mul(F.sub_raw(u, v, 5), w), F.mul(F.sub(u, v, 5), w), F.sub(u, v, 5))
        labels[label] = labels.get(label, 0) + 1
    assert {"v at the bound", "both at the bound", "u = v", "u at the bound", "v above u + 16 r", "random"} <= set(labels), labels
    assert any("pending" in x for x in labels)
    labels = {}
    for label, u, v, w in K.inverse_cases():
        assert F.val(u) < 38 * R and F.val(v) < 42 * R and F.val(w) < R and K.is_exact(w)
        t = F.mul(v, w)
        K.check_inverse(u, v, w, t, F.add(u, t), F.sub(u, t, 2))
        labels[label] = labels.get(label, 0) + 1
    assert {"at the bounds", "zero", "random"} <= set(labels) and any("pending" in x for x in labels)
    for v in K.word_cases():
        assert F.pack_exact(F.unpack_words(F.words8(v))) == F.words8(v)
