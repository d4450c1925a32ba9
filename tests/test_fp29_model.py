"""The integer model of the base-field limb layer (tests/fp29_model.py) over the case table (tests/fp29_cases.py), without a GPU.  Values are compared with
plain `%` and pow(x, -1, p); the model's own assertions hold what the device code relies on without checking.

Rows of the three tables of spread multiples of p.  REACHABLE is computed here from FP_MAX_BOUND as ff.cuh states it: the rows a function's template
arguments can select without tripping a static_assert.  INSTANTIATED is a record, and this is how it was obtained: in a scratch copy of ff.cuh every
function below was given a static_assert that fails for every template argument; every translation unit of zukelang_amd/csrc at this commit was
compiled with -fsyntax-only -ferror-limit=0, and the template arguments were read off the compiler's "in instantiation of function template
specialization" notes, keyed by the line of the failing assertion.  It is not recomputed here (that takes a compiler and a minute): the test holds it
to REACHABLE, holds the hook's instantiations (csrc/fp29_selftest.hip) to all of REACHABLE, and holds the direct uses of the tables in the sources
to the list below, so that a new use of a table is noticed.  Rows nobody instantiates are listed in DESIGN.md."""
import os
import re

import pytest

import fp29_cases as Cs
import fp29_model as F

P = F.P
FF = open(os.path.join(F.CSRC, "ff.cuh")).read()
FP_INV = open(os.path.join(F.CSRC, "fp_inv.cuh")).read()

# function -> the subtrahend / operand bounds it is instantiated with by the shipped kernels (every .hip of csrc but the selftest units of this hook)
INSTANTIATED_BOUNDS = {
    "fe_sub": [1, 2, 3, 4, 7, 8, 10, 12, 15, 18, 20, 26, 30, 31, 36, 42, 60, 64, 66, 74, 120, 128, 138, 256, 312, 936],
    "fe_neg": [1, 2, 10, 30, 64, 256],
    "fe_neg_lazy": [2, 4, 64, 65],
    "fe_sub_sub_dbl": [2 + 2 * 2, 3 + 2 * 3, 10 + 2 * 10, 64 + 2 * 64],          # B + 2 C of the instantiated (B, C)
}
INSTANTIATED_ROWS = {"fe_sub": ("KP", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]), "fe_neg": ("KP", [0, 1, 3, 4, 6, 8]), "fe_neg_lazy": ("KPN", [1, 2, 6]),
                     "fe_sub_sub_dbl": ("KPW", [2, 3, 4, 7])}
IS_ZERO_BOUNDS = [2, 4, 6, 8, 12, 26, 64, 68, 80, 130, 131, 132, 138, 192]          # fe_is_zero<B> of FpB, found the same way
# tables named directly, outside the four functions: fp_inv29_call adds 32 p (KP row 4), fp2h_mul_body negates with 256 p (KPN row 7), and fe_sqr of
# Fp2HB<A> subtracts with KPN row fp_ki(fp_ks(A)): instantiated with the A below, KPN rows 1, 2, 3, 6, 7
FP2H_SQR_BOUNDS = [2, 4, 6, 8, 12, 64, 128, 130, 131, 192]
DIRECT_USES = {"ff.cuh": ["FP29_KP[KI][i]", "FP29_KPW[KI][i]", "FP29_KPN[KI][i]", "FP29_KP[KI][i]", "FP29_KPN[KI][i]", "FP29_KPN[KI][i]"], "fp_inv.cuh": ["FP29_KP[KI][i]"]}


def reachable_rows():
    mx = int(re.search(r"FP_MAX_BOUND = (\d+);", FF).group(1))
    assert mx == F.FP_MAX_BOUND
    r = {"fe_sub": set(), "fe_neg": set(), "fe_neg_lazy": set(), "fe_sub_sub_dbl": set()}
    for b in range(1, mx + 1):
        ki = F.fp_ki(F.fp_ks(b))
        if ki < F.NK:
            if 1 + F.fp_ks(b) <= mx:          # the result type FpB<A + fp_ks(B)> exists for some A >= 1
                r["fe_sub"].add(ki)
                if ki >= 1 and b >= 3:        # B + 2 C >= 3
                    r["fe_sub_sub_dbl"].add(ki)
            if F.fp_ks(b) <= mx:              # FpB<fp_ks(A)>; FpLazyNeg has no bound of its own, KI < FP29_NK is its limit
                r["fe_neg"].add(ki)
            r["fe_neg_lazy"].add(ki)
    return {k: sorted(v) for k, v in r.items()}


def test_every_row_of_every_table_is_a_power_of_two_times_p_inside_its_stated_spread():
    F.check_tables()
    for k in range(F.NK):
        assert F.val(F.KP[k]) == F.val(F.KPN[k]) == (2 << k) * P
        if k:
            assert F.val(F.KPW[k]) == (2 << k) * P
    # the other constants
    assert F.val(F.MOD) == P and all(x <= F.M for x in F.MOD)
    assert (F.NINV * P + 1) % (1 << F.W) == 0 and (F.PINV * P - 1) % (1 << F.W) == 0
    for k, c in enumerate((F.R1, F.R2, F.R3), 1):
        assert F.val(c) == pow(2, F.RBITS * k, P) and all(x <= F.M for x in c)
    assert float(F.PTOP_INV) == pytest.approx(1.0 / ((P >> 348) + 1), rel=2 ** -23)


def test_fp_ks_and_fp_ki_map_each_bound_to_the_row_the_header_uses():
    assert "constexpr int fp_ks(int b) { int k = 2; while (k < b + 1) k <<= 1; return k; }" in FF
    assert "constexpr int fp_ki(int k) { int i = 0; while ((2 << i) < k) i++; return i; }" in FF
    for b in range(1, F.FP_MAX_BOUND):
        k = F.fp_ks(b)
        assert k > b and (k == 2 or k // 2 <= b) and k & (k - 1) == 0          # the smallest power of two above b, at least 2
        assert F.val(F.KP[F.fp_ki(k)]) == k * P
    for row in range(F.NK):
        assert F.fp_ki(F.fp_ks(Cs.row_bound(row))) == row


@pytest.mark.parametrize("fn", ["fe_sub", "fe_neg", "fe_neg_lazy", "fe_sub_sub_dbl"])
def test_reachable_rows_instantiated_rows_and_the_rows_the_hook_builds(fn):
    reach = reachable_rows()[fn]
    assert reach == {"fe_sub": Cs.SUB_ROWS, "fe_neg": Cs.NEG_ROWS, "fe_neg_lazy": Cs.NEG_ROWS, "fe_sub_sub_dbl": Cs.SSD_ROWS}[fn]
    table, rows = INSTANTIATED_ROWS[fn]
    assert sorted({F.fp_ki(F.fp_ks(b)) for b in INSTANTIATED_BOUNDS[fn]}) == rows
    assert set(rows) <= set(reach)
    assert sorted(Cs.additive_cases()[fn]) == reach, "the case table does not hold every reachable row"
    print("%s: table %s, reachable rows %s, instantiated by the shipped kernels %s, never instantiated %s" % (fn, table, reach, rows, sorted(set(reach) - set(rows))))


def test_direct_uses_of_the_tables_in_the_sources_are_the_known_ones():
    for name, src in (("ff.cuh", FF), ("fp_inv.cuh", FP_INV)):
        assert re.findall(r"FP29_KP[NW]?\[[^\]]*\]\[[^\]]*\]", src) == DIRECT_USES[name], name
    for f in os.listdir(F.CSRC):
        if f.endswith((".hip", ".cuh", ".h", ".cpp")) and f not in ("ff.cuh", "fp_inv.cuh", "fp29_consts.cuh"):
            assert "FP29_KP" not in open(os.path.join(F.CSRC, f)).read(), f
    assert "constexpr int KI = fp_ki(32);" in FP_INV and "FP2H_NEG_K = 256" in FF
    assert max(IS_ZERO_BOUNDS) == Cs.ZERO_BOUNDS[-1] and F.FP_REST in IS_ZERO_BOUNDS and 2 in IS_ZERO_BOUNDS


def test_reduction_of_every_k_p_and_its_neighbours_up_to_8192_p():
    cases = Cs.reduction_cases()
    stats = {}
    for name, cl in cases.items():
        assert cl, "empty class %s" % name
        for l in cl:
            r = F.canon(l, stats)
            assert F.val(r) == F.val(l) % P
    assert len(cases["exact"]) == 4 * Cs.CANON_BOUND - 1
    assert all(l != F.unpack(F.val(l)) for l in cases["weak"]) and all(l[:13] == [F.WEAK] * 13 for l in cases["all_weak"])
    assert max(F.val(l) for l in cases["exact"]) == Cs.CANON_BOUND * P - 1
    # Q - q: all three values occur, found with the model
    assert sorted(stats) == [0, 1, 2] and all(stats[d] > 0 for d in (0, 1, 2)), stats
    print("reduction: %s lanes; Q - q counts %s" % ({k: len(v) for k, v in cases.items()}, stats))


def test_the_header_s_decrement_and_second_subtraction_are_live_code():
    """what a build without `q = q ? q - 1 : 0`, or with one conditional subtraction, returns on the table: the model shows both mutations"""
    cases = Cs.reduction_cases()["exact"]
    no_dec = sum(1 for l in cases[::7] if F.val(F.canon(l, dec=False)) != F.val(l) % P)
    one_sub = sum(1 for l in cases[::7] if F.val(F.canon(l, reps=1)) != F.val(l) % P)
    assert no_dec > 0 and one_sub > 0
    print("without the decrement %d of %d wrong; with one subtraction %d of %d wrong" % (no_dec, len(cases[::7]), one_sub, len(cases[::7])))


def test_multiples_of_p_have_one_weak_form():
    """why the classes of true multiples hold exact limbs: no k p, k p - 1 or k p + p - 1 below 8192 p has a limb small enough to hold a pending carry"""
    assert all(Cs.no_second_weak_form(k * P) and Cs.no_second_weak_form(k * P - 1) for k in range(1, F.FP_MAX_BOUND + 1))


@pytest.mark.parametrize("b", Cs.ZERO_BOUNDS)
def test_zero_test_classes_in_both_slow_path_forms(b):
    cases = Cs.zero_cases()[b]
    slow = 0
    for name, cl in cases.items():
        assert cl, "empty class %s" % name
        for l in cl:
            want = F.val(l) % P == 0
            for form in ("call", "inline"):
                got, path = F.is_zero(l, b, form)
                assert got == want, (name, form)
            assert path == {"multiples": "slow", "non_multiples_small_k": "slow", "k_at_least_B": "fast", "exact_zero": "zero"}[name], (name, path)
            slow += path == "slow"
            assert F.is_zero_mod_p_inline(l) == (F.val(l) == ((l[0] * F.PINV) & F.M) * P)
    assert len(cases["multiples"]) == b - 1
    assert any(l != F.unpack(F.val(l)) for l in cases["non_multiples_small_k"])
    print("fe_is_zero<%d>: %s; %d reach the slow path" % (b, {k: len(v) for k, v in cases.items()}, slow))


def test_additive_rows_at_the_limb_maxima_and_at_zero():
    ac = Cs.additive_cases()
    n = 0
    for row, cl in ac["fe_sub"].items():
        assert cl
        for x, y in cl:
            assert F.val(F.fe_sub(x, y, Cs.row_bound(row))) == F.val(x) - F.val(y) + (2 << row) * P
            n += 1
    for fn, f in (("fe_neg", F.fe_neg), ("fe_neg_lazy", F.fe_neg_lazy)):
        for row, cl in ac[fn].items():
            assert cl
            for (x,) in cl:
                assert F.val(f(x, Cs.row_bound(row))) == (2 << row) * P - F.val(x)
                n += 1
    for row, cl in ac["fe_sub_sub_dbl"].items():
        assert cl
        b = Cs.row_bound(row - 1)
        for x, y, z in cl:
            assert F.val(F.fe_sub_sub_dbl(x, y, z, b, b)) == F.val(x) - F.val(y) - 2 * F.val(z) + (2 << row) * P
            n += 1
    # every row sees limbs 0..12 at 2^29 + 7 and all-zero limbs on every side
    for fn, rows in ac.items():
        for row, cl in rows.items():
            for side in range(len(cl[0])):
                assert any(ops[side][:13] == [F.WEAK] * 13 for ops in cl) and any(not any(ops[side]) for ops in cl), (fn, row, side)
    for fn, cl in Cs.add_cases().items():
        assert cl
        for ops in cl:
            r = {"fe_add": F.fe_add, "fe_dbl": F.fe_dbl, "fp_carry": lambda t: F.carry(list(t))}[fn](*ops)
            if fn != "fp_carry":
                assert F.val(r) == sum(F.val(o) for o in ops) * (2 if fn == "fe_dbl" else 1)
            else:
                assert F.val(r) % (1 << (F.TOPSHIFT + 32)) == F.val(ops[0]) % (1 << (F.TOPSHIFT + 32))
    print("additive lanes: %d" % n)


def test_a_table_row_whose_spread_claim_breaks_is_caught_by_the_model():
    """limb 3 of FP29_KP row 4 one more and limb 2 less by 2^29: the value is still 32 p, the spread claim (limbs at least 2^30 - 2) is not, and the
    model's table check says so.  On the device the same edit changes no value but moves a carry: tests/test_gpu_fp29.py sees it in the raw limbs."""
    row = list(F.KP[4])
    row[3] += 1
    row[2] -= 1 << 29
    assert F.val(row) == 32 * P
    saved = F.KP[4]
    F.KP[4] = row
    try:
        with pytest.raises(AssertionError):
            F.check_tables()
    finally:
        F.KP[4] = saved
    F.check_tables()


def test_pack_and_unpack_round_trip_below_p():
    cl = Cs.pack_cases()["below_p"]
    assert cl
    for v in cl:
        l = F.unpack_words(F.words12(v))
        assert l == F.unpack(v) and F.pack(l) == F.words12(v)


INV_CHUNKS = 10


def _all_inversion_operands():
    fam = Cs._families()
    return [x for k in sorted(fam) for x in fam[k]]


@pytest.mark.parametrize("chunk", range(INV_CHUNKS))
def test_inversion_model_on_the_families(chunk):
    xs = _all_inversion_operands()[chunk::INV_CHUNKS]
    assert xs
    for x in xs:
        limbs, zero_at = Cs.inversion_expected(x)
        if x:
            assert F.val(limbs) % P == pow(x, -1, P) and 4 * P < F.val(limbs) < 60 * P and 1 <= zero_at <= F.FP_INV_ITERS
        else:
            assert limbs == [0] * F.L


@pytest.mark.slow
def test_inversion_classes_are_populated_and_the_search_finds_nothing_longer_than_27():
    ic = Cs.inversion_cases()
    for name, cl in ic.items():
        assert cl, "empty class %s" % name
    full = ic["needs_all_27"]
    assert len(full) >= 32
    assert (1 << 380) in full and 3 << 379 in full
    assert len(ic["wrong_after_26"]) >= 16
    found, runs = Cs.inversion_search()
    assert runs == Cs.SEARCH_BUDGET
    assert all(s <= F.FP_INV_ITERS for _, s in found), "an operand needs a 28th iteration: %s" % [hex(x) for x, s in found if s > F.FP_INV_ITERS]
    worst = max((Cs._run(x)[2], x) for cl in ic.values() for x in cl)
    assert worst[0] < 3 * P
    print("inversion: %s; search: %d runs, %d more full-length operands, none longer; max |u|, |v| = %.3f p at X = %s"
          % ({k: len(v) for k, v in ic.items()}, runs, len(found), worst[0] / P, hex(worst[1])))


@pytest.mark.slow
def test_the_inversion_needs_its_27th_iteration():
    """what a build with FP_INV_ITERS = 26 computes: the model shows the mutation, on the operands that reach b = 1 only in the last iteration"""
    late = Cs.inversion_cases()["wrong_after_26"]
    assert len(late) >= 16 and 3 << 379 in late
    assert (1 << 380) not in late          # b = 1 long before a = 0: its v is final early, and 26 iterations return the right inverse
