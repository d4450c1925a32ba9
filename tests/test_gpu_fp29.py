"""GPU parity of the layer under every Fp product (csrc/ff.cuh, csrc/fp_inv.cuh) on bare limbs: zk_selftest_fp29 takes every class of tests/fp29_cases.py
through the shipped functions, and the raw limbs that come back are compared limb for limb with the integer model (tests/fp29_model.py) and by value
with Python integers -- plain `%`, pow(x, -1, p).  No tolerances.  What only this hook reaches: the integer 2^380 (and the other operands that keep
fp_inv29_call busy for all 27 iterations) arriving AS that integer, values up to 8192 p at the quotient estimate with Q - q = 0, 1 and 2, non-multiples
of p on the slow path of the zero test in both of its compiled forms, and every reachable row of the three tables of spread multiples of p."""
import ctypes as C

import numpy as np
import pytest

import fp29_cases as Cs
import fp29_model as F
from zukelang_amd import _lib

pytestmark = pytest.mark.gpu
P, L = F.P, F.L
P32 = C.POINTER(C.c_uint32)
OUT_WORDS = {4: 26, 5: 28, 8: 1, 9: 1, 10: 1}


def run(op, lanes):
    """lanes: tuples of up to three limb lists -> one list of output words per lane"""
    n = len(lanes)
    words = np.zeros((n, 48), dtype=np.uint32)
    for i, lane in enumerate(lanes):
        for s, l in enumerate(lane):
            words[i, 16 * s:16 * s + len(l)] = l
    ow = OUT_WORDS.get(op, 14)
    out = np.full((n, ow), 0xDEADBEEF, dtype=np.uint32)
    _lib.check(_lib.lib().zk_selftest_fp29(C.c_int(op), words.ctypes.data_as(P32), C.c_size_t(n), out.ctypes.data_as(P32)))
    return [[int(x) for x in row] for row in out]


def test_full_reduction_of_every_k_p_and_its_neighbours_up_to_8192_p():
    cases = Cs.reduction_cases()
    lanes, stats = [], {}
    for name in ("exact", "weak", "all_weak"):
        assert cases[name], name
        lanes += cases[name]
    got = run(0, [(l,) for l in lanes])
    for l, g in zip(lanes, got):
        assert g == F.canon(l, stats), [hex(x) for x in l]
        assert F.val(g) == F.val(l) % P and all(x <= F.M for x in g)
    assert all(stats.get(d, 0) > 0 for d in (0, 1, 2)), stats          # the estimate was off by 0, 1 and 2 on lanes the device reduced


@pytest.mark.parametrize("which", range(3))
def test_zero_test_in_both_compiled_forms_and_the_inline_reduction(which):
    b = Cs.ZERO_BOUNDS[which]
    cases = Cs.zero_cases()[b]
    lanes, names = [], []
    for name, cl in cases.items():
        assert cl, name
        lanes += cl
        names += [name] * len(cl)
    got = run(8 + which, [(l,) for l in lanes])
    slow = 0
    for l, name, (g,) in zip(lanes, names, got):
        want = F.val(l) % P == 0
        k = (l[0] * F.PINV) & F.M
        direct = F.val(l) == k * P
        assert g == (1 if want else 0) | (2 if want else 0) | (4 if direct else 0), (b, name, [hex(x) for x in l], g)
        assert F.is_zero(l, b, "call")[0] == F.is_zero(l, b, "inline")[0] == want and F.is_zero_mod_p_inline(l) == direct
        slow += F.is_zero(l, b, "call")[1] == "slow"
    assert slow >= len(cases["multiples"]) + len(cases["non_multiples_small_k"]) > 0


def test_every_reachable_row_of_the_three_tables():
    ac = Cs.additive_cases()
    for fn, base, model in (("fe_sub", 16, lambda row, x, y: F.fe_sub(x, y, Cs.row_bound(row))),
                            ("fe_neg", 32, lambda row, x: F.fe_neg(x, Cs.row_bound(row))),
                            ("fe_neg_lazy", 48, lambda row, x: F.fe_neg_lazy(x, Cs.row_bound(row))),
                            ("fe_sub_sub_dbl", 64, lambda row, x, y, z: F.fe_sub_sub_dbl(x, y, z, Cs.row_bound(row - 1), Cs.row_bound(row - 1)))):
        rows = ac[fn]
        assert sorted(rows) == {"fe_sub": Cs.SUB_ROWS, "fe_neg": Cs.NEG_ROWS, "fe_neg_lazy": Cs.NEG_ROWS, "fe_sub_sub_dbl": Cs.SSD_ROWS}[fn]
        for row, cl in rows.items():
            assert cl, (fn, row)
            got = run(base + row, cl)
            k = (2 << row) * P
            for ops, g in zip(cl, got):
                assert g == model(row, *ops), (fn, row, ops)
                v = [F.val(o) for o in ops]
                want = {"fe_sub": lambda: v[0] - v[1] + k, "fe_neg": lambda: k - v[0], "fe_neg_lazy": lambda: k - v[0], "fe_sub_sub_dbl": lambda: v[0] - v[1] - 2 * v[2] + k}[fn]()
                assert F.val(g) == want, (fn, row)
                if fn == "fe_neg_lazy":
                    assert all(1 <= x <= 1 << 30 for x in g[:13])
                else:
                    assert F.is_weak(g)


def test_add_double_and_the_carry_pass():
    for fn, op in (("fe_add", 2), ("fe_dbl", 3), ("fp_carry", 1)):
        cl = Cs.add_cases()[fn]
        assert cl, fn
        got = run(op, cl)
        for ops, g in zip(cl, got):
            if fn == "fp_carry":
                assert g == F.carry(list(ops[0]))
                assert F.val(g) % (1 << (F.TOPSHIFT + 32)) == F.val(ops[0]) % (1 << (F.TOPSHIFT + 32))
            else:
                assert g == (F.fe_add(*ops) if fn == "fe_add" else F.fe_dbl(*ops))
                assert F.val(g) == sum(F.val(o) for o in ops) * (2 if fn == "fe_dbl" else 1)
            assert F.is_weak(g)


def test_the_dense_memory_format_round_trips_below_p():
    cl = Cs.pack_cases()["below_p"]
    assert cl
    got = run(4, [(F.words12(v),) for v in cl])
    for v, g in zip(cl, got):
        assert g[:14] == F.unpack(v) == F.unpack_words(F.words12(v)), hex(v)
        assert g[14:] == F.words12(v) == F.pack(F.unpack(v)), hex(v)


INV_CHUNKS = 10


def _inversion(xs):
    got = run(5, [(F.unpack(x),) for x in xs])
    for x, g in zip(xs, got):
        limbs, _ = Cs.inversion_expected(x)
        assert g[:14] == limbs, ("fp_inv29_call", hex(x))
        assert F.val(g[14:]) == F.inv_fast(F.unpack(x)) and all(w <= F.M for w in g[14:]), ("fe_inv_fast", hex(x))
        if x:
            assert F.val(g[:14]) % P == pow(x, -1, P) and 4 * P < F.val(g[:14]) < 60 * P and F.is_weak(g[:14]), hex(x)
            assert F.val(g[14:]) == pow(x, -1, P) * pow(2, 812, P) % P
        else:
            assert g == [0] * 28


@pytest.mark.parametrize("chunk", range(INV_CHUNKS))
def test_inversion_of_plain_integers_limb_for_limb(chunk):
    fam = Cs._families()
    xs = [x for k in sorted(fam) for x in fam[k]][chunk::INV_CHUNKS]
    assert xs
    _inversion(xs)


def test_inversion_of_the_operands_that_need_all_27_iterations():
    ic = Cs.inversion_cases()
    for name, cl in ic.items():
        assert cl, "empty class %s" % name
    assert len(ic["needs_all_27"]) >= 32 and len(ic["wrong_after_26"]) >= 16 and (1 << 380) in ic["needs_all_27"] and 3 << 379 in ic["wrong_after_26"]
    _inversion(list(dict.fromkeys(ic["needs_all_27"] + ic["wrong_after_26"] + ic["search"] + ic["exact_switch"] + ic["zero"])))
