"""zk_selftest_fp29 without a GPU: include/zkmi355x.h, _lib.EXPORTS and _lib.FP29_PROTOTYPES name the same call with the same argument list; every
refusal comes before the device, each limb rule on its own and each op's top-limb bound at its last admitted value; a valid call is ZK_ERR_HIP here
(no CPU fallback).  What the hook computes: tests/test_gpu_fp29.py."""
import ctypes as C
import os
import re

import pytest

import fp29_cases as Cs
import fp29_model as F
from zukelang_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
ZK_OK, ZK_ERR_ARG, ZK_ERR_HIP = 0, -1, -5
P, L = F.P, F.L
P32 = C.POINTER(C.c_uint32)
GOOD = lambda: ZK_OK if _lib.lib().zk_device_count() > 0 else ZK_ERR_HIP          # what a call that passes every argument check returns

OP_CANON, OP_CARRY, OP_ADD, OP_DBL, OP_PACK, OP_INV, OP_ZERO, OP_ROWS = 0, 1, 2, 3, 4, 5, 8, 16
SUB, NEG, NEG_LAZY, SSD = (lambda k: 16 + k), (lambda k: 32 + k), (lambda k: 48 + k), (lambda k: 64 + k)
VALID_OPS = [0, 1, 2, 3, 4, 5, 8, 9, 10] + [SUB(k) for k in Cs.SUB_ROWS] + [NEG(k) for k in Cs.NEG_ROWS] + [NEG_LAZY(k) for k in Cs.NEG_ROWS] + [SSD(k) for k in Cs.SSD_ROWS]


def out_words(op):
    return 26 if op == OP_PACK else 28 if op == OP_INV else 1 if op in (8, 9, 10) else 14


def bounds_of(op):
    """the value bound of each slot the op reads with the weak-limb rule (None: the slot is not read, or has a rule of its own)"""
    if op == OP_CANON:
        return [F.FP_MAX_BOUND, None, None]
    if op in (OP_ADD,):
        return [64, 64, None]
    if op == OP_DBL:
        return [64, None, None]
    if op in (8, 9, 10):
        return [Cs.ZERO_BOUNDS[op - 8], None, None]
    if op >= 64:
        b = Cs.row_bound(op - 64 - 1)
        return [64, b, b]
    if op >= 32:
        return [Cs.row_bound((op - 32) % 16), None, None]
    if op >= 16:
        return [64, Cs.row_bound(op - 16), None]
    return [None, None, None]


def slots(*lanes):
    """lanes of (a, b, c), each 14 limbs -> 48 words per lane"""
    flat = []
    for lane in lanes:
        for l in lane:
            flat += list(l) + [0, 0]
    assert len(flat) % 48 == 0
    return (C.c_uint32 * len(flat))(*flat)


def with_limb(l, k, x):
    r = list(l)
    r[k] = x
    return r


ZERO = [0] * L
JUNK = [0xFFFFFFFF] * L


def test_header_exports_and_ctypes_agree():
    body = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"\bint\s+zk_selftest_fp29\s*\(([^)]*)\)\s*;", body)
    assert m, "zk_selftest_fp29 is not declared in include/zkmi355x.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["int op", "const uint32_t* operands", "size_t n", "uint32_t* out"]
    lib = _lib.lib()
    assert "zk_selftest_fp29" in _lib.EXPORTS and hasattr(lib, "zk_selftest_fp29")
    assert _lib.FP29_PROTOTYPES == {"zk_selftest_fp29": [C.c_int, P32, C.c_size_t, P32]}
    assert lib.zk_selftest_fp29.argtypes == _lib.FP29_PROTOTYPES["zk_selftest_fp29"] and lib.zk_selftest_fp29.restype is C.c_int
    comment = HEADER[HEADER.index("The base field under its products, on bare limbs"):HEADER.index("int zk_selftest_fp29")]
    for op in (0, 1, 2, 3, 4, 5):
        assert "op %d " % op in comment
    for text in ("op 8, 9, 10", "op 16 + k, k = 0..11", "op 32 + k, k = 0..12", "op 48 + k, k = 0..12", "op 64 + k, k = 1..11", "fp_canon_call", "fp_inv29_call", "fe_inv_fast",
                 "fp_is_zero_mod_p_inline", "fe_sub_sub_dbl", "fe_neg_lazy", "fp_carry", "fp_unpack", "fp_pack", "ZK_ERR_ARG"):
        assert text in comment, text
    # the op numbers of the header are those of the shared device header
    cuh = open(os.path.join(F.CSRC, "fp29_selftest.cuh")).read()
    for name, v in (("FP29_OP_CANON", 0), ("FP29_OP_CARRY", 1), ("FP29_OP_ADD", 2), ("FP29_OP_DBL", 3), ("FP29_OP_PACK", 4), ("FP29_OP_INV", 5), ("FP29_OP_ZERO", 8), ("FP29_OP_ROWS", 16)):
        assert re.search(r"\b%s = %d\b" % (name, v), cuh), name
    assert tuple(int(re.search(r"FP29_ZERO_B%d = (\d+)" % i, cuh).group(1)) for i in range(3)) == Cs.ZERO_BOUNDS


def test_null_pointers_no_operands_and_unknown_ops_are_refused():
    call = _lib.lib().zk_selftest_fp29
    out = (C.c_uint32 * 28)(*([0x09090909] * 28))
    ok = slots((ZERO, ZERO, ZERO))
    for op in VALID_OPS:
        assert call(op, None, 1, out) == ZK_ERR_ARG
        assert call(op, ok, 1, None) == ZK_ERR_ARG
        assert call(op, ok, 0, out) == ZK_ERR_ARG
        assert call(op, ok, 1 << 24, out) == ZK_ERR_ARG          # n >= 2^24 is refused before any operand is read
    for bad in [-1, 6, 7, 11, 12, 15, SUB(12), SUB(15), NEG(13), NEG_LAZY(13), NEG_LAZY(15), SSD(0), SSD(12), 80, 96, 1 << 20]:
        assert bad not in VALID_OPS and call(bad, ok, 1, out) == ZK_ERR_ARG, bad
    assert list(out) == [0x09090909] * 28


@pytest.mark.parametrize("op", [o for o in VALID_OPS if any(bounds_of(o))])
def test_each_limb_rule_on_its_own_and_every_top_limb_at_its_last_admitted_value(op):
    call = _lib.lib().zk_selftest_fp29
    out = (C.c_uint32 * 28)(*([0x09090909] * 28))
    bounds = bounds_of(op)
    good = [F.unpack(b * P - 1) if b else JUNK for b in bounds]          # slots that are not read hold junk
    for s, b in enumerate(bounds):
        if b is None:
            continue
        top = F.top_limb_of(b)
        assert good[s][L - 1] == top
        for k in (0, 5, 12):
            for x in (F.WEAK + 1, 0xFFFFFFFF):
                lane = list(good)
                lane[s] = with_limb(good[s], k, x)
                assert call(op, slots(lane), 1, out) == ZK_ERR_ARG, (s, k)
        lane = list(good)
        lane[s] = with_limb(good[s], L - 1, top + 1)
        assert call(op, slots(lane), 1, out) == ZK_ERR_ARG, s
        assert call(op, slots(good, lane), 2, out) == ZK_ERR_ARG, s          # the second lane is checked too
    assert list(out) == [0x09090909] * 28
    # what is not refused: every limb at its last admitted value
    edge = [Cs.max_weak(b) if b else JUNK for b in bounds]
    assert all(e is not None for e in edge)
    assert call(op, slots(good), 1, out) == GOOD()
    assert call(op, slots([with_limb([F.WEAK] * L, L - 1, F.top_limb_of(b)) if b else JUNK for b in bounds]), 1, out) == GOOD()


def test_the_ops_with_rules_of_their_own():
    call = _lib.lib().zk_selftest_fp29
    out = (C.c_uint32 * 28)(*([0x09090909] * 28))
    # op 5: exact limbs and a value below p
    for big in [F.unpack(P), F.unpack(P + 1), with_limb(F.MOD, L - 1, F.MOD[L - 1] + 1)] + [with_limb(F.MOD, k, F.MOD[k] + 1) for k in range(L - 1) if F.MOD[k] < F.M]:
        assert call(OP_INV, slots((big, JUNK, JUNK)), 1, out) == ZK_ERR_ARG
    for k in range(L - 1):
        assert call(OP_INV, slots((with_limb(ZERO, k, F.M + 1), JUNK, JUNK)), 1, out) == ZK_ERR_ARG, k
        assert call(OP_INV, slots((F.unpack(5), JUNK, JUNK), (with_limb(ZERO, k, F.M + 1), JUNK, JUNK)), 2, out) == ZK_ERR_ARG, k
    # op 4: 12 dense words below p
    for big in (P, P + 1, (1 << 384) - 1, P + (1 << 352)):
        assert call(OP_PACK, slots((F.words12(big) + [0, 0], JUNK, JUNK)), 1, out) == ZK_ERR_ARG
    assert list(out) == [0x09090909] * 28
    assert call(OP_INV, slots((F.unpack(P - 1), JUNK, JUNK)), 1, out) == GOOD()
    for k in range(L):
        if F.MOD[k]:
            assert call(OP_INV, slots((with_limb(F.MOD, k, F.MOD[k] - 1), JUNK, JUNK)), 1, out) == GOOD(), k
    assert call(OP_PACK, slots((F.words12(P - 1) + [0xFFFFFFFF] * 2, JUNK, JUNK)), 1, out) == GOOD()
    assert call(OP_CARRY, slots((JUNK, JUNK, JUNK)), 1, out) == GOOD()          # fp_carry: any 14 words


@pytest.mark.skipif(_lib.lib().zk_device_count() > 0, reason="a GPU is visible: the calls run (tests/test_gpu_fp29.py)")
def test_without_a_gpu_a_valid_call_is_a_hip_error():
    lib = _lib.lib()
    out = (C.c_uint32 * 28)()
    for op in VALID_OPS:
        assert lib.zk_selftest_fp29(op, slots((ZERO, ZERO, ZERO)), 1, out) == ZK_ERR_HIP, op
    assert b"no HIP device" in lib.zk_last_error()
