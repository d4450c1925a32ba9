"""zk_selftest_fr and zk_selftest_fr29 without a GPU: include/zkmi355x.h, _lib.EXPORTS and _lib.FR_PROTOTYPES name the same calls with the same
argument lists; every refusal comes before the device, each limb rule of the raw-limb hook on its own; a valid call is ZK_ERR_HIP here (no CPU
fallback).  What the hooks compute: tests/test_gpu_fr_field.py."""
import ctypes as C
import os
import re

import pytest

import fr29_model as F
from zukelang_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
ZK_OK, ZK_ERR_ARG, ZK_ERR_HIP = 0, -1, -5
R, L = F.R, F.L
P32 = C.POINTER(C.c_uint32)
WANT = {"zk_selftest_fr": ["int", "u8p", "u8p", "size_t", "u8p"], "zk_selftest_fr29": ["int", "u32p", "size_t", "u32p"]}

u8 = lambda b: C.cast(C.c_char_p(b), _lib._P8)
le32 = lambda x: int(x).to_bytes(32, "little")
GOOD = lambda: ZK_OK if _lib.lib().zk_device_count() > 0 else ZK_ERR_HIP          # what a call that passes every argument check returns


def words(*values):
    """u | v | w slots of 9 limbs each, one lane per triple"""
    flat = [x for l in values for x in l]
    assert len(flat) % (3 * L) == 0
    return (C.c_uint32 * len(flat))(*flat)


def test_header_exports_and_ctypes_agree():
    body = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    kinds = {_lib._P8: "u8p", P32: "u32p", C.c_size_t: "size_t", C.c_int: "int"}
    lib = _lib.lib()
    for name, want in WANT.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, body)
        assert m, "%s is not declared in include/zkmi355x.h" % name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        got = [("u8p" if "uint8_t" in p else "u32p") if "*" in p else next(t for t in ("size_t", "int") if re.search(r"\b%s\b" % t, p)) for p in params]
        assert got == want
        assert all(("const" in p) == ("*" in p) for p in params[:-1]) and "const" not in params[-1]          # operands are read, out is written
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert [kinds[a] for a in _lib.FR_PROTOTYPES[name]] == want
        assert getattr(lib, name).argtypes == _lib.FR_PROTOTYPES[name] and getattr(lib, name).restype is C.c_int
    assert set(_lib.FR_PROTOTYPES) == set(WANT)
    assert (ZK_ERR_ARG, ZK_ERR_HIP) == tuple(int(re.search(r"#define %s \((-?\d+)\)" % n, HEADER).group(1)) for n in ("ZK_ERR_ARG", "ZK_ERR_HIP"))
    # the header's comment names every output and op
    comment = HEADER[HEADER.index("The scalar field on 8 x 32-bit words"):HEADER.index("int zk_selftest_fr29")]
    for k in range(14):
        assert re.search(r"\b%d\b" % k, comment), k
    for op in range(6):
        assert "op %d" % op in comment


def test_the_word_hook_refuses_before_the_device():
    call = _lib.lib().zk_selftest_fr
    a, b = le32(5), le32(R - 1)
    out = C.create_string_buffer(b"\x09" * (14 * 32 * 2), 14 * 32 * 2)
    o8 = C.cast(out, _lib._P8)
    assert call(0, None, u8(b), 1, o8) == ZK_ERR_ARG
    assert call(0, u8(a), None, 1, o8) == ZK_ERR_ARG                 # op 0 reads b
    assert call(0, u8(a), u8(b), 1, None) == ZK_ERR_ARG
    assert call(0, u8(a), u8(b), 0, o8) == ZK_ERR_ARG                # no operands
    assert call(1, None, None, 1, o8) == ZK_ERR_ARG
    assert call(1, u8(a), None, 0, o8) == ZK_ERR_ARG
    assert call(1, u8(a), None, 1, None) == ZK_ERR_ARG
    for bad_op in (2, -1, 99):
        assert call(bad_op, u8(a), u8(b), 1, o8) == ZK_ERR_ARG
    # an operand >= r, on either side, in either of two lanes: r itself, r + 1, 2^256 - 1, r with its top word incremented
    for big in (R, R + 1, (1 << 256) - 1, R + (1 << 224)):
        assert call(0, u8(le32(big)), u8(b), 1, o8) == ZK_ERR_ARG, hex(big)
        assert call(0, u8(a), u8(le32(big)), 1, o8) == ZK_ERR_ARG, hex(big)
        assert call(0, u8(a + le32(big)), u8(b + b), 2, o8) == ZK_ERR_ARG, hex(big)
        assert call(0, u8(a + a), u8(b + le32(big)), 2, o8) == ZK_ERR_ARG, hex(big)
    assert out.raw == b"\x09" * (14 * 32 * 2)
    # what is not refused: r - 1 on both sides, and for op 1 any 256 bits with no b at all
    assert call(0, u8(le32(R - 1)), u8(le32(R - 1)), 1, o8) == GOOD()
    assert call(1, u8(le32((1 << 256) - 1)), None, 1, o8) == GOOD()


def test_the_limb_hook_refuses_each_limb_rule_on_its_own_before_the_device():
    call = _lib.lib().zk_selftest_fr29
    good_u, good_v, good_w = F.unpack(63 * R + 5), F.unpack(24 * R - 1), F.unpack(R - 1)
    out = (C.c_uint32 * 90)(*([0x09090909] * 90))
    assert call(3, None, 1, out) == ZK_ERR_ARG
    assert call(3, words(good_u, good_v, good_w), 1, None) == ZK_ERR_ARG
    assert call(3, words(good_u, good_v, good_w), 0, out) == ZK_ERR_ARG
    for bad_op in (6, -1, 99):
        assert call(bad_op, words(good_u, good_v, good_w), 1, out) == ZK_ERR_ARG

    def with_limb(l, k, x):
        r = list(l)
        r[k] = x
        return r
    for k in range(L - 1):
        # limbs 0..7 of u and v: 2^29 + 7 is the last admitted value
        hi = with_limb(good_u, k, F.WEAK + 1)
        for op in range(5):
            assert call(op, words(hi, good_v, good_w), 1, out) == ZK_ERR_ARG, (op, k)
        for op in (2, 3, 4):
            assert call(op, words(good_u, with_limb(good_v, k, F.WEAK + 1), good_w), 1, out) == ZK_ERR_ARG, (op, k)
            assert call(op, words(good_u, with_limb(good_v, k, 0xFFFFFFFF), good_w), 1, out) == ZK_ERR_ARG, (op, k)
        # limbs 0..7 of w: exact, 2^29 - 1 is the last admitted value
        for op in (3, 4):
            assert call(op, words(good_u, good_v, with_limb([0] * L, k, F.M + 1)), 1, out) == ZK_ERR_ARG, (op, k)
    # the top limb: that of 64 r is the last admitted value
    for op in range(5):
        assert call(op, words(with_limb(good_u, L - 1, F.TOP_64R + 1), good_v, good_w), 1, out) == ZK_ERR_ARG, op
    for op in (2, 3, 4):
        assert call(op, words(good_u, with_limb(good_v, L - 1, F.TOP_64R + 1), good_w), 1, out) == ZK_ERR_ARG, op
    # w >= r: r itself, r + 1, r with each limb incremented where that keeps the limb exact, a top limb above r's
    for op in (3, 4):
        for big in [F.unpack(R), F.unpack(R + 1), with_limb(F.MOD, L - 1, F.MOD[L - 1] + 1)] + [with_limb(F.MOD, k, F.MOD[k] + 1) for k in range(L - 1) if F.MOD[k] < F.M]:
            assert call(op, words(good_u, good_v, big), 1, out) == ZK_ERR_ARG, (op, big)
        # the second lane is checked too
        assert call(op, words(good_u, good_v, good_w, good_u, good_v, F.unpack(R)), 2, out) == ZK_ERR_ARG
        assert call(op, words(good_u, good_v, good_w, with_limb(good_u, 3, F.WEAK + 1), good_v, good_w), 2, out) == ZK_ERR_ARG
    assert list(out) == [0x09090909] * 90
    # what is not refused: every limb at its last admitted value; operands an op does not read; any 8 words for op 5
    edge = [F.WEAK] * (L - 1) + [F.TOP_64R - 1]
    assert F.val(edge) < 64 * R
    top_w = F.unpack(R - 1)
    junk = [0xFFFFFFFF] * L
    for op in (0, 1):
        assert call(op, words(edge, junk, junk), 1, out) == GOOD(), op
    assert call(2, words(F.unpack(R - 1), with_limb([0] * L, L - 1, F.TOP_64R), junk), 1, out) == GOOD()          # the top limb of 64 r itself, below 64 r
    for op in (3, 4):
        for k in range(L - 1):          # r with limb k decremented is below r
            if F.MOD[k]:
                assert call(op, words(good_u, good_v, with_limb(F.MOD, k, F.MOD[k] - 1)), 1, out) == GOOD(), (op, k)
        assert call(op, words(good_u, good_v, top_w), 1, out) == GOOD(), op
    assert call(5, words(junk, junk, junk), 1, out) == GOOD()


@pytest.mark.skipif(_lib.lib().zk_device_count() > 0, reason="a GPU is visible: the calls run (tests/test_gpu_fr_field.py)")
def test_without_a_gpu_a_valid_call_is_a_hip_error():
    lib = _lib.lib()
    out = C.create_string_buffer(14 * 32)
    assert lib.zk_selftest_fr(0, u8(le32(3)), u8(le32(R - 1)), 1, C.cast(out, _lib._P8)) == ZK_ERR_HIP
    assert lib.zk_selftest_fr(1, u8(le32(R)), None, 1, C.cast(out, _lib._P8)) == ZK_ERR_HIP
    o32 = (C.c_uint32 * 45)()
    for op in range(6):
        assert lib.zk_selftest_fr29(op, words(F.unpack(38 * R - 1), F.unpack(24 * R - 1), F.unpack(R - 1)), 1, o32) == ZK_ERR_HIP, op
    assert b"no HIP device" in lib.zk_last_error()
