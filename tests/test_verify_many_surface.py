"""The batched verifiers' surface without a GPU: include/zkmi355x.h, _lib.EXPORTS, the ctypes prototypes and the OCaml stubs name the same calls with
the same argument lists; argument checks come before the device (a null pointer is ZK_ERR_ARG, count = 0 is ZK_OK and touches nothing); without a
GPU every call is ZK_ERR_HIP (there is no CPU fallback); the Python functions exist and refuse lists that do not match; the public options are untouched.
What the calls compute is held to the host verifiers on the GPU: tests/test_gpu_pairing.py, tests/test_gpu_verify_many.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import option_cases
from oracle import pyref as P
from zukelang_amd import _lib, curve
from zukelang_amd import pinocchio as PIN
from zukelang_amd.groth16 import Groth16, Proof, VKey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
NEW = ["zk_pairing_product_many", "zk_groth16_verify_many", "zk_pinocchio_verify_many", "zk_selftest_fp12"]
ZK_OK, ZK_ERR_ARG, ZK_ERR_HIP = 0, -1, -5
# the issue's prototypes, parameter kinds in order
WANT = {
    "zk_pairing_product_many": ["u8p", "u8p", "u64p", "uint32_t", "u8p"],
    "zk_groth16_verify_many": ["u8p", "u8p", "size_t", "u8p", "u8p", "u8p", "u8p", "uint32_t", "u8p", "i32p"],
    "zk_pinocchio_verify_many": ["u8p", "u8p", "size_t", "u8p", "u8p", "uint32_t", "u8p", "i32p"],
    "zk_selftest_fp12": ["int", "u8p", "u8p", "size_t", "u8p"],
}


def _header_params(name):
    body = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, body)
    assert m, "%s is not declared in include/zkmi355x.h" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _c_kind(param):
    p = re.sub(r"\[[^\]]*\]", "*", param)
    if "*" in p:
        return "u64p" if "uint64_t" in p else "i32p" if "int32_t" in p else "u8p"
    return next(t for t in ("uint32_t", "size_t", "int") if re.search(r"\b%s\b" % t, p))


def _gpu_present():
    return _lib.lib().zk_device_count() > 0


def test_header_exports_ctypes_and_ocaml_agree():
    kinds = {_lib._P8: "u8p", _lib._PH: "u64p", _lib._PI32: "i32p", C.c_uint32: "uint32_t", C.c_size_t: "size_t", C.c_int: "int"}
    lib = _lib.lib()
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    for name in NEW:
        assert [_c_kind(p) for p in _header_params(name)] == WANT[name], name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert [kinds[a] for a in _lib.VERIFY_PROTOTYPES[name]] == WANT[name], name
        assert getattr(lib, name).argtypes == _lib.VERIFY_PROTOTYPES[name] and getattr(lib, name).restype is C.c_int
    assert set(_lib.VERIFY_PROTOTYPES) == set(NEW)
    ml_kind = {"ocaml_bytes": "u8p", "ptr uint64_t": "u64p", "ptr int32_t": "i32p", "uint32_t": "uint32_t", "size_t": "size_t"}
    for name in NEW[:3]:          # the three calls a host makes; the self-test hook is the test suite's
        m = re.search(r'fn\s+"%s"\s*\((.*?)returning int\)' % name, ml, flags=re.S)
        assert m, "%s is not bound in ocaml/mi355x.ml" % name
        args = [" ".join(a.split()) for a in m.group(1).split("@->")][:-1]
        assert [ml_kind[a] for a in args] == WANT[name], name
    # the comments cite the reference lines the calls stand for
    for cite in ("curve.mli:46-54", "groth16.ml:163-173", "pinocchio.ml:254-420"):
        assert cite in HEADER[HEADER.index("the same three on the device"):]
    # the protocol files call the stubs once per list of proofs
    for f, sym in (("groth16_mi355x.ml", "zk_groth16_verify_many"), ("pinocchio_mi355x.ml", "zk_pinocchio_verify_many")):
        src = open(os.path.join(ROOT, "ocaml", f)).read()
        assert "verify_many" in src and len(re.findall(r"\b%s\b" % sym, re.sub(r"\(\*.*?\*\)", " ", src, flags=re.S))) == 1, f


def _bufs():
    g1, g2 = P.g1_to_bytes(P.G1), P.g2_to_bytes(P.G2)
    return g1, g2, bytes(576), (C.c_uint8 * 8)(), (C.c_int32 * 8)()


def test_null_pointers_are_argument_errors_before_the_device():
    lib = _lib.lib()
    g1, g2, gt, ok, st = _bufs()
    one = (C.c_uint64 * 1)(1)
    out = C.create_string_buffer(576)
    u8 = lambda b: C.cast(C.c_char_p(b), _lib._P8)
    o8 = C.cast(out, _lib._P8)
    assert lib.zk_pairing_product_many(u8(g1), u8(g2), None, 1, o8) == ZK_ERR_ARG
    assert lib.zk_pairing_product_many(u8(g1), u8(g2), one, 1, None) == ZK_ERR_ARG
    assert lib.zk_pairing_product_many(None, u8(g2), one, 1, o8) == ZK_ERR_ARG
    assert lib.zk_pairing_product_many(u8(g1), None, one, 1, o8) == ZK_ERR_ARG
    pr, sc = g1 + g2 + g1, bytes(32)
    okp = C.cast(ok, _lib._P8)
    for hole in range(9):          # every pointer but status
        args = [u8(gt), u8(g1), 1, u8(g2), u8(g2), u8(sc), u8(pr), 1, okp, st]
        if hole in (2, 7):
            continue
        args[hole] = None
        assert lib.zk_groth16_verify_many(*args) == ZK_ERR_ARG, hole
    vk1, vk2, ppr = g1 * 5, g2 * 7, (g1 + g2 + g1 + g1 + g1 + g2 + g1 + g1)
    for hole in (0, 1, 3, 4, 6):
        args = [u8(vk1), u8(vk2), 1, u8(sc), u8(ppr), 1, okp, st]
        args[hole] = None
        assert lib.zk_pinocchio_verify_many(*args) == ZK_ERR_ARG, hole
    assert lib.zk_selftest_fp12(0, None, u8(gt), 1, o8) == ZK_ERR_ARG
    assert lib.zk_selftest_fp12(0, u8(gt), None, 1, o8) == ZK_ERR_ARG          # op 0 reads b
    assert lib.zk_selftest_fp12(3, u8(gt), u8(gt), 1, None) == ZK_ERR_ARG
    assert lib.zk_selftest_fp12(8, u8(gt), u8(gt), 1, o8) == ZK_ERR_ARG        # no such operation
    assert lib.zk_selftest_fp12(3, u8(gt), u8(gt), 0, o8) == ZK_ERR_ARG        # no elements


def test_count_zero_is_ok_and_touches_nothing():
    lib = _lib.lib()
    g1, g2, gt, ok, st = _bufs()
    u8 = lambda b: C.cast(C.c_char_p(b), _lib._P8)
    for i in range(8):
        ok[i], st[i] = 7, 7
    out = C.create_string_buffer(b"\x55" * 576, 576)
    assert lib.zk_pairing_product_many(None, None, None, 0, C.cast(out, _lib._P8)) == ZK_OK and out.raw == b"\x55" * 576
    assert lib.zk_groth16_verify_many(u8(gt), u8(g1), 1, u8(g2), u8(g2), None, None, 0, C.cast(ok, _lib._P8), st) == ZK_OK
    assert lib.zk_pinocchio_verify_many(u8(g1 * 5), u8(g2 * 7), 1, None, None, 0, C.cast(ok, _lib._P8), st) == ZK_OK
    assert list(ok) == [7] * 8 and list(st) == [7] * 8


@pytest.mark.skipif(_gpu_present(), reason="a GPU is visible: the calls run (tests/test_gpu_pairing.py, tests/test_gpu_verify_many.py)")
def test_without_a_gpu_every_call_is_a_hip_error():
    lib = _lib.lib()
    g1, g2, gt, ok, st = _bufs()
    u8 = lambda b: C.cast(C.c_char_p(b), _lib._P8)
    out = C.create_string_buffer(576)
    one = (C.c_uint64 * 1)(1)
    assert lib.zk_pairing_product_many(u8(g1), u8(g2), one, 1, C.cast(out, _lib._P8)) == ZK_ERR_HIP
    assert lib.zk_groth16_verify_many(u8(gt), u8(g1), 1, u8(g2), u8(g2), u8(bytes(32)), u8(g1 + g2 + g1), 1, C.cast(ok, _lib._P8), st) == ZK_ERR_HIP
    assert lib.zk_pinocchio_verify_many(u8(g1 * 5), u8(g2 * 7), 1, u8(bytes(32)), u8(g1 + g2 + g1 + g1 + g1 + g2 + g1 + g1), 1, C.cast(ok, _lib._P8), st) == ZK_ERR_HIP
    assert lib.zk_selftest_fp12(3, u8(gt), None, 1, C.cast(out, _lib._P8)) == ZK_ERR_HIP
    with pytest.raises(_lib.ZkError) as e:
        curve.Pairing.product_many(g1, g2, [1])
    assert e.value.code == ZK_ERR_HIP


def test_python_functions_exist_and_refuse_mismatched_lengths():
    g1, g2 = P.g1_to_bytes(P.G1), P.g2_to_bytes(P.G2)
    with pytest.raises(ValueError):
        curve.Pairing.product_many(g1 * 2, g2 * 2, [1])           # two pairs, lengths say one
    with pytest.raises(ValueError):
        curve.Pairing.product_many(g1, g2 * 2, [1])
    assert curve.Pairing.product_many(b"", b"", []) == []
    vk = VKey(g1, np.frombuffer(g1 * 2, dtype=np.uint8), g2, g2, g2, bytes(576))
    pr = Proof(g1, g2, g1)
    with pytest.raises(ValueError):
        Groth16.verify_many([[1, 2]], vk, [pr, pr])                # one list of inputs, two proofs
    with pytest.raises(AssertionError):
        Groth16.verify_many([[1, 2, 3]], vk, [pr])                 # three inputs against a key of two
    pvk = PIN.VKey(np.frombuffer(g1 * 5, dtype=np.uint8), np.frombuffer(g2 * 7, dtype=np.uint8))
    ppr = PIN.Proof(g1, g2, g1, g1, g1, g2, g1, g1)
    for cls in (PIN.ZK, PIN.NonZK):
        with pytest.raises(ValueError):
            cls.verify_many([[1]], pvk, [ppr, ppr])
        with pytest.raises(AssertionError):
            cls.verify_many([[1, 2]], pvk, [ppr])
    assert PIN.verify_many is not None and Groth16.verify_many([], vk, []) == [] and PIN.ZK.verify_many([], pvk, []) == []


def test_public_options_are_unchanged():
    names = option_cases.public_options()
    assert len(names) == 28 and sorted(names) == sorted(option_cases.CASES)
    assert not [n for n in names if "VERIFY" in n or "PAIRING" in n]
    dev = open(os.path.join(ROOT, "zukelang_amd", "csrc", "pairing_dev.hip")).read() + open(os.path.join(ROOT, "zukelang_amd", "csrc", "pairing_tower.cuh")).read()
    assert not option_cases.OPTION_READ.search(dev)          # the batched verifiers read no knob
