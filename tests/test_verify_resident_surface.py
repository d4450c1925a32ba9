"""The resident verification keys' surface without a GPU: include/zkmi355x.h, _lib.EXPORTS, _lib.VK_PROTOTYPES and the OCaml stubs name the same seven
calls with the same argument lists; argument checks come before the device; without a GPU every upload is ZK_ERR_HIP (no CPU fallback, so no handle
can exist) and a handle of 0 is ZK_ERR_HANDLE; the Python objects exist and refuse lists that do not match; the public options are untouched.
What the calls compute is held to the batched and the host verifiers on the GPU: tests/test_gpu_verify_resident.py, tests/test_gpu_subgroup_endo.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import option_cases
from oracle import pyref as P
from zukelang_amd import _lib
from zukelang_amd import pinocchio as PIN
from zukelang_amd.groth16 import Proof, ResidentVKey, VKey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
ZK_OK, ZK_ERR_ARG, ZK_ERR_HIP, ZK_ERR_HANDLE = 0, -1, -5, -7
# the issue's prototypes, parameter kinds in order
WANT = {
    "zk_groth16_vk_upload": ["u8p", "u8p", "size_t", "u8p", "u8p", "u64p"],
    "zk_pinocchio_vk_upload": ["u8p", "u8p", "size_t", "u64p"],
    "zk_vk_info": ["uint64_t", "intp", "u64p"],
    "zk_vk_free": ["uint64_t"],
    "zk_groth16_verify_resident": ["uint64_t", "u8p", "u8p", "uint32_t", "u8p", "i32p"],
    "zk_pinocchio_verify_resident": ["uint64_t", "u8p", "u8p", "uint32_t", "u8p", "i32p"],
    "zk_selftest_subgroup": ["int", "int", "u8p", "size_t", "u8p"],
}
HOST_CALLS = list(WANT)[:6]          # the self-test hook is the test suite's


def _header_params(name):
    body = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, body)
    assert m, "%s is not declared in include/zkmi355x.h" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _c_kind(param):
    p = re.sub(r"\[[^\]]*\]", "*", param)
    if "*" in p:
        return "u64p" if "uint64_t" in p else "i32p" if "int32_t" in p else "u8p" if "uint8_t" in p else "intp"
    return next(t for t in ("uint64_t", "uint32_t", "size_t", "int") if re.search(r"\b%s\b" % t, p))


def _gpu_present():
    return _lib.lib().zk_device_count() > 0


def test_header_exports_ctypes_and_ocaml_agree():
    kinds = {_lib._P8: "u8p", _lib._PH: "u64p", _lib._PI32: "i32p", C.POINTER(C.c_int): "intp", C.c_uint64: "uint64_t", C.c_uint32: "uint32_t",
             C.c_size_t: "size_t", C.c_int: "int"}
    word = lambda k: {"size_t": "uint64_t", "intp": "i32p"}.get(k, k)          # ctypes has ONE type for each pair on this ABI (c_size_t is c_uint64, c_int is c_int32)
    lib = _lib.lib()
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    for name in WANT:
        assert [_c_kind(p) for p in _header_params(name)] == WANT[name], name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert [word(kinds[a]) for a in _lib.VK_PROTOTYPES[name]] == [word(k) for k in WANT[name]], name
        assert getattr(lib, name).argtypes == _lib.VK_PROTOTYPES[name] and getattr(lib, name).restype is C.c_int
    assert set(_lib.VK_PROTOTYPES) == set(WANT)
    ml_kind = {"ocaml_bytes": "u8p", "ptr uint64_t": "u64p", "ptr int32_t": "i32p", "ptr int": "intp", "uint64_t": "uint64_t", "uint32_t": "uint32_t", "size_t": "size_t"}
    at = []
    for name in HOST_CALLS:
        m = re.search(r'fn\s+"%s"\s*\((.*?)returning int\)' % name, ml, flags=re.S)
        assert m, "%s is not bound in ocaml/mi355x.ml" % name
        args = [" ".join(a.split()) for a in m.group(1).split("@->")][:-1]
        assert [ml_kind[a] for a in args] == WANT[name], name
        at.append(m.start())
    assert at == sorted(at)                                                          # the stubs in the header's order
    assert [HEADER.index("int %s(" % n) for n in HOST_CALLS] == sorted(HEADER.index("int %s(" % n) for n in HOST_CALLS)
    # the section cites the reference lines the calls stand for
    section = HEADER[HEADER.index("verification keys resident on the device"):]
    for cite in ("groth16.ml:163-173", "pinocchio.ml:254-420", "curve.ml:199-212"):
        assert cite in section[:section.index("int zk_groth16_vk_upload")]
    # the protocol files: a Verifier beside verify_many, which still names its stub once
    for f, many, calls in (("groth16_mi355x.ml", "zk_groth16_verify_many", ("zk_groth16_vk_upload", "zk_groth16_verify_resident")),
                           ("pinocchio_mi355x.ml", "zk_pinocchio_verify_many", ("zk_pinocchio_vk_upload", "zk_pinocchio_verify_resident"))):
        src = re.sub(r"\(\*.*?\*\)", " ", open(os.path.join(ROOT, "ocaml", f)).read(), flags=re.S)
        assert len(re.findall(r"\b%s\b" % many, src)) == 1, f
        v = src[src.index("module Verifier = struct"):]
        for word in ("let create", "let verify_many", "let free", "vk_free") + calls:
            assert word in v, (f, word)


def _bufs():
    g1, g2 = P.g1_to_bytes(P.G1), P.g2_to_bytes(P.G2)
    return g1, g2, bytes(576), (C.c_uint8 * 8)(), (C.c_int32 * 8)()


u8 = lambda b: C.cast(C.c_char_p(b), _lib._P8)


def test_null_pointers_and_bad_selectors_are_argument_errors_before_the_device():
    lib = _lib.lib()
    g1, g2, gt, ok, st = _bufs()
    h = C.c_uint64(5)
    for hole in (0, 1, 3, 4, 5):
        args = [u8(gt), u8(g1), 1, u8(g2), u8(g2), C.byref(h)]
        args[hole] = None
        assert lib.zk_groth16_vk_upload(*args) == ZK_ERR_ARG, hole
    for hole in (0, 1, 3):
        args = [u8(g1 * 5), u8(g2 * 7), 1, C.byref(h)]
        args[hole] = None
        assert lib.zk_pinocchio_vk_upload(*args) == ZK_ERR_ARG, hole
    assert lib.zk_groth16_vk_upload(u8(gt), u8(g1), 8193, u8(g2), u8(g2), C.byref(h)) == ZK_ERR_ARG          # more public inputs than a resident key holds
    assert h.value == 5
    out = (C.c_uint8 * 1)(9)
    o8 = C.cast(out, _lib._P8)
    assert lib.zk_selftest_subgroup(0, 1, None, 1, o8) == ZK_ERR_ARG
    assert lib.zk_selftest_subgroup(0, 1, u8(g1), 1, None) == ZK_ERR_ARG
    assert lib.zk_selftest_subgroup(0, 1, u8(g1), 0, o8) == ZK_ERR_ARG           # no points
    assert lib.zk_selftest_subgroup(2, 1, u8(g1), 1, o8) == ZK_ERR_ARG           # no such group
    assert lib.zk_selftest_subgroup(-1, 0, u8(g1), 1, o8) == ZK_ERR_ARG
    assert lib.zk_selftest_subgroup(1, 2, u8(g2), 1, o8) == ZK_ERR_ARG           # no such method
    assert lib.zk_selftest_subgroup(1, -1, u8(g2), 1, o8) == ZK_ERR_ARG
    assert list(out) == [9]


def test_a_handle_of_zero_is_unknown():
    lib = _lib.lib()
    g1, g2, gt, ok, st = _bufs()
    okp = C.cast(ok, _lib._P8)
    pr, ppr = g1 + g2 + g1, g1 + g2 + g1 + g1 + g1 + g2 + g1 + g1
    for i in range(8):
        ok[i], st[i] = 7, 7
    assert lib.zk_groth16_verify_resident(0, u8(bytes(32)), u8(pr), 1, okp, st) == ZK_ERR_HANDLE
    assert lib.zk_pinocchio_verify_resident(0, u8(bytes(32)), u8(ppr), 1, okp, st) == ZK_ERR_HANDLE
    assert lib.zk_groth16_verify_resident(0x7FFFFFFFFFFFFFFF, None, None, 0, okp, st) == ZK_ERR_HANDLE          # count = 0 does not excuse an unknown handle
    assert lib.zk_vk_free(0) == ZK_ERR_HANDLE and lib.zk_vk_info(0, None, None) == ZK_ERR_HANDLE
    assert list(ok) == [7] * 8 and list(st) == [7] * 8


@pytest.mark.skipif(not _gpu_present(), reason="no handle can exist without a GPU")
def test_count_zero_is_ok_and_touches_nothing():
    lib = _lib.lib()
    g1, g2, gt, ok, st = _bufs()
    h = C.c_uint64(0)
    assert lib.zk_groth16_vk_upload(u8(gt), u8(g1), 1, u8(g2), u8(g2), C.byref(h)) == ZK_OK
    for i in range(8):
        ok[i], st[i] = 7, 7
    assert lib.zk_groth16_verify_resident(h, None, None, 0, C.cast(ok, _lib._P8), st) == ZK_OK
    assert lib.zk_groth16_verify_resident(h, None, None, 0, None, None) == ZK_OK
    assert list(ok) == [7] * 8 and list(st) == [7] * 8
    assert lib.zk_vk_free(h) == ZK_OK


@pytest.mark.skipif(_gpu_present(), reason="a GPU is visible: the calls run (tests/test_gpu_verify_resident.py, tests/test_gpu_subgroup_endo.py)")
def test_without_a_gpu_every_upload_is_a_hip_error():
    lib = _lib.lib()
    g1, g2, gt, ok, st = _bufs()
    h = C.c_uint64(0)
    assert lib.zk_groth16_vk_upload(u8(gt), u8(g1), 1, u8(g2), u8(g2), C.byref(h)) == ZK_ERR_HIP
    assert lib.zk_groth16_vk_upload(u8(gt), None, 0, u8(g2), u8(g2), C.byref(h)) == ZK_ERR_HIP                 # n_io = 0 is legal
    assert lib.zk_pinocchio_vk_upload(u8(g1 * 5), u8(g2 * 7), 1, C.byref(h)) == ZK_ERR_HIP
    assert h.value == 0
    out = (C.c_uint8 * 1)()
    assert lib.zk_selftest_subgroup(0, 1, u8(g1), 1, C.cast(out, _lib._P8)) == ZK_ERR_HIP
    vk = VKey(g1, np.frombuffer(g1 * 2, dtype=np.uint8), g2, g2, g2, bytes(576))
    with pytest.raises(_lib.ZkError) as e:
        vk.resident()
    assert e.value.code == ZK_ERR_HIP
    with pytest.raises(_lib.ZkError) as e:
        PIN.VKey(np.frombuffer(g1 * 5, dtype=np.uint8), np.frombuffer(g2 * 7, dtype=np.uint8)).resident()
    assert e.value.code == ZK_ERR_HIP


def test_python_objects_exist_and_refuse_mismatched_lengths():
    g1, g2 = P.g1_to_bytes(P.G1), P.g2_to_bytes(P.G2)
    assert callable(VKey.resident) and callable(PIN.VKey.resident)
    with pytest.raises(ValueError):
        VKey(g1, np.frombuffer(g1 * 2, dtype=np.uint8), g2, g2, g2, bytes(575)).resident()          # ab is not 576 bytes
    with pytest.raises(AssertionError):
        PIN.VKey(np.frombuffer(g1 * 5, dtype=np.uint8), np.frombuffer(g2 * 8, dtype=np.uint8)).resident()      # the key maps' domains differ
    # the object's own checks come before the library: a made-up handle is never handed over
    pr = Proof(g1, g2, g1)
    rv = ResidentVKey(0x7FFFFFFFFFFFFFFF, 2, lambda p: bytes(p.a) + bytes(p.b) + bytes(p.c), 384, "zk_groth16_verify_resident")
    with pytest.raises(ValueError):
        rv.verify_many([[1, 2]], [pr, pr])                        # one list of inputs, two proofs
    with pytest.raises(AssertionError):
        rv.verify_many([[1, 2, 3]], [pr])                         # three inputs against a key of two
    with pytest.raises(ValueError):
        rv.verify_many([[1, 2]], [Proof(g1, g2, g1[:95])])        # a proof of 383 bytes
    with pytest.raises(_lib.ZkError) as e:
        rv.verify_many([[1, 2]], [pr])                            # the handle is unknown to the library
    assert e.value.code == ZK_ERR_HANDLE
    rv.handle = 0                                                 # as after close(): nothing to free
    with pytest.raises(ValueError):
        rv.verify_many([[1, 2]], [pr])
    with ResidentVKey(0, 0, bytes, 960, "zk_pinocchio_verify_resident") as closed:
        assert closed.handle == 0


def test_public_options_are_unchanged():
    names = option_cases.public_options()
    assert len(names) == 28 and sorted(names) == sorted(option_cases.CASES)
    new = open(os.path.join(ROOT, "zukelang_amd", "csrc", "verify_resident.hip")).read()
    assert not option_cases.OPTION_READ.search(new)          # the resident path reads no knob
