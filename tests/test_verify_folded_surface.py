"""The folded verifier's surface without a GPU: include/zkmi355x.h, _lib.EXPORTS, _lib.FOLD_PROTOTYPES and the OCaml stubs name the same two calls with
the same argument lists; what needs no handle is refused before the handle table or the device is looked at (a null pointer, a zero rho, too many
proofs); a handle of 0 is ZK_ERR_HANDLE and, without a GPU, any other is ZK_ERR_HIP (no handle can exist, and nothing falls back to the CPU); the Python
object refuses what it can refuse itself, and verify_many without fold_first hands the library exactly what it handed it before.
What the calls compute is held to pyref and the host pairing on the GPU: tests/test_gpu_verify_folded.py."""
import ctypes as C
import os
import re

import pytest

from oracle import pyref as P
from zukelang_amd import _lib
from zukelang_amd import groth16 as G
from zukelang_amd.groth16 import Proof, ResidentVKey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
ZK_OK, ZK_ERR_ARG, ZK_ERR_HIP, ZK_ERR_HANDLE = 0, -1, -5, -7
# the issue's prototypes, parameter kinds in order
WANT = {
    "zk_groth16_verify_folded": ["uint64_t", "u8p", "u8p", "u8p", "uint32_t", "intp", "i32p"],
    "zk_selftest_groth16_fold": ["uint64_t", "u8p", "u8p", "u8p", "uint32_t", "u8p", "u8p", "u8p", "u8p", "i32p"],
}
u8 = lambda b: C.cast(C.c_char_p(b), _lib._P8)


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
    kinds = {_lib._P8: "u8p", _lib._PI32: "i32p", C.c_uint64: "uint64_t", C.c_uint32: "uint32_t"}
    word = lambda k: "i32p" if k == "intp" else k          # ctypes has ONE type for int and int32_t on this ABI
    lib = _lib.lib()
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    ml_kind = {"ocaml_bytes": "u8p", "ptr int32_t": "i32p", "ptr int": "intp", "uint64_t": "uint64_t", "uint32_t": "uint32_t"}
    assert set(_lib.FOLD_PROTOTYPES) == set(WANT)
    for name in WANT:
        assert [_c_kind(p) for p in _header_params(name)] == WANT[name], name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert [kinds[a] for a in _lib.FOLD_PROTOTYPES[name]] == [word(k) for k in WANT[name]], name
        assert getattr(lib, name).argtypes == _lib.FOLD_PROTOTYPES[name] and getattr(lib, name).restype is C.c_int
        m = re.search(r'fn\s+"%s"\s*\((.*?)returning int\)' % name, ml, flags=re.S)
        assert m, "%s is not bound in ocaml/mi355x.ml" % name
        assert [ml_kind[" ".join(a.split())] for a in m.group(1).split("@->")[:-1]] == WANT[name], name
    # the header states the contract for rho where the call is declared
    doc = HEADER[:HEADER.index("int zk_groth16_verify_folded(")]
    doc = " ".join(doc[doc.rindex("/*"):].split())
    for words in ("AFTER the proofs are fixed", "unpredictable", "2^-128", "CAN pass", "non-zero", "test.ml:107-179"):
        assert words in doc, words
    # the protocol file: Verifier.verify_all beside verify_many, drawing from an rng
    src = re.sub(r"\(\*.*?\*\)", " ", open(os.path.join(ROOT, "ocaml", "groth16_mi355x.ml")).read(), flags=re.S)
    v = src[src.index("module Verifier = struct"):]
    assert re.search(r"let verify_all\s+\(?rng\b", v) and "zk_groth16_verify_folded" in v


def _args(count=1, rho=None):
    g1, g2 = P.g1_to_bytes(P.G1), P.g2_to_bytes(P.G2)
    rho = bytes([5] + [0] * 15) * count if rho is None else rho
    return [u8(bytes(64) * count), u8((g1 + g2 + g1) * count), u8(rho), count]


def test_what_needs_no_handle_is_an_argument_error_before_the_table_and_the_device():
    lib = _lib.lib()
    ok, st = C.c_int(9), (C.c_int32 * 4)(7, 7, 7, 7)
    for handle in (0, 0x7FFFFFFFFFFFFFFF):                      # whatever the handle: these come first
        for hole in (1, 2):
            args = _args()
            args[hole] = None
            assert lib.zk_groth16_verify_folded(handle, *args, C.byref(ok), st) == ZK_ERR_ARG, hole
        assert lib.zk_groth16_verify_folded(handle, *_args(), None, st) == ZK_ERR_ARG
        assert lib.zk_groth16_verify_folded(handle, *_args(rho=bytes(16)), C.byref(ok), st) == ZK_ERR_ARG                          # rho = 0
        assert lib.zk_groth16_verify_folded(handle, *_args(3, rho=bytes([1] + [0] * 15) * 2 + bytes(16)), C.byref(ok), st) == ZK_ERR_ARG    # the last rho = 0
        assert b"rho" in lib.zk_last_error()
        args = _args()
        args[3] = (1 << 24) + 1
        assert lib.zk_groth16_verify_folded(handle, *args, C.byref(ok), st) == ZK_ERR_ARG
        out = [(C.c_uint8 * k)() for k in (576, 576, 96, 96)]
        outs = [C.cast(b, _lib._P8) for b in out]
        assert lib.zk_selftest_groth16_fold(handle, *_args(rho=bytes(16)), *outs, st) == ZK_ERR_ARG
        args = _args()
        args[3] = 0
        assert lib.zk_selftest_groth16_fold(handle, *args, *outs, st) == ZK_ERR_ARG                                               # the hook wants proofs
        for hole in range(4):
            o2 = list(outs)
            o2[hole] = None
            assert lib.zk_selftest_groth16_fold(handle, *_args(), *o2, st) == ZK_ERR_ARG
    assert ok.value == 9 and list(st) == [7] * 4


def test_a_handle_of_zero_is_unknown():
    lib = _lib.lib()
    ok, st = C.c_int(9), (C.c_int32 * 1)(7)
    assert lib.zk_groth16_verify_folded(0, *_args(), C.byref(ok), st) == ZK_ERR_HANDLE
    assert lib.zk_groth16_verify_folded(0, None, None, None, 0, C.byref(ok), None) == ZK_ERR_HANDLE          # count = 0 does not excuse it
    out = [C.cast((C.c_uint8 * k)(), _lib._P8) for k in (576, 576, 96, 96)]
    assert lib.zk_selftest_groth16_fold(0, *_args(), *out, st) == ZK_ERR_HANDLE
    assert ok.value == 9 and list(st) == [7]


@pytest.mark.skipif(_gpu_present(), reason="a GPU is visible: the call runs (tests/test_gpu_verify_folded.py)")
def test_without_a_gpu_the_call_is_a_hip_error():
    lib = _lib.lib()
    ok, st = C.c_int(9), (C.c_int32 * 1)(7)
    assert lib.zk_groth16_verify_folded(0x7FFFFFFFFFFFFFFF, *_args(), C.byref(ok), st) == ZK_ERR_HIP
    out = [C.cast((C.c_uint8 * k)(), _lib._P8) for k in (576, 576, 96, 96)]
    assert lib.zk_selftest_groth16_fold(0x7FFFFFFFFFFFFFFF, *_args(), *out, st) == ZK_ERR_HIP
    assert ok.value == 9 and list(st) == [7]


def test_verify_all_refuses_what_the_object_can_see():
    g1, g2 = P.g1_to_bytes(P.G1), P.g2_to_bytes(P.G2)
    pr = Proof(g1, g2, g1)
    rv = ResidentVKey(0x7FFFFFFFFFFFFFFF, 2, lambda p: bytes(p.a) + bytes(p.b) + bytes(p.c), 384, "zk_groth16_verify_resident")
    with pytest.raises(ValueError):
        rv.verify_all([[1, 2]], [pr, pr])                        # one list of inputs, two proofs
    with pytest.raises(AssertionError):
        rv.verify_all([[1, 2, 3]], [pr])                         # three inputs against a key of two
    with pytest.raises(ValueError):
        rv.verify_all([[1, 2]], [Proof(g1, g2, g1[:95])])        # a proof of 383 bytes
    for rho in ([1, 2], [0], [1 << 128], [-1]):
        with pytest.raises(ValueError):
            rv.verify_all([[1, 2]], [pr], rho=rho)               # one coefficient per proof, 0 < rho < 2^128
    with pytest.raises(_lib.ZkError) as e:
        rv.verify_all([[1, 2]], [pr])                            # the made-up handle reaches the library only now
    assert e.value.code == (ZK_ERR_HANDLE if _gpu_present() else ZK_ERR_HIP)
    rv.handle = 0                                                # as after close()
    with pytest.raises(ValueError):
        rv.verify_all([[1, 2]], [pr])
    with pytest.raises(ValueError):
        rv.verify_many([[1, 2]], [pr], fold_first=True)
    pin = ResidentVKey(0x7FFFFFFFFFFFFFFF, 1, bytes, 960, "zk_pinocchio_verify_resident")
    for call in (lambda: pin.verify_all([[1]], [bytes(960)]), lambda: pin.verify_many([[1]], [bytes(960)], fold_first=True)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "Pinocchio" in str(e.value)
    pin.handle = 0
    assert all(0 < G._draw_rho() < 1 << 128 for _ in range(8))


def test_verify_many_without_fold_first_builds_the_call_it_built_before(monkeypatch):
    g1, g2 = P.g1_to_bytes(P.G1), P.g2_to_bytes(P.G2)
    seen = []

    class Lib:
        def zk_groth16_verify_resident(self, handle, io, proofs, count, ok, status):
            seen.append(("resident", handle.value, bytes(C.cast(io, C.POINTER(C.c_uint8 * 128)).contents), bytes(C.cast(proofs, C.POINTER(C.c_uint8 * 768)).contents),
                         count.value))
            ok[0], ok[1], status[0], status[1] = 1, 0, 0, -2
            return 0

        def zk_groth16_verify_folded(self, *a):
            seen.append(("folded",))
            a[5]._obj.value = 0
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    rv = ResidentVKey(77, 2, lambda p: bytes(p.a) + bytes(p.b) + bytes(p.c), 384, "zk_groth16_verify_resident")
    prs = [Proof(g1, g2, g1), Proof(g1, g2, g1)]
    want = ("resident", 77, b"".join(int(x).to_bytes(32, "little") for x in (1, 2, 3, 4)), (g1 + g2 + g1) * 2, 2)
    assert rv.verify_many([[1, 2], [3, 4]], prs, return_status=True) == ([True, False], [0, -2]) and seen == [want]
    assert rv.verify_many([[1, 2], [3, 4]], prs, fold_first=False) == [True, False] and seen == [want, want]
    assert rv.verify_many([[1, 2], [3, 4]], prs, fold_first=True) == [True, False] and seen == [want, want, ("folded",), want]       # a failed fold falls through
    rv.handle = 0
