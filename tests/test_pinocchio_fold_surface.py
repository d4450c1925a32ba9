"""Pinocchio's folded verifier's surface without a GPU: include/zkmi355x.h, _lib.EXPORTS, _lib.PIN_FOLD_PROTOTYPES and the OCaml stubs name the same
two calls with the same argument lists; the header states the contract for the five coefficients where the call is declared; what needs no handle is
refused before the handle table or the device is looked at (a null pointer, a zero in any of a proof's five positions, too many proofs) and leaves the
outputs alone; a handle of 0 is ZK_ERR_HANDLE and, without a GPU, any other is ZK_ERR_HIP; the Python object refuses what it can refuse itself.
What the calls compute is held to pyref and the host pairing on the GPU: tests/test_gpu_pinocchio_verify_folded.py."""
import ctypes as C
import os
import re

import pytest

from oracle import pyref as P
from zukelang_amd import _lib
from zukelang_amd import pinocchio as PIN
import test_verify_folded_surface as S

ROOT = S.ROOT
ZK_OK, ZK_ERR_ARG, ZK_ERR_HIP, ZK_ERR_HANDLE = 0, -1, -5, -7
# the issue's prototypes, parameter kinds in order
WANT = {
    "zk_pinocchio_verify_folded": ["uint64_t", "u8p", "u8p", "u8p", "uint32_t", "intp", "i32p"],
    "zk_selftest_pinocchio_fold": ["uint64_t", "u8p", "u8p", "u8p", "uint32_t", "u8p", "u8p", "u8p", "i32p"],
}
u8 = S.u8
ANY = 0x7FFFFFFFFFFFFFFF
ROW = b"".join(bytes([k] + [0] * 15) for k in (1, 2, 3, 4, 5))          # rho_0 .. rho_4 of one proof


def test_header_exports_ctypes_and_ocaml_agree():
    kinds = {_lib._P8: "u8p", _lib._PI32: "i32p", C.c_uint64: "uint64_t", C.c_uint32: "uint32_t"}
    word = lambda k: "i32p" if k == "intp" else k          # ctypes has ONE type for int and int32_t on this ABI
    lib = _lib.lib()
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    ml_kind = {"ocaml_bytes": "u8p", "ptr int32_t": "i32p", "ptr int": "intp", "uint64_t": "uint64_t", "uint32_t": "uint32_t"}
    assert set(_lib.PIN_FOLD_PROTOTYPES) == set(WANT)
    for name in WANT:
        assert [S._c_kind(p) for p in S._header_params(name)] == WANT[name], name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert [kinds[a] for a in _lib.PIN_FOLD_PROTOTYPES[name]] == [word(k) for k in WANT[name]], name
        assert getattr(lib, name).argtypes == _lib.PIN_FOLD_PROTOTYPES[name] and getattr(lib, name).restype is C.c_int
        m = re.search(r'fn\s+"%s"\s*\((.*?)returning int\)' % name, ml, flags=re.S)
        assert m, "%s is not bound in ocaml/mi355x.ml" % name
        assert [ml_kind[" ".join(a.split())] for a in m.group(1).split("@->")[:-1]] == WANT[name], name
    # the header states the contract for rho where the call is declared: the Groth16 call's words, five coefficients, both cancellations
    doc = S.HEADER[:S.HEADER.index("int zk_pinocchio_verify_folded(")]
    doc = " ".join(doc[doc.rindex("/*"):].split())
    for words in ("AFTER the proofs are fixed", "unpredictable", "2^-128", "CAN pass", "non-zero", "FIVE coefficients per proof", "rho_00 = rho_10", "rho_i0 = rho_i2",
                  "five independent coefficients"):
        assert words in doc, words
    # the protocol file: Verifier.verify_all beside verify_many, drawing from an rng
    src = re.sub(r"\(\*.*?\*\)", " ", open(os.path.join(ROOT, "ocaml", "pinocchio_mi355x.ml")).read(), flags=re.S)
    v = src[src.index("module Verifier = struct"):]
    assert re.search(r"let verify_all\s+\(?rng\b", v) and "zk_pinocchio_verify_folded" in v and "5 * count" in v


def _args(count=1, rho=None):
    g1, g2 = P.g1_to_bytes(P.G1), P.g2_to_bytes(P.G2)
    proof = g1 + g2 + g1 * 3 + g2 + g1 * 2
    assert len(proof) == 960
    return [u8(bytes(32) * count), u8(proof * count), u8(ROW * count if rho is None else rho), count]


def _outs():
    return [C.cast((C.c_uint8 * k)(), _lib._P8) for k in (576, 7 * 96, 3 * 192)]


def test_what_needs_no_handle_is_an_argument_error_before_the_table_and_the_device():
    lib = _lib.lib()
    ok, st = C.c_int(9), (C.c_int32 * 4)(7, 7, 7, 7)
    for handle in (0, ANY):                                     # whatever the handle: these come first
        for hole in (1, 2):                                     # proofs, rho
            args = _args()
            args[hole] = None
            assert lib.zk_pinocchio_verify_folded(handle, *args, C.byref(ok), st) == ZK_ERR_ARG, hole
        assert lib.zk_pinocchio_verify_folded(handle, *_args(), None, st) == ZK_ERR_ARG
        for e in range(5):                                      # a zero in any of the five positions
            zero = ROW[:16 * e] + bytes(16) + ROW[16 * e + 16:]
            assert lib.zk_pinocchio_verify_folded(handle, *_args(rho=zero), C.byref(ok), st) == ZK_ERR_ARG, e
            assert b"rho" in lib.zk_last_error()
            assert lib.zk_pinocchio_verify_folded(handle, *_args(3, rho=ROW * 2 + zero), C.byref(ok), st) == ZK_ERR_ARG, e          # in the last proof's row
            assert lib.zk_selftest_pinocchio_fold(handle, *_args(rho=zero), *_outs(), st) == ZK_ERR_ARG, e
        args = _args()
        args[3] = (1 << 24) + 1
        assert lib.zk_pinocchio_verify_folded(handle, *args, C.byref(ok), st) == ZK_ERR_ARG
        args = _args()
        args[3] = 0
        assert lib.zk_selftest_pinocchio_fold(handle, *args, *_outs(), st) == ZK_ERR_ARG                                               # the hook wants proofs
        for hole in range(3):
            outs = _outs()
            outs[hole] = None
            assert lib.zk_selftest_pinocchio_fold(handle, *_args(), *outs, st) == ZK_ERR_ARG
    assert ok.value == 9 and list(st) == [7] * 4


def test_a_handle_of_zero_is_unknown():
    lib = _lib.lib()
    ok, st = C.c_int(9), (C.c_int32 * 1)(7)
    assert lib.zk_pinocchio_verify_folded(0, *_args(), C.byref(ok), st) == ZK_ERR_HANDLE
    assert lib.zk_pinocchio_verify_folded(0, None, None, None, 0, C.byref(ok), None) == ZK_ERR_HANDLE          # count = 0 does not excuse it
    assert lib.zk_selftest_pinocchio_fold(0, *_args(), *_outs(), st) == ZK_ERR_HANDLE
    assert ok.value == 9 and list(st) == [7]


@pytest.mark.skipif(S._gpu_present(), reason="a GPU is visible: the call runs (tests/test_gpu_pinocchio_verify_folded.py)")
def test_without_a_gpu_the_call_is_a_hip_error():
    lib = _lib.lib()
    ok, st = C.c_int(9), (C.c_int32 * 1)(7)
    assert lib.zk_pinocchio_verify_folded(ANY, *_args(), C.byref(ok), st) == ZK_ERR_HIP
    assert lib.zk_selftest_pinocchio_fold(ANY, *_args(), *_outs(), st) == ZK_ERR_HIP
    assert ok.value == 9 and list(st) == [7]


def test_verify_all_refuses_what_the_object_can_see():
    pr = bytes(960)
    rv = PIN.PinocchioResidentVKey(ANY, 1)
    good = [[1, 2, 3, 4, 5]]
    with pytest.raises(ValueError):
        rv.verify_all([[1]], [pr, pr])                           # one list of inputs, two proofs
    with pytest.raises(ValueError):
        rv.verify_all([[1]], [bytes(959)])                       # a proof of 959 bytes
    for rho in ([[1, 2, 3, 4]], [[1, 2, 0, 4, 5]], [[1, 2, 3, 4, 1 << 128]], [[-1, 2, 3, 4, 5]], [1, 2, 3, 4, 5], good * 2):
        with pytest.raises(ValueError):
            rv.verify_all([[1]], [pr], rho=rho)                  # one row of five per proof, 0 < rho < 2^128
    with pytest.raises(_lib.ZkError) as e:
        rv.verify_all([[1]], [pr], rho=good)                     # the made-up handle reaches the library only now
    assert e.value.code == (ZK_ERR_HANDLE if S._gpu_present() else ZK_ERR_HIP)
    with pytest.raises(_lib.ZkError):
        rv.verify_all([[1]], [pr])                               # ... and with rows drawn here
    rv.handle = 0                                                # as after close()
    with pytest.raises(ValueError):
        rv.verify_all([[1]], [pr], rho=good)
    with pytest.raises(ValueError):
        rv.verify_many([[1]], [pr], fold_first=True)
    assert all(len(row) == 5 and all(0 < r < 1 << 128 for r in row) for row in (PIN._draw_rho_row() for _ in range(8)))
