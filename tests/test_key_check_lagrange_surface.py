"""zk_groth16_key_check_lagrange without a GPU: include/zkmi355x.h, _lib.EXPORTS, _lib.KEY_CHECK_LAGRANGE_PROTOTYPES and the OCaml files name the same
call with the argument list of zk_groth16_key_check; every refusal that needs no handle comes before the device is touched; a box without a GPU
answers ZK_ERR_HIP; the Python method refuses a seed that is not 32 bytes before it calls anything; and the documents point to the call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from zukelang_amd import _lib
from zukelang_amd.groth16 import Groth16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
NAME = "zk_groth16_key_check_lagrange"
WANT = ["uint64_t", "ptr", "size_t", "ptr", "ptr", "ptr"]


def _header_kinds(name):
    body = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, body)
    assert m, "%s is not declared in include/zkmi355x.h" % name
    out = []
    for p in m.group(1).split(","):
        p = re.sub(r"\[[^\]]*\]", "*", p)
        out.append("ptr" if "*" in p else next(t for t in ("uint64_t", "uint32_t", "size_t", "int") if re.search(r"\b%s\b" % t, p)))
    return out


def test_the_call_is_declared_exported_and_bound():
    lib = _lib.lib()
    assert _header_kinds(NAME) == WANT == _header_kinds("zk_groth16_key_check")
    assert NAME in _lib.EXPORTS and hasattr(lib, NAME)
    assert set(_lib.KEY_CHECK_LAGRANGE_PROTOTYPES) == {NAME}
    assert _lib.KEY_CHECK_LAGRANGE_PROTOTYPES[NAME] == _lib.KEY_CHECK_PROTOTYPES["zk_groth16_key_check"]
    assert getattr(lib, NAME).argtypes == _lib.KEY_CHECK_LAGRANGE_PROTOTYPES[NAME] and getattr(lib, NAME).restype is C.c_int
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    assert 'fn "%s"' % NAME in ml and "let groth16_key_check_lagrange" in ml
    g = open(os.path.join(ROOT, "ocaml", "groth16_mi355x.ml")).read()
    assert "let check_key_lagrange" in g and "Mi355x.groth16_key_check_lagrange" in g
    assert callable(Groth16.check_lagrange_key)


def test_the_documents_point_to_the_call():
    for text in ("THE SAME CONTRACT", "(zk_groth16_key_check is its call)", "zk_groth16_key_check_lagrange checks that form"):
        assert text in HEADER, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "2n" in design and NAME in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc


def _p8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def test_argument_errors_come_before_the_device():
    lib = _lib.lib()
    fn = getattr(lib, NAME)
    v1, v2, seed = np.zeros(96 * 3, dtype=np.uint8), np.zeros(192 * 3, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
    failed = C.c_uint32(77)
    h = C.c_uint64(0x7777)          # no key was ever uploaded in this process
    assert fn(h, _p8(v1), 2, _p8(v2), _p8(seed), None) == -1                       # null failed
    assert b"key_check_lagrange" in lib.zk_last_error() and b"failed" in lib.zk_last_error()
    assert fn(h, _p8(v1), 2, None, _p8(seed), C.byref(failed)) == -1               # exactly one of vk_g1 / vk_g2
    assert fn(h, None, 2, _p8(v2), _p8(seed), C.byref(failed)) == -1
    assert b"together" in lib.zk_last_error()
    assert failed.value == 77                                                      # a refused call writes no verdict
    # valid arguments, a handle that does not exist: ZK_ERR_HANDLE where a device answers, ZK_ERR_HIP on a box without one
    want = -7 if lib.zk_device_count() > 0 else -5
    assert fn(h, _p8(v1), 2, _p8(v2), _p8(seed), C.byref(failed)) == want
    assert fn(h, None, 0, None, None, C.byref(failed)) == want
    assert failed.value == 77


def test_the_method_wants_a_seed_of_32_bytes():
    prover = Groth16.__new__(Groth16)          # no handle: the seed is looked at before anything is called
    prover.handle = None
    for bad in (b"", bytes(31), bytes(33)):
        with pytest.raises(ValueError, match="check_lagrange_key: the seed is 32 bytes"):
            prover.check_lagrange_key(seed=bad)
