"""The key check without a GPU: include/zkmi355x.h, _lib.EXPORTS, _lib.KEY_CHECK_PROTOTYPES and the OCaml files name the same call with the same
argument list and the same bits; every refusal that needs no handle comes before the device is touched; a box without a GPU answers ZK_ERR_HIP; and
the Python wrapper maps the mask's bits to names."""
import ctypes as C
import os
import re

import numpy as np

from zukelang_amd import _lib
from zukelang_amd.groth16 import Groth16, KeyCheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
WANT = {"zk_groth16_key_check": ["uint64_t", "ptr", "size_t", "ptr", "ptr", "ptr"]}
BITS = {"GENERATORS": 1, "TAU_G1": 2, "TAU_G2": 4, "BETA": 8, "DELTA": 16, "H_BASES": 32, "L": 64, "GAMMA": 128}


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
    kinds = {C.c_uint32: "uint32_t", C.c_uint64: "uint64_t", C.c_size_t: "size_t", C.c_int: "int"}
    assert set(_lib.KEY_CHECK_PROTOTYPES) == set(WANT)
    for name, want in WANT.items():
        assert _header_kinds(name) == want, name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert [kinds.get(a, "ptr") for a in _lib.KEY_CHECK_PROTOTYPES[name]] == [kinds[C.c_uint64] if w in ("uint64_t", "size_t") else w for w in want], name
        assert getattr(lib, name).argtypes == _lib.KEY_CHECK_PROTOTYPES[name] and getattr(lib, name).restype is C.c_int
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    assert 'fn "zk_groth16_key_check"' in ml and "let groth16_key_check" in ml
    g = open(os.path.join(ROOT, "ocaml", "groth16_mi355x.ml")).read()
    assert "let check_key" in g and "Mi355x.groth16_key_check" in g
    assert callable(Groth16.check_key)


def test_the_bits_have_one_value_everywhere():
    defs = dict(re.findall(r"#define ZK_KEYCHK_([A-Z0-9_]+)\s+(\d+)u", HEADER))
    assert {k: int(v) for k, v in defs.items()} == BITS
    assert _lib.KEYCHK_BITS == {k.lower(): v for k, v in BITS.items()}
    assert list(_lib.KEYCHK_BITS.values()) == sorted(_lib.KEYCHK_BITS.values())
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    assert dict((name, int(bit)) for bit, name in re.findall(r'\((\d+), "([a-z0-9_]+)"\)', ml)) == _lib.KEYCHK_BITS
    assert _lib.KEYCHK_AB not in BITS.values() and _lib.KEYCHK_AB & sum(BITS.values()) == 0
    # the header states the seed's contract by the call it shares it with, and what the check leaves out
    for text in ("THE CONTRACT FOR seed is that of rho in zk_groth16_verify_folded", "std::random_device", "Out of scope: Pinocchio keys"):
        assert text in HEADER, text


def test_the_wrapper_maps_bits_to_names():
    assert KeyCheck(0).ok and KeyCheck(0).names == [] and bool(KeyCheck(0))
    for name, bit in _lib.KEYCHK_BITS.items():
        r = KeyCheck(bit)
        assert not r.ok and r.failed == bit and r.names == [name]
    r = KeyCheck(2 | 64 | _lib.KEYCHK_AB)
    assert r.names == ["tau_g1", "l", "ab"] and not r and "tau_g1|l|ab" in repr(r)
    assert KeyCheck(sum(BITS.values())).names == list(_lib.KEYCHK_BITS)


def _p8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def test_argument_errors_come_before_the_device():
    lib = _lib.lib()
    fn = lib.zk_groth16_key_check
    v1, v2, seed = np.zeros(96 * 3, dtype=np.uint8), np.zeros(192 * 3, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
    failed = C.c_uint32(77)
    h = C.c_uint64(0x7777)          # no key was ever uploaded in this process
    assert fn(h, _p8(v1), 2, _p8(v2), _p8(seed), None) == -1                       # null failed
    assert b"failed" in lib.zk_last_error()
    assert fn(h, _p8(v1), 2, None, _p8(seed), C.byref(failed)) == -1               # exactly one of vk_g1 / vk_g2
    assert fn(h, None, 2, _p8(v2), _p8(seed), C.byref(failed)) == -1
    assert b"together" in lib.zk_last_error()
    assert failed.value == 77                                                      # a refused call writes no verdict
    # valid arguments, a handle that does not exist: ZK_ERR_HANDLE where a device answers, ZK_ERR_HIP on a box without one
    want = -7 if lib.zk_device_count() > 0 else -5
    assert fn(h, _p8(v1), 2, _p8(v2), _p8(seed), C.byref(failed)) == want
    assert fn(h, None, 0, None, None, C.byref(failed)) == want
