"""A batch of witnesses proved in one call, the proofs out as wire bytes -- without a GPU: include/zkmi355x.h, _lib.EXPORTS, _lib.PROVE_MANY_PROTOTYPES
and the OCaml files name the same three calls with the same argument lists; every refusal the header promises comes before the device is touched; a box
without a GPU answers ZK_ERR_HIP; and wire.groth16_proof_json_of_bytes / pinocchio_proof_json_of_bytes are the inverses of the *_proof_bytes_of_json
readers on the golden proofs (no point arithmetic on the way)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from oracle import pyref as P
from zukelang_amd import _lib, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()

MANY = ["uint64_t", "ptr", "ptr", "uint32_t", "uint32_t", "ptr", "ptr"]
WANT = {
    "zk_groth16_prove_many_compressed": MANY,
    "zk_pinocchio_prove_many_compressed": MANY,
    "zk_selftest_proof_wire": ["int", "ptr", "ptr", "size_t", "ptr"],
}


def _header_kinds(name):
    body = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, body)
    assert m, "%s is not declared in include/zkmi355x.h" % name
    out = []
    for p in m.group(1).split(","):
        p = re.sub(r"\[[^\]]*\]", "*", p)
        out.append("ptr" if "*" in p else next(t for t in ("uint64_t", "uint32_t", "size_t", "int") if re.search(r"\b%s\b" % t, p)))
    return out


def test_the_three_calls_are_declared_exported_and_bound():
    lib = _lib.lib()
    kinds = {C.c_uint32: "uint32_t", C.c_uint64: "uint64_t", C.c_size_t: "size_t", C.c_int: "int"}
    assert set(_lib.PROVE_MANY_PROTOTYPES) == set(WANT)
    for name, want in WANT.items():
        assert _header_kinds(name) == want, name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        # (ctypes has ONE class for uint64_t and size_t on this ABI: the two compare as one kind)
        assert [kinds.get(a, "ptr") for a in _lib.PROVE_MANY_PROTOTYPES[name]] == [kinds[C.c_uint64] if w in ("uint64_t", "size_t") else w for w in want], name
        assert getattr(lib, name).argtypes == _lib.PROVE_MANY_PROTOTYPES[name] and getattr(lib, name).restype is C.c_int
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    for name in WANT:
        assert 'fn "%s"' % name in ml, name
    g = open(os.path.join(ROOT, "ocaml", "groth16_mi355x.ml")).read()
    p = open(os.path.join(ROOT, "ocaml", "pinocchio_mi355x.ml")).read()
    assert "let prove_many_compressed" in g and "zk_groth16_prove_many_compressed" in g
    assert "let prove_many " in p and "let prove_many_with" in p and "zk_pinocchio_prove_many_compressed" in p
    # the header cites what the calls replace and names the default it chose
    for cite in ("groth16.ml:123-161,235-237", "pinocchio.ml:427-514", "0 = the library's default, 14"):
        assert cite in HEADER, cite
    # ... and the Python surface is there
    from zukelang_amd import pinocchio as PIN
    from zukelang_amd.groth16 import Groth16
    assert all(callable(getattr(c, "prove_many")) for c in (Groth16, PIN.ZK, PIN.NonZK))


def _p8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


@pytest.mark.parametrize("name,rnd,size", [("zk_groth16_prove_many_compressed", 64, 192), ("zk_pinocchio_prove_many_compressed", 96, 480)])
def test_every_refusal_comes_before_the_device(name, rnd, size):
    lib = _lib.lib()
    fn = getattr(lib, name)
    count = 3
    sols, r = np.zeros(32 * 5 * count, dtype=np.uint8), np.zeros(rnd * count, dtype=np.uint8)
    out, st = np.full(size * count, 0x55, dtype=np.uint8), np.full(count, 77, dtype=np.int32)
    pst = st.ctypes.data_as(C.POINTER(C.c_int32))
    h = C.c_uint64(0x7777)          # no key was ever uploaded in this process: whatever comes AFTER the argument checks cannot be ZK_ERR_ARG
    assert fn(h, _p8(sols), None, count, 0, _p8(out), pst) == -1           # null rs / blind
    assert fn(h, _p8(sols), _p8(r), count, 0, None, pst) == -1             # null proofs
    assert fn(h, _p8(sols), _p8(r), count, 0, _p8(out), None) == -1        # null status
    assert fn(h, _p8(sols), _p8(r), count, 16, _p8(out), pst) == -1        # in_flight > 15
    assert fn(h, _p8(sols), _p8(r), (1 << 24) + 1, 0, _p8(out), pst) == -1          # count > 2^24: refused before a byte of the (too short) buffers is read
    assert b"2^24" in lib.zk_last_error()
    # count = 0 touches nothing and is fine, whatever the handle
    assert fn(h, None, _p8(r), 0, 0, _p8(out), pst) == 0
    assert fn(h, None, _p8(r), 0, 15, _p8(out), pst) == 0
    # valid arguments, a handle that does not exist: ZK_ERR_HANDLE where a device answers, ZK_ERR_HIP on a box without one
    want = -7 if lib.zk_device_count() > 0 else -5
    for infl in (0, 1, 15):
        assert fn(h, _p8(sols), _p8(r), count, infl, _p8(out), pst) == want, infl
        assert fn(h, None, _p8(r), count, infl, _p8(out), pst) == want, infl
    assert (out == 0x55).all() and (st == 77).all()          # nothing was written by any of the refusals


def test_the_hook_refuses_before_the_device():
    lib = _lib.lib()
    a, z, out = np.zeros(192 * 2, dtype=np.uint8), np.ones(64, dtype=np.uint8), np.zeros(96 * 2, dtype=np.uint8)
    assert lib.zk_selftest_proof_wire(0, None, _p8(z), 2, _p8(out)) == -1
    assert lib.zk_selftest_proof_wire(0, _p8(a), None, 2, _p8(out)) == -1
    assert lib.zk_selftest_proof_wire(0, _p8(a), _p8(z), 2, None) == -1
    assert lib.zk_selftest_proof_wire(0, _p8(a), _p8(z), 0, _p8(out)) == -1
    assert lib.zk_selftest_proof_wire(2, _p8(a), _p8(z), 2, _p8(out)) == -1
    assert lib.zk_selftest_proof_wire(-1, _p8(a), _p8(z), 2, _p8(out)) == -1
    if lib.zk_device_count() == 0:
        assert lib.zk_selftest_proof_wire(0, _p8(a), _p8(z), 2, _p8(out)) == -5
        assert lib.zk_selftest_proof_wire(1, _p8(a), _p8(z), 2, _p8(out)) == -5


def _golden_groth16():
    return bytes.fromhex(open(os.path.join(GOLDEN, "readme_groth16_wire.hex")).read().split()[1])


def _golden_pinocchio():
    """the golden proofs' 480 wire bytes through the oracle's compressor (oracle/pyref.py)"""
    fix = json.load(open(os.path.join(GOLDEN, "readme_pinocchio_key.json")))
    out = []
    for key in ("proof", "proof_nonzk"):
        b, o, w = bytes.fromhex(fix[key]), 0, b""
        for _, g in wire._PIN_FIELDS:
            w += P.g1_compress(P.g1_from_bytes(b[o:o + 96])) if g == 1 else P.g2_compress(P.g2_from_bytes(b[o:o + 192]))
            o += 96 * g
        out.append(w)
    return out


def test_json_of_bytes_round_trips_the_golden_proofs():
    js = _golden_groth16()
    b = wire.groth16_proof_bytes_of_json(js)
    assert len(b) == 192 and wire.groth16_proof_json_of_bytes(b) == js          # the reference's text, byte for byte
    assert wire.groth16_proof_json_of_bytes(bytearray(b)) == js and wire.groth16_proof_json_of_bytes(np.frombuffer(b, dtype=np.uint8)) == js
    for b in _golden_pinocchio():
        js = wire.pinocchio_proof_json_of_bytes(b)
        assert wire.pinocchio_proof_bytes_of_json(js) == b
        d = wire.loads(js)
        assert list(d) == [f for f, _ in wire._PIN_FIELDS] and [len(d[f]) for f, _ in wire._PIN_FIELDS] == [48 * g for _, g in wire._PIN_FIELDS]
        assert b"".join(d[f] for f, _ in wire._PIN_FIELDS) == b
    # no point arithmetic: bytes that are no points at all pass through both ways
    junk = bytes(range(192))
    assert wire.groth16_proof_bytes_of_json(wire.groth16_proof_json_of_bytes(junk)) == junk
    assert wire.pinocchio_proof_bytes_of_json(wire.pinocchio_proof_json_of_bytes(bytes(480))) == bytes(480)


def test_json_of_bytes_refuses_wrong_lengths():
    for bad in (b"", bytes(191), bytes(193), bytes(480), bytes(384)):
        with pytest.raises(ValueError, match="192 wire bytes"):
            wire.groth16_proof_json_of_bytes(bad)
    for bad in (b"", bytes(479), bytes(481), bytes(192), bytes(960)):
        with pytest.raises(ValueError, match="480 wire bytes"):
            wire.pinocchio_proof_json_of_bytes(bad)
