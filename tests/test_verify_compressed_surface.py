"""The compressed verifiers' surface without a GPU: include/zkmi355x.h, _lib.EXPORTS, _lib.COMPRESSED_PROTOTYPES and the OCaml stubs name the same four
calls (and the decompression hook) with the argument lists of their uncompressed twins; the argument, handle and no-GPU answers are the twins', in the
twins' order, and leave the outputs alone; wire.*_proof_bytes_of_json turns a JSON proof into the bytes the calls take without a library call; the
Python objects refuse a proof of the wrong length themselves.  What the calls compute is held to pyref and the host verifiers on the GPU:
tests/test_gpu_verify_compressed.py, tests/test_gpu_point_decompress.py."""
import ctypes as C
import json
import os
import re

import pytest

from oracle import pyref as P
from zukelang_amd import _lib, wire
from zukelang_amd import groth16 as G
from zukelang_amd import pinocchio as PIN
import test_verify_folded_surface as S

ROOT = S.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden")
ZK_OK, ZK_ERR_ARG, ZK_ERR_HIP, ZK_ERR_HANDLE = 0, -1, -5, -7
ANY = 0x7FFFFFFFFFFFFFFF
RESIDENT = ["uint64_t", "u8p", "u8p", "uint32_t", "u8p", "i32p"]
FOLDED = ["uint64_t", "u8p", "u8p", "u8p", "uint32_t", "intp", "i32p"]
WANT = {
    "zk_groth16_verify_resident_compressed": RESIDENT,
    "zk_pinocchio_verify_resident_compressed": RESIDENT,
    "zk_groth16_verify_folded_compressed": FOLDED,
    "zk_pinocchio_verify_folded_compressed": FOLDED,
    "zk_selftest_point_decompress": ["int", "u8p", "size_t", "u8p", "u8p"],
}
u8 = S.u8
G1C, G2C = P.g1_compress(P.G1), P.g2_compress(P.G2)
WIRE = {"groth16": G1C + G2C + G1C, "pinocchio": G1C + G2C + G1C * 3 + G2C + G1C * 2}
RHO = {"groth16": bytes([5] + [0] * 15), "pinocchio": b"".join(bytes([k] + [0] * 15) for k in (1, 2, 3, 4, 5))}
PROTOCOLS = ("groth16", "pinocchio")


def test_header_exports_ctypes_and_ocaml_agree():
    assert len(WIRE["groth16"]) == 192 and len(WIRE["pinocchio"]) == 480
    kinds = {_lib._P8: "u8p", _lib._PI32: "i32p", C.c_uint64: "uint64_t", C.c_uint32: "uint32_t", C.c_int: "int"}
    word = lambda k: {"intp": "i32p", "size_t": "uint64_t"}.get(k, k)          # ctypes has ONE type for int and int32_t, and for size_t and uint64_t, on this ABI
    lib = _lib.lib()
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    ml_kind = {"ocaml_bytes": "u8p", "ptr int32_t": "i32p", "ptr int": "intp", "uint64_t": "uint64_t", "uint32_t": "uint32_t"}
    assert set(_lib.COMPRESSED_PROTOTYPES) == set(WANT)
    for name in WANT:
        assert [S._c_kind(p) for p in S._header_params(name)] == WANT[name], name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert [kinds[a] for a in _lib.COMPRESSED_PROTOTYPES[name]] == [word(k) for k in WANT[name]], name
        assert getattr(lib, name).argtypes == _lib.COMPRESSED_PROTOTYPES[name] and getattr(lib, name).restype is C.c_int
        twin = name.replace("_compressed", "")
        if twin != name:
            # the twin's parameter list, kind for kind, in the header and in the OCaml stubs
            assert [S._c_kind(p) for p in S._header_params(twin)] == WANT[name], name
            m = re.search(r'fn\s+"%s"\s*\((.*?)returning int\)' % name, ml, flags=re.S)
            assert m, "%s is not bound in ocaml/mi355x.ml" % name
            assert [ml_kind[" ".join(a.split())] for a in m.group(1).split("@->")[:-1]] == WANT[name], name
    # the header states the contract where the calls are declared
    doc = S.HEADER[:S.HEADER.index("int zk_groth16_verify_resident_compressed(")]
    doc = " ".join(doc[doc.rindex("/*"):].split())
    for words in ("FIRST bad point", "ZK_ERR_ARG", "ZK_ERR_NOT_ON_CURVE", "ZK_ERR_SCALAR_RANGE", "byte for byte", "by endomorphism", "verify_point_decompress",
                  "have no compressed form", "before the device is touched", "A 48 | B 96 | C 48", "vv 48 | ww 96 | yy 48 | h 48", "= 480 B"):
        assert words in doc, words
    # the protocol files: Verifier.verify_many_compressed and verify_all_compressed, the second drawing from an rng
    for proto in PROTOCOLS:
        src = re.sub(r"\(\*.*?\*\)", " ", open(os.path.join(ROOT, "ocaml", "%s_mi355x.ml" % proto)).read(), flags=re.S)
        v = src[src.index("module Verifier = struct"):]
        assert re.search(r"let verify_many_compressed\s+\(t\b", v) and "zk_%s_verify_resident_compressed" % proto in v
        assert re.search(r"let verify_all_compressed\s+rng\b", v) and "zk_%s_verify_folded_compressed" % proto in v
        assert "Bytes.length p = %d" % len(WIRE[proto]) in v


def _resident_args(proto, count=1):
    return [u8(bytes(64) * count), u8(WIRE[proto] * count), count]


def _folded_args(proto, count=1, rho=None):
    return [u8(bytes(64) * count), u8(WIRE[proto] * count), u8(RHO[proto] * count if rho is None else rho), count]


@pytest.mark.parametrize("proto", PROTOCOLS)
def test_the_resident_call_answers_as_its_twin(proto):
    """vk_verify's order: the handle first (unknown: ZK_ERR_HANDLE, whatever else is wrong), then count = 0, then null pointers and count > 2^24"""
    lib = _lib.lib()
    for name in ("zk_%s_verify_resident" % proto, "zk_%s_verify_resident_compressed" % proto):
        fn = getattr(lib, name)
        ok, st = (C.c_uint8 * 2)(7, 7), (C.c_int32 * 2)(7, 7)
        okp = C.cast(ok, _lib._P8)
        for handle in (0, ANY):
            assert fn(handle, *_resident_args(proto), okp, st) == ZK_ERR_HANDLE, name
            assert fn(handle, None, None, 0, okp, st) == ZK_ERR_HANDLE, name                       # count = 0 does not excuse it
            assert fn(handle, None, None, 1, None, st) == ZK_ERR_HANDLE, name
            assert fn(handle, *_resident_args(proto)[:2], (1 << 24) + 1, okp, st) == ZK_ERR_HANDLE, name
        assert list(ok) == [7, 7] and list(st) == [7, 7]


@pytest.mark.parametrize("proto", PROTOCOLS)
def test_the_folded_call_answers_as_its_twin(proto):
    """vk_fold's order: what needs no handle first (null pointers, a zero rho, count > 2^24: ZK_ERR_ARG whatever the handle), then the handle -- 0 is
    unknown, and without a GPU any other is ZK_ERR_HIP -- and count = 0 touches nothing but *all_ok"""
    lib = _lib.lib()
    answers = []
    for name in ("zk_%s_verify_folded" % proto, "zk_%s_verify_folded_compressed" % proto):
        fn = getattr(lib, name)
        ok, st = C.c_int(9), (C.c_int32 * 4)(7, 7, 7, 7)
        got = []
        for handle in (0, ANY):
            for hole in (1, 2):
                args = _folded_args(proto)
                args[hole] = None
                got.append(fn(handle, *args, C.byref(ok), st))
            got.append(fn(handle, *_folded_args(proto), None, st))
            got.append(fn(handle, *_folded_args(proto, rho=bytes(len(RHO[proto]))), C.byref(ok), st))
            assert b"rho" in lib.zk_last_error()
            got.append(fn(handle, *_folded_args(proto, 3, rho=RHO[proto] * 2 + RHO[proto][:-16] + bytes(16)), C.byref(ok), st))
            args = _folded_args(proto)
            args[3] = (1 << 24) + 1
            got.append(fn(handle, *args, C.byref(ok), st))
        assert got == [ZK_ERR_ARG] * 12, (name, got)
        assert fn(0, *_folded_args(proto), C.byref(ok), st) == ZK_ERR_HANDLE
        assert fn(0, None, None, None, 0, C.byref(ok), None) == ZK_ERR_HANDLE                        # count = 0 does not excuse it
        want = ZK_ERR_HANDLE if S._gpu_present() else ZK_ERR_HIP                                      # no handle can exist without a device
        assert fn(ANY, *_folded_args(proto), C.byref(ok), st) == want
        assert fn(ANY, None, None, None, 0, C.byref(ok), None) == want
        assert ok.value == 9 and list(st) == [7] * 4
        answers.append(got)
    assert answers[0] == answers[1]


def test_the_hook_refuses_bad_arguments_before_the_device():
    lib = _lib.lib()
    s, out, v = u8(G1C), C.cast((C.c_uint8 * 192)(), _lib._P8), C.cast((C.c_uint8 * 1)(), _lib._P8)
    for args in ((0, None, 1, out, v), (0, s, 1, None, v), (0, s, 1, out, None), (0, s, 0, out, v), (2, s, 1, out, v), (-1, s, 1, out, v)):
        assert lib.zk_selftest_point_decompress(*args) == ZK_ERR_ARG
    if not S._gpu_present():
        assert lib.zk_selftest_point_decompress(0, s, 1, out, v) == ZK_ERR_HIP


# ---------------------------------------------------------------------------------------------------------------- wire.*_proof_bytes_of_json
def _golden_proofs():
    g = json.load(open(os.path.join(GOLDEN, "readme_groth16_key.json")))["proof"]
    g16 = G.Proof(*(bytes.fromhex(g[f]) for f in ("a", "b", "c")))
    p = json.load(open(os.path.join(GOLDEN, "readme_pinocchio_key.json")))
    sizes = [96 * g for _, g in wire._PIN_FIELDS]
    pins = []
    for key in ("proof", "proof_nonzk"):
        raw, off, parts = bytes.fromhex(p[key]), 0, []
        for size in sizes:
            parts.append(raw[off:off + size])
            off += size
        pins.append(PIN.Proof(*parts))
    return g16, pins


def test_proof_bytes_of_json_round_trips_the_golden_proofs(monkeypatch):
    g16, pins = _golden_proofs()
    data = wire.groth16_proof_to_json(g16)
    pdata = [wire.pinocchio_proof_to_json(p) for p in pins]
    want, pwant = g16.to_compressed(), [p.to_compressed() for p in pins]
    text = bytes.fromhex(open(os.path.join(GOLDEN, "readme_groth16_wire.hex")).read().split()[1])
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("proof_bytes_of_json made a library call"))
    got = wire.groth16_proof_bytes_of_json(data)
    assert got == want and len(got) == 192
    assert got == P.g1_compress(P.g1_from_bytes(g16.a)) + P.g2_compress(P.g2_from_bytes(g16.b)) + P.g1_compress(P.g1_from_bytes(g16.c))
    for w, d in zip(pwant, pdata):
        got = wire.pinocchio_proof_bytes_of_json(d)
        assert got == w and len(got) == 480
    # the golden JSON text itself (tests/golden/readme_groth16_wire.hex: pkey, then proof)
    assert wire.groth16_proof_bytes_of_json(text) == want


def test_proof_bytes_of_json_refuses_what_is_not_the_record():
    g16, pins = _golden_proofs()
    c = g16.to_compressed()
    a, b, cc = c[:48], c[48:144], c[144:]
    good = wire.dumps({"a": a, "b": b, "c": cc})
    assert wire.groth16_proof_bytes_of_json(good) == c
    bad = [wire.dumps({"a": a[:47], "b": b, "c": cc}),            # a short string
           wire.dumps({"a": a, "b": b + b"\x00", "c": cc}),       # a long one
           wire.dumps({"a": a, "b": b[:48], "c": cc}),            # a G1 string where a G2 string belongs
           wire.dumps({"a": a, "c": cc}),                         # a missing field
           wire.dumps({"a": a, "b": 5, "c": cc}),                 # not a string
           wire.dumps([a, b, cc]),                                # not a record
           good + b"x", good[:-1]]                                # trailing bytes, a truncated text
    for data in bad:
        with pytest.raises(ValueError):
            wire.groth16_proof_bytes_of_json(data)
    pc = pins[0].to_compressed()
    fields, off = {}, 0
    for f, g in wire._PIN_FIELDS:
        fields[f] = pc[off:off + 48 * g]
        off += 48 * g
    assert wire.pinocchio_proof_bytes_of_json(wire.dumps(fields)) == pc
    for f, _ in wire._PIN_FIELDS:
        with pytest.raises(ValueError):
            wire.pinocchio_proof_bytes_of_json(wire.dumps({k: v for k, v in fields.items() if k != f}))
        with pytest.raises(ValueError):
            wire.pinocchio_proof_bytes_of_json(wire.dumps(dict(fields, **{f: fields[f][:-1]})))
    with pytest.raises(ValueError):
        wire.pinocchio_proof_bytes_of_json(wire.dumps(fields) + b" 1")


# ---------------------------------------------------------------------------------------------------------------- the Python objects
def test_compressed_refuses_a_proof_of_the_wrong_length_before_any_library_call(monkeypatch):
    g16, pins = _golden_proofs()
    rv = G.ResidentVKey(ANY, 2, lambda p: bytes(p.a) + bytes(p.b) + bytes(p.c), 384, "zk_groth16_verify_resident")
    pv = PIN.PinocchioResidentVKey(ANY, 1)
    wires = {id(g16): g16.to_compressed(), id(pins[0]): pins[0].to_compressed()}
    seen = []

    class Lib:
        def __getattr__(self, name):
            def fn(*a):
                if "_verify_" in name:
                    seen.append((name, a[3].value if name.endswith("resident_compressed") else a[4].value))
                return 0
            return fn

    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    for obj, good, n_io in ((rv, g16, 2), (pv, pins[0], 1)):
        io = [list(range(1, n_io + 1))]
        c = wires[id(good)]
        for wrong in (c[:-1], c + b"\x00", (bytes(good.a) + bytes(good.b) + bytes(good.c)) if obj is rv else good.to_bytes(), b""):
            with pytest.raises(ValueError):
                obj.verify_many(io, [wrong], compressed=True)
            with pytest.raises(ValueError):
                obj.verify_all(io, [wrong], compressed=True)
            with pytest.raises(ValueError):
                obj.verify_many(io * 2, [c, wrong], compressed=True)
        if obj is pv:
            with pytest.raises(ValueError):
                obj.verify_many(io, [c])                            # wire bytes without the keyword: not an uncompressed proof
        assert seen == []
        # ... and what is right reaches the compressed entry, as bytes or as a Proof
        obj.verify_many(io * 2, [c, good], compressed=True)
        obj.verify_all(io, [good], compressed=True)
        assert [s[0].split("_", 2)[2] for s in seen] == ["verify_resident_compressed", "verify_folded_compressed"] and [s[1] for s in seen] == [2, 1]
        del seen[:]
        obj.handle = 0
