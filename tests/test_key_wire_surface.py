"""Keys and base lists in wire form, without a GPU: include/zkmi355x.h, _lib.EXPORTS, _lib.KEY_WIRE_PROTOTYPES and the OCaml stubs name the same five
calls with the same argument lists; the argument checks that come before the device is touched; the JSON readers that hand the record's compressed
strings over as they stand (no square root, no library call) against the host decoder; and that the reference cases the GPU test builds its
rejections from (tests/encoding_cases.py) cover every kind of refusal for both groups."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import encoding_cases as E
from oracle import pyref as P
from zukelang_amd import _lib, wire, r1cs as RC
from zukelang_amd.curve import G1, G2
from zukelang_amd.groth16 import _csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()

UPLOAD = ["uint32_t", "uint32_t", "ptr", "ptr", "ptr", "ptr", "ptr", "size_t", "ptr", "size_t"]
WANT = {
    "zk_groth16_pk_upload_compressed": UPLOAD + ["uint32_t", "ptr"],
    "zk_pinocchio_pk_upload_compressed": UPLOAD + ["ptr", "ptr"],
    "zk_bases_upload_compressed": ["int", "ptr", "size_t", "ptr"],
    "zk_groth16_pool_points_compressed": ["uint64_t", "int", "ptr", "size_t", "ptr"],
    "zk_pinocchio_pool_points_compressed": ["uint64_t", "int", "ptr", "size_t", "ptr"],
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


def test_the_five_calls_are_declared_exported_and_bound():
    lib = _lib.lib()
    kinds = {C.c_uint32: "uint32_t", C.c_uint64: "uint64_t", C.c_size_t: "size_t", C.c_int: "int"}
    assert set(_lib.KEY_WIRE_PROTOTYPES) == set(WANT)
    for name, want in WANT.items():
        assert _header_kinds(name) == want, name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        # (ctypes has ONE class for uint64_t and size_t on this ABI: the two compare as one kind)
        assert [kinds.get(a, "ptr") for a in _lib.KEY_WIRE_PROTOTYPES[name]] == [kinds[C.c_uint64] if w == "uint64_t" else w for w in want], name
        assert getattr(lib, name).argtypes == _lib.KEY_WIRE_PROTOTYPES[name] and getattr(lib, name).restype is C.c_int
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    for name in WANT:
        assert 'fn "%s"' % name in ml, name
    for f in ("groth16_mi355x.ml", "pinocchio_mi355x.ml"):
        assert "let upload_compressed" in open(os.path.join(ROOT, "ocaml", f)).read(), f
    # the header says what differs from the uncompressed uploads
    assert "C0 00 .. 00 and nothing else" in HEADER and "curve.ml:199-219" in HEADER


def _readme_groth16():
    cs, _ = RC.readme_circuit(3)
    g1, g2, _ = wire.groth16_pkey_bytes_of_json(bytes.fromhex(open(os.path.join(GOLDEN, "readme_groth16_wire.hex")).read().split()[0]))
    return cs, np.frombuffer(g1, dtype=np.uint8), np.frombuffer(g2, dtype=np.uint8)


def test_argument_checks_come_before_the_device():
    """Null L / R / O / mid / pools / handle and an unknown form are ZK_ERR_ARG; with valid arguments a box without a GPU answers ZK_ERR_HIP."""
    lib = _lib.lib()
    cs, g1, g2 = _readme_groth16()
    L, R, O = _csr(cs.L), _csr(cs.R), _csr(cs.O)
    mid = np.ascontiguousarray(cs.mid, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    h = C.c_uint64(0)
    good = [cs.n, cs.m, C.byref(L), C.byref(R), C.byref(O), p(mid), p(g1), len(g1) // 48, p(g2), len(g2) // 96]
    for i in (2, 3, 4, 5, 6, 8):
        bad = list(good)
        bad[i] = None
        assert lib.zk_groth16_pk_upload_compressed(*bad, 0, C.byref(h)) == -1, i
        assert lib.zk_pinocchio_pk_upload_compressed(*bad, None, C.byref(h)) == -1, i
    assert lib.zk_groth16_pk_upload_compressed(*good, 0, None) == -1
    assert lib.zk_pinocchio_pk_upload_compressed(*good, None, None) == -1
    assert lib.zk_groth16_pk_upload_compressed(*good, 2, C.byref(h)) == -1          # neither ZK_KEY_FORM_TAU_POWERS nor ZK_KEY_FORM_LAGRANGE
    assert lib.zk_bases_upload_compressed(0, None, 3, C.byref(h)) == -1
    assert lib.zk_bases_upload_compressed(0, p(g1), 3, None) == -1
    assert lib.zk_bases_upload_compressed(2, p(g1), 3, C.byref(h)) == -1
    assert lib.zk_bases_upload_compressed(0, p(g1), 0, C.byref(h)) == -1
    assert h.value == 0
    if lib.zk_device_count() > 0:
        return          # the rest is the answer of a box WITHOUT a GPU; with one, tests/test_gpu_key_wire.py runs the calls
    cnt = C.c_size_t(0)
    assert lib.zk_groth16_pk_upload_compressed(*good, 0, C.byref(h)) == -5
    assert lib.zk_groth16_pk_upload_compressed(*good, 1, C.byref(h)) == -5
    assert lib.zk_pinocchio_pk_upload_compressed(*good, None, C.byref(h)) == -5
    assert lib.zk_bases_upload_compressed(0, p(g1), 3, C.byref(h)) == -5
    assert lib.zk_bases_upload_compressed(1, p(g2), 3, C.byref(h)) == -5
    assert h.value == 0
    # no key can exist here: the read-backs answer ZK_ERR_HANDLE
    assert lib.zk_groth16_pool_points_compressed(C.c_uint64(1), 1, None, 0, C.byref(cnt)) == -7
    assert lib.zk_pinocchio_pool_points_compressed(C.c_uint64(1), 0, None, 0, C.byref(cnt)) == -7
    assert lib.zk_pinocchio_pool_points_compressed(C.c_uint64(1), 8, None, 0, C.byref(cnt)) == -1


def test_groth16_reader_hands_over_the_strings_the_host_decoder_reads():
    js = bytes.fromhex(open(os.path.join(GOLDEN, "readme_groth16_wire.hex")).read().split()[0])
    g1, g2, mids = wire.groth16_pkey_bytes_of_json(js)
    pk, mids2 = wire.groth16_pkey_of_json(js)          # the host decoder: 13 + 7 points, below BATCH_MIN
    assert mids == mids2 == [("c", 4), ("c", 5), ("input", 3)]
    assert g1 == G1.to_compressed_bytes_many(pk.g1) and g2 == G2.to_compressed_bytes_many(pk.g2)
    assert len(g1) == 48 * 13 and len(g2) == 96 * 7


def _pinocchio_json():
    import json
    from zukelang_amd.pinocchio import PKey
    fix = json.load(open(os.path.join(GOLDEN, "readme_pinocchio_key.json")))
    cat = lambda xs: b"".join(bytes.fromhex(x) for x in xs)
    pk = PKey(np.frombuffer(cat(fix["pk_g1"]), dtype=np.uint8), np.frombuffer(cat(fix["pk_g2"]), dtype=np.uint8))
    cs, _ = RC.readme_circuit(3)
    all_vars = [("v", i) for i in range(cs.m)]          # any names in Var order: the reader keeps them, the pools do not depend on them
    mid_vars = [v for v, is_mid in zip(all_vars, cs.mid) if is_mid]
    return pk, wire.pinocchio_pkey_to_json(pk, cs.n, mid_vars, all_vars), mid_vars


def test_pinocchio_reader_hands_over_the_strings_the_host_decoder_reads():
    pk, js, mid_vars = _pinocchio_json()
    g1, g2, mids = wire.pinocchio_pkey_bytes_of_json(js)
    pk2, n, mids2, _ = wire.pinocchio_pkey_of_json(js)
    assert mids == mids2 == mid_vars and n == 3
    assert bytes(pk2.g1) == bytes(pk.g1) and bytes(pk2.g2) == bytes(pk.g2)
    assert g1 == G1.to_compressed_bytes_many(pk.g1) and g2 == G2.to_compressed_bytes_many(pk.g2)


def test_readers_refuse_wrong_shapes_like_the_other_readers():
    js = bytes.fromhex(open(os.path.join(GOLDEN, "readme_groth16_wire.hex")).read().split()[0])
    doc = wire.loads(js)
    for path, value, what in ((("a",), doc["a"][:47], "48 bytes"), (("b2",), doc["b2"] + b"\0", "96 bytes"), (("ti1", 2), 7, "JSON string"),
                              (("ltd_mid", 0, 1), doc["b2"], "48 bytes"), (("ti2", 4), doc["a"], "96 bytes")):
        with pytest.raises(ValueError, match=what):
            wire.groth16_pkey_bytes_of_json(wire.dumps(E.replaced(doc, path, value)))
    with pytest.raises(ValueError, match="not a groth16_pkey_bytes record"):
        wire.groth16_pkey_bytes_of_json(wire.dumps({k: v for k, v in doc.items() if k != "tiztd"}))
    with pytest.raises(ValueError, match="not a groth16_pkey_bytes record"):
        wire.groth16_pkey_bytes_of_json(b"[1,2]")
    with pytest.raises(ValueError):
        wire.groth16_pkey_bytes_of_json(js[:-3])
    _, pjs, _ = _pinocchio_json()
    pdoc = wire.loads(pjs)
    for path, value, what in ((("vt",), pdoc["vt"][:1], "48 bytes"), (("wt",), pdoc["vt"], "96 bytes"), (("si", 1), 3, "JSON string"),
                              (("ww", 0, 1), pdoc["vt"], "96 bytes")):
        with pytest.raises(ValueError, match=what):
            wire.pinocchio_pkey_bytes_of_json(wire.dumps(E.replaced(pdoc, path, value)))
    with pytest.raises(ValueError, match="not a pinocchio_pkey_bytes record"):
        wire.pinocchio_pkey_bytes_of_json(wire.dumps({k: v for k, v in pdoc.items() if k != "si2"}))
    # a point string of the right shape is NOT looked into here: the device decides
    zero = E.replaced(doc, ("a",), bytes(48))
    assert wire.groth16_pkey_bytes_of_json(wire.dumps(zero))[0][:48] == bytes(48)


def test_the_reference_cases_cover_every_refusal_for_both_groups():
    """tests/test_gpu_key_wire.py places every flags / range / curve case at three positions of a list and expects pyref's verdict: the cases alone must
    hold all three kinds of refusal, for G1 and for G2 (pyref decides, nothing of the product is asked)."""
    for group in (1, 2):
        seen = {v for c, v, _ in E.matrix(group, True) if c.kind in ("flags", "range", "curve")}
        assert {P.BAD_ENCODING, P.NOT_ON_CURVE, P.NOT_IN_SUBGROUP} <= seen, (group, seen)
        assert P.OK not in seen, "a refusal case that pyref accepts"
        # the uncompressed uploads' zero-string identity has no compression flag: a bad encoding on the wire
        assert (P.g1_decompress if group == 1 else P.g2_decompress)(bytes(48 * group))[0] == P.BAD_ENCODING
