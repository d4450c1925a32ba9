"""The surface of key generation in one call, without a GPU: the four C prototypes, their EXPORTS entries and ctypes prototypes, the OCaml stubs and
the two OCaml keygen bodies, the argument checks that come before the device is touched, the data fixture of the C host's new leg, and the option
table (no new public option name came with the feature)."""
import ctypes as C
import json
import os
import re

import numpy as np

import option_cases
from zukelang_amd import _lib
from zukelang_amd import r1cs as RC
from zukelang_amd.groth16 import _csr, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
ML = {f: open(os.path.join(ROOT, "ocaml", f)).read() for f in ("mi355x.ml", "groth16_mi355x.ml", "pinocchio_mi355x.ml")}
R = RC.FR_MODULUS
ZK_ERR_ARG, ZK_ERR_SCALAR_RANGE, ZK_ERR_HIP, ZK_ERR_DOMAIN = -1, -3, -5, -8

KEYGEN_ARGS = ("uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t toxic[%d], uint32_t form, "
               "uint8_t* pk_g1, size_t pk_g1_points, uint8_t* pk_g2, size_t pk_g2_points, uint8_t* vk_g1, uint8_t* vk_g2, uint64_t* handle")
PROTOS = {
    "zk_fr_lagrange_at": "int zk_fr_lagrange_at(uint32_t n, uint32_t first, const uint8_t x[32], uint8_t* out, uint8_t z_out[32]);",
    "zk_groth16_keygen": "int zk_groth16_keygen(" + KEYGEN_ARGS % 160 + ");",
    "zk_pinocchio_keygen": "int zk_pinocchio_keygen(" + KEYGEN_ARGS % 256 + ");",
    "zk_pinocchio_pk_upload_lagrange": "int zk_pinocchio_pk_upload_lagrange(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, "
                                       "const uint8_t* pk_g1, size_t pk_g1_points, const uint8_t* pk_g2, size_t pk_g2_points, const uint8_t* h_lagrange, uint64_t* handle);",
}


def _flat(src):
    """C source without comments, whitespace runs folded"""
    return " ".join(re.sub(r"/\*.*?\*/", " ", src, flags=re.S).split())


def _ml_code(src):
    out, depth, i = [], 0, 0
    while i < len(src):
        if src.startswith("(*", i):
            depth += 1; i += 2
        elif src.startswith("*)", i) and depth:
            depth -= 1; i += 2
        else:
            if not depth:
                out.append(src[i])
            i += 1
    return "".join(out)


def test_prototypes_exports_and_forms():
    flat = _flat(HEADER).replace("( ", "(").replace(" )", ")").replace(" ,", ",")
    for name, proto in PROTOS.items():
        assert proto in flat, name
        assert name in _lib.EXPORTS, name
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in PROTOS)
    assert re.search(r"#define ZK_KEY_FORM_TAU_POWERS 0\b", HEADER) and re.search(r"#define ZK_KEY_FORM_LAGRANGE\s+1\b", HEADER)
    assert _lib.KEY_FORMS == {"tau_powers": 0, "lagrange": 1}
    # every entry cites the reference lines it replaces
    for cite in ("groth16.ml:45-108", "pinocchio.ml:77-189", "QAP.ml:84"):
        assert cite in HEADER


def _c_kind(param):
    p = re.sub(r"\[[^\]]*\]", "*", param)
    if "zk_csr" in p:
        return "csr"
    if "uint64_t" in p and "*" in p:
        return "u64p"
    if "*" in p:
        return "u8p"
    return next(t for t in ("uint32_t", "size_t") if t in p)


def test_ctypes_prototypes_agree_with_the_header():
    kinds = {_lib._P8: "u8p", _lib._PCSR: "csr", _lib._PH: "u64p", C.c_uint32: "uint32_t", C.c_size_t: "size_t"}
    assert set(_lib.PROTOTYPES) == set(PROTOS)
    lib = _lib.lib()
    for name, proto in PROTOS.items():
        params = [p.strip() for p in proto[proto.index("(") + 1:proto.rindex(")")].split(",")]
        assert [kinds[a] for a in _lib.PROTOTYPES[name]] == [_c_kind(p) for p in params], name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name] and getattr(lib, name).restype is C.c_int


def test_ocaml_stubs_agree_with_the_header():
    code = _ml_code(ML["mi355x.ml"])
    ml_kind = {"uint32_t": "uint32_t", "size_t": "size_t", "ocaml_bytes": "u8p", "ptr csr": "csr", "ptr uint64_t": "u64p"}
    for name, proto in PROTOS.items():
        m = re.search(r"let\s+%s\s*=\s*fn\s+\"%s\"\s*\((.*?)returning int\)" % (name, name), code, flags=re.S)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split("@->")][:-1]
        params = [p.strip() for p in proto[proto.index("(") + 1:proto.rindex(")")].split(",")]
        assert [ml_kind[a] for a in args] == [_c_kind(p) for p in params], name
    assert re.search(r"let key_form_tau_powers = 0\b", code) and re.search(r"let key_form_lagrange = 1\b", code)


def _keygen_body(src):
    code = _ml_code(src)
    start = code.index("  let keygen ")
    nxt = re.search(r"\n  let \w", code[start + 5:])
    return code[start:start + 5 + nxt.start()]


def test_ocaml_keygen_bodies_make_one_library_call():
    for f, sym in (("groth16_mi355x.ml", "zk_groth16_keygen"), ("pinocchio_mi355x.ml", "zk_pinocchio_keygen")):
        body = _keygen_body(ML[f])
        assert body.count(sym) == 1, f
        assert "Poly.apply" not in body and "of_fr_many" not in body and "upload" not in body, f
        assert "key_form_lagrange" in body and "Handles.replace handles pkey h" in body, f
        assert "Gc.finalise" in body, f
        # matrices_of_qap keeps its Poly.apply: it builds the CSR for keys read from JSON
        code = _ml_code(ML[f])
        mq = code[code.index("let matrices_of_qap"):]
        assert "Poly.apply" in mq[:mq.index("\n  let ", 5)], f
        assert "derive_lagrange_on_upload" in code
        # several entries in the device list (Mi355x.use_all_devices before keygen): no handle is asked for, the bytes are registered as the keys read from
        # JSON are, which shards them over the list behind one handle -- keygen keeps working there
        assert re.search(r"\| None ->\s*ignore \(register vars \(l, r, o\) n pkey\)", body), f
        assert re.search(r"let register = upload\b", code), f
        assert "register_circuit" not in code, f
    stubs = _ml_code(ML["mi355x.ml"])
    call = stubs[stubs.index("let keygen_call"):]
    call = call[:call.index("\nlet ", 5)]
    assert re.search(r"let want_handle = device_list_length \(\) <= 1 in", call)
    assert re.search(r"if want_handle then h else from_voidp uint64_t null", call) and re.search(r"if want_handle then Some !@h else None", call)
    assert re.search(r"let device_list_length \(\) =.*?zk_get_device_list", stubs, flags=re.S)
    g = _keygen_body(ML["groth16_mi355x.ml"])
    assert re.search(r"fr_bytes \[ alpha; beta; gamma; delta; tau \]", g) and "Pairing.pairing pkey.a pkey.b2" in g
    p = _keygen_body(ML["pinocchio_mi355x.ml"])
    assert re.search(r"fr_bytes \[ rv; rw; s; av; aw; ay; b; gm \]", p)


def _call(fn, cs, toxic, form=1, counts=None, nulls=(), handle=True, n=None):
    nm = int(np.count_nonzero(cs.mid))
    if fn.__name__ == "zk_groth16_keygen":
        c1, c2 = 3 + (cs.n + 2) + (cs.n - 1) + nm, 2 + cs.n + 2
    else:
        c1, c2 = 5 * nm + (cs.n + 1) + 2 * cs.m + 7, 2 * nm + (cs.n + 1) + 2
    if counts:
        c1, c2 = c1 + counts[0], c2 + counts[1]
    g1, g2 = np.zeros(96 * max(c1, 1), dtype=np.uint8), np.zeros(192 * max(c2, 1), dtype=np.uint8)
    mid = np.ascontiguousarray(cs.mid, dtype=np.uint8)
    A, B, Cc = _csr(cs.L), _csr(cs.R), _csr(cs.O)
    t = np.frombuffer(bytes(toxic), dtype=np.uint8).copy()
    h = C.c_uint64()
    args = [cs.n if n is None else n, cs.m, C.byref(A), C.byref(B), C.byref(Cc), _p(mid), _p(t), form, _p(g1), c1, _p(g2), c2, None, None, C.byref(h) if handle else None]
    for i in nulls:
        args[i] = None
    return fn(*args)


def test_argument_checks_come_before_the_device():
    """null arguments, an unknown form, wrong point counts and a bad trapdoor are refused with their own codes whether or not a GPU is there; a call
    that passes them needs the device (ZK_ERR_HIP without one: the MI355X path has no CPU fallback)."""
    L = _lib.lib()
    cs, _w = RC.iterated_cubic(6, 9)
    st = RC.fr_stream(0x5A)
    for fn, ntox in ((L.zk_groth16_keygen, 5), (L.zk_pinocchio_keygen, 8)):
        tox = [next(st) for _ in range(ntox)]
        ok = bytes(RC.fr_bytes(tox))
        for i in (2, 3, 4, 5, 6):
            assert _call(fn, cs, ok, nulls=(i,)) == ZK_ERR_ARG, (fn.__name__, i)
        assert _call(fn, cs, ok, form=2) == ZK_ERR_ARG
        assert _call(fn, cs, ok, n=0) == ZK_ERR_ARG
        assert _call(fn, cs, ok, counts=(1, 0)) == ZK_ERR_DOMAIN
        assert _call(fn, cs, ok, counts=(0, -1)) == ZK_ERR_DOMAIN
        for i in range(ntox):
            bad = list(tox); bad[i] = R + 1
            assert _call(fn, cs, b"".join(x.to_bytes(32, "little") for x in bad)) == ZK_ERR_SCALAR_RANGE, (fn.__name__, i)
        if ntox == 5:
            for i in (2, 3):                                              # gamma = 0, delta = 0: the reference divides by them
                bad = list(tox); bad[i] = 0
                assert _call(fn, cs, bytes(RC.fr_bytes(bad))) == ZK_ERR_ARG
        if L.zk_device_count() == 0:
            assert _call(fn, cs, ok) == ZK_ERR_HIP
            assert _call(fn, cs, ok, handle=False) == ZK_ERR_HIP
    x = RC.fr_bytes([7])
    out = np.zeros(64, dtype=np.uint8)
    assert L.zk_fr_lagrange_at(2, 0, None, _p(out), None) == ZK_ERR_ARG
    assert L.zk_fr_lagrange_at(0, 0, _p(x), _p(out), None) == ZK_ERR_ARG
    assert L.zk_fr_lagrange_at(2, 0, _p(np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8).copy()), _p(out), None) == ZK_ERR_SCALAR_RANGE
    # zk_pinocchio_pk_upload_lagrange: null first, then the device
    mid = np.ascontiguousarray(cs.mid, dtype=np.uint8)
    A, B, Cc = _csr(cs.L), _csr(cs.R), _csr(cs.O)
    g = np.zeros(192 * 64, dtype=np.uint8)
    h = C.c_uint64()
    assert L.zk_pinocchio_pk_upload_lagrange(cs.n, cs.m, C.byref(A), C.byref(B), C.byref(Cc), _p(mid), _p(g), 1, _p(g), 1, None, C.byref(h)) == ZK_ERR_ARG
    assert L.zk_pinocchio_pk_upload_lagrange(cs.n, cs.m, C.byref(A), C.byref(B), C.byref(Cc), _p(mid), _p(g), 1, _p(g), 1, _p(g), None) == ZK_ERR_ARG
    if L.zk_device_count() == 0:
        assert L.zk_fr_lagrange_at(2, 0, _p(x), _p(out), None) == ZK_ERR_HIP
        assert L.zk_pinocchio_pk_upload_lagrange(cs.n, cs.m, C.byref(A), C.byref(B), C.byref(Cc), _p(mid), _p(g), 1, _p(g), 1, _p(g), C.byref(h)) == ZK_ERR_HIP


def test_python_surface():
    import inspect
    from zukelang_amd import pinocchio as PIN
    from zukelang_amd.groth16 import Groth16
    assert list(inspect.signature(Groth16.generate).parameters) == ["rng", "circuit", "form"]
    assert inspect.signature(Groth16.generate).parameters["form"].default == "lagrange"
    assert list(inspect.signature(PIN.generate).parameters)[:3] == ["rng", "circuit", "form"]
    for cls in (PIN.ZK, PIN.NonZK):
        assert list(inspect.signature(cls.generate).parameters) == ["rng", "circuit", "form"]
        assert list(inspect.signature(cls.from_lagrange).parameters) == ["circuit", "pkey", "h_lagrange"]
        assert "lagrange" in inspect.signature(cls.__init__).parameters
    # the host-side keygen functions stay as they were (bench.py and the older tests use them)
    assert list(inspect.signature(Groth16.keygen).parameters) == ["rng", "circuit", "lagrange"]
    assert list(inspect.signature(PIN.keygen).parameters) == ["rng", "circuit"]


def test_h_lagrange_fixture_is_first_principles_and_the_header_is_the_json():
    """tests/golden/readme_pinocchio_h_lagrange.json (make_readme_pinocchio_lagrange.py): [lambda_t(s)] (n-1) | [Z(s)] for the README key -- its
    exponents against the product formula, its points against the oracle and against the derived pool of the key's own fixture, and
    examples/readme_pinocchio_lagrange_fixture.h byte for byte."""
    import oracle_lib as O
    from oracle import pyref as P
    gold = os.path.join(ROOT, "tests", "golden")
    fix = json.load(open(os.path.join(gold, "readme_pinocchio_h_lagrange.json")))
    key = json.load(open(os.path.join(gold, "readme_pinocchio_key.json")))
    n, s = fix["n"], int(key["toxic"][2], 16)
    assert n == 3
    ex = [int(x, 16) for x in fix["exponents"]]
    pts = list(range(n, 2 * n - 1))
    for i, xi in enumerate(pts):
        num = den = 1
        for xj in pts:
            if xj != xi:
                num, den = num * (s - xj) % R, den * (xi - xj) % R
        assert ex[i] == num * pow(den, R - 2, R) % R
    assert ex[n - 1] == s * (s - 1) * (s - 2) % R
    assert [O.g1_mul(O.g1_generator(), P.fr_to_bytes(e)).hex() for e in ex] == fix["h_lagrange_g1"] == key["derived_h_pool_g1"][:n]
    h = open(os.path.join(ROOT, "examples", "readme_pinocchio_lagrange_fixture.h")).read()
    m = re.search(r"static const uint8_t PFIX_H_LAGRANGE\[(\d+)\] = \{([^}]*)\};", h)
    assert int(m.group(1)) == 96 * n and bytes(int(x) for x in m.group(2).split(",")).hex() == "".join(fix["h_lagrange_g1"])
    src = open(os.path.join(ROOT, "examples", "c_pinocchio.c")).read()
    assert "zk_pinocchio_pk_upload_lagrange" in src and "PFIX_H_LAGRANGE" in src


def test_no_new_public_option():
    names = option_cases.public_options()
    assert len(names) == 28 and not any("KEYGEN" in n or "KEY_FORM" in n for n in names)
    src = open(os.path.join(ROOT, "zukelang_amd", "csrc", "keygen.hip")).read()
    assert not option_cases.OPTION_READ.search(src) and "getenv" not in src          # ZK_PIN_COMPACT_H / ZK_PIN_SHARED_SORT through pinocchio.hip's helpers
