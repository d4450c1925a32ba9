"""zk_groth16_pk_contribute and zk_selftest_g1_scale without a GPU: include/zkmi355x.h, _lib.EXPORTS, _lib.CONTRIBUTE_PROTOTYPES, the built library and the
OCaml files name the same calls with the same argument lists; every refusal that needs no handle comes before the device is touched, in the header's
order; a box without a GPU answers ZK_ERR_HIP; the constants restated for the host are those of their sources; and the name of the call
stays out of the words tests/option_cases.py routes on."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from zukelang_amd import _lib
from zukelang_amd import groth16 as G16
from zukelang_amd.groth16 import Groth16, VKey
from zukelang_amd.r1cs import FR_MODULUS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import option_cases as OC
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zukelang_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
CALL, HOOK = "zk_groth16_pk_contribute", "zk_selftest_g1_scale"
WANT = {CALL: ["uint64_t", "ptr", "ptr", "ptr", "ptr"], HOOK: ["ptr", "size_t", "ptr", "uint32_t", "ptr"]}
ARG, RANGE, HIP, HANDLE = -1, -3, -5, -7


def _header_kinds(name):
    body = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, body)
    assert m, "%s is not declared in include/zkmi355x.h" % name
    out = []
    for p in m.group(1).split(","):
        p = re.sub(r"\[[^\]]*\]", "*", p)
        out.append("ptr" if "*" in p else next(t for t in ("uint64_t", "uint32_t", "size_t", "int") if re.search(r"\b%s\b" % t, p)))
    return out


def test_the_calls_are_declared_exported_and_bound():
    lib = _lib.lib()
    kinds = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "size_t": C.c_size_t, "ptr": _lib._P8}
    assert set(_lib.CONTRIBUTE_PROTOTYPES) == set(WANT)
    for name, want in WANT.items():
        assert _header_kinds(name) == want, name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert _lib.CONTRIBUTE_PROTOTYPES[name] == [kinds[k] for k in want], name
        assert getattr(lib, name).argtypes == _lib.CONTRIBUTE_PROTOTYPES[name] and getattr(lib, name).restype is C.c_int
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    assert 'fn "%s" (uint64_t @-> ptr char @-> ptr char @-> ptr char @-> ptr char @-> returning int)' % CALL in ml and "let groth16_pk_contribute" in ml
    g = open(os.path.join(ROOT, "ocaml", "groth16_mi355x.ml")).read()
    assert "let contribute" in g and "Mi355x.groth16_pk_contribute" in g
    assert callable(Groth16.contribute) and callable(VKey.with_delta) and callable(G16.verify_contributions)


def test_the_name_holds_no_routed_word():
    for word in OC.ROUTED_WORDS:
        assert word not in CALL and word not in HOOK, (
            "tests/test_option_cases.py asks every header call whose name holds %r for a row of option_cases.ROUTES; that table is an existing test "
            "file and cannot gain a row here, so the promise behind it -- no public option changes a contributed key or its proofs -- is kept by "
            "tests/test_gpu_contribute_options.py instead, and the name must stay out of the routed words" % word)
    assert os.path.exists(os.path.join(ROOT, "tests", "test_gpu_contribute_options.py"))


def _p8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _fr(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint8).copy()


def test_argument_errors_of_the_call_come_before_the_device_in_the_headers_order():
    lib = _lib.lib()
    fn = getattr(lib, CALL)
    h = C.c_uint64(0x7777)          # no key was ever uploaded in this process
    link, dg2, vkd = (np.full(192, 0x5a, dtype=np.uint8) for _ in range(3))
    assert fn(h, None, _p8(link), _p8(dg2), _p8(vkd)) == ARG
    assert b"pk_contribute" in lib.zk_last_error() and b"null dmul" in lib.zk_last_error()
    assert fn(h, _p8(_fr(0)), _p8(link), _p8(dg2), _p8(vkd)) == ARG
    assert b"delta' = 0" in lib.zk_last_error()
    for big in (FR_MODULUS, FR_MODULUS + 1, (1 << 256) - 1):
        assert fn(h, _p8(_fr(big)), _p8(link), _p8(dg2), _p8(vkd)) == RANGE, hex(big)
    # valid arguments, a handle that does not exist: ZK_ERR_HANDLE where a device answers, ZK_ERR_HIP on a box without one
    want = HANDLE if lib.zk_device_count() > 0 else HIP
    for k in (1, 2, FR_MODULUS - 1):
        assert fn(h, _p8(_fr(k)), _p8(link), _p8(dg2), _p8(vkd)) == want
        assert fn(h, _p8(_fr(k)), None, None, None) == want          # the three outputs are optional
    for out in (link, dg2, vkd):
        assert (out == 0x5a).all()          # a refused call writes nothing


def test_argument_errors_of_the_hook_come_before_the_device():
    lib = _lib.lib()
    fn = getattr(lib, HOOK)
    pts, out = np.zeros(96 * 3, dtype=np.uint8), np.full(96 * 3, 0x5a, dtype=np.uint8)
    k = _fr(5)
    assert fn(None, 3, _p8(k), 0, _p8(out)) == ARG
    assert fn(_p8(pts), 3, None, 0, _p8(out)) == ARG
    assert fn(_p8(pts), 3, _p8(k), 0, None) == ARG
    assert fn(_p8(pts), 0, _p8(k), 0, _p8(out)) == ARG
    assert b"zk_selftest_g1_scale" in lib.zk_last_error()
    for big in (FR_MODULUS, (1 << 256) - 1):
        assert fn(_p8(pts), 3, _p8(_fr(big)), 64, _p8(out)) == ARG, hex(big)
    assert b"k >= r" in lib.zk_last_error()
    if lib.zk_device_count() == 0:
        assert fn(_p8(pts), 3, _p8(k), 0, _p8(out)) == HIP
        assert fn(_p8(pts), 3, _p8(_fr(0)), 64, _p8(out)) == HIP          # k = 0 is served
    assert (out == 0x5a).all()


def test_the_python_layer_checks_before_it_calls():
    prover = Groth16.__new__(Groth16)          # no handle: the arguments are looked at before anything is called
    prover.handle = None
    for bad in (-1, 1 << 256):
        with pytest.raises(ValueError, match="contribute: dmul is an element of Fr"):
            prover.contribute(bad)
    vk = VKey(b"\x01" * 96, np.zeros(96, dtype=np.uint8), b"\x02" * 192, b"\x03" * 192, b"\x04" * 192, b"\x05" * 576)
    new = vk.with_delta(b"\x09" * 192)
    assert new.d == b"\x09" * 192 and vk.d == b"\x04" * 192
    assert (new.one1, new.one2, new.gm, new.ab) == (vk.one1, vk.one2, vk.gm, vk.ab) and new.ltgm_io is vk.ltgm_io
    with pytest.raises(ValueError, match="with_delta"):
        vk.with_delta(b"\x09" * 96)
    # what verify_contributions refuses without a pairing: lengths, the identity, a chain that does not start or end where it should
    g = pyref.g1_to_bytes(pyref.G1)
    assert G16.verify_contributions(g, [], g) is True
    assert G16.verify_contributions(g, [], pyref.g1_to_bytes(pyref.pt_mul(pyref.G1, 2))) is False
    assert G16.verify_contributions(bytes(96), [], bytes(96)) is False
    assert G16.verify_contributions(g, [(bytes(96), g, bytes(192))], g) is False
    assert G16.verify_contributions(g, [(g, g[:95], bytes(192))], g) is False


def test_the_restated_constants_are_those_of_their_sources():
    scalar_h = open(os.path.join(CSRC, "contribute_scalar.h")).read()
    r64 = [int(x, 16) for x in re.findall(r"0x([0-9a-f]+)ull", re.search(r"CS_R\[4\] = \{([^}]*)\}", scalar_h).group(1))]
    assert sum(w << (64 * i) for i, w in enumerate(r64)) == pyref.R == FR_MODULUS
    assert G16._G2_ONE == pyref.g2_to_bytes(pyref.G2) and G16._FP_MODULUS == pyref.P
    p = pyref.pt_mul(pyref.G1, 7)
    assert G16._g1_negate(pyref.g1_to_bytes(p)) == pyref.g1_to_bytes(pyref.pt_neg(p))


def test_the_call_runs_on_the_derivations_kernels_unchanged():
    """the measurement ruled the call's own kernel out: contribute.hip adds a table of equal scalars and the slabs, no group law of its
    own, and reaches the multiplication through the one host function lagrange_derive.hip gained"""
    text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "contribute.hip")).read())
    assert "points_scale_tabmul(CURVE_G1" in text and "lagrange_derive.hip" not in text
    assert not re.search(r"\b(jac_\w+|window_table\w*|xyzz_\w+|fe_mul|fe_sqr|fe_inv\w*)\s*\(", text)
    assert re.findall(r"__global__[^(]*\b(\w+)\s*\(", text) == ["k_scalar_table"]
    derive = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "lagrange_derive.hip")).read())
    body = derive[derive.index("static int scale_affine_tabmul("):derive.index("int points_scale_tabmul(")]
    for k in ("k_aff_to_raw<T>", "g_tabmul<T>", "k_raw_to_aff<T>"):
        assert k in body, k


def test_the_documents_point_to_the_call():
    for text in ("a delta contribution to a resident key", "RATIO of two delta", "Timer family contribute", "profiles/contribute_kernel_ab.json"):
        assert text in HEADER, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "2q" in design and CALL in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert CALL in open(os.path.join(ROOT, doc)).read(), doc
    assert "Contribution round trip" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
