"""zk_selftest_group without a GPU: include/zkmi355x.h, _lib.EXPORTS and _lib.GROUP_PROTOTYPES name the same call with the same argument list; every
refusal comes before the device; a valid call is ZK_ERR_HIP here (no CPU fallback); and the form table of tests/group_law_cases.py names every
function of the group law that csrc/ defines, so that a form added later must join the battery.  What the forms compute: tests/test_gpu_group_law.py."""
import ctypes as C
import glob
import os
import re

import pytest

import group_law_cases as GL
from oracle import pyref as P
from zukelang_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zukelang_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
ZK_ERR_ARG, ZK_ERR_SCALAR_RANGE, ZK_ERR_HIP = -1, -3, -5
WANT = {"zk_selftest_group": ["int", "int", "int", "u8p", "u8p", "size_t", "u8p"]}

u8 = lambda b: C.cast(C.c_char_p(b), _lib._P8)


def test_header_exports_and_ctypes_agree():
    body = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    kinds = {_lib._P8: "u8p", C.c_size_t: "size_t", C.c_int: "int"}
    lib = _lib.lib()
    for name, want in WANT.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, body)
        assert m, "%s is not declared in include/zkmi355x.h" % name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert ["u8p" if "*" in p else next(t for t in ("size_t", "int") if re.search(r"\b%s\b" % t, p)) for p in params] == want
        assert all("const" in p for p in params[3:5]) and "const" not in params[6]          # a and b are read, out is written
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert [kinds[a] for a in _lib.GROUP_PROTOTYPES[name]] == want
        assert getattr(lib, name).argtypes == _lib.GROUP_PROTOTYPES[name] and getattr(lib, name).restype is C.c_int
    assert set(_lib.GROUP_PROTOTYPES) == set(WANT)
    assert ZK_ERR_SCALAR_RANGE == int(re.search(r"#define ZK_ERR_SCALAR_RANGE \((-?\d+)\)", HEADER).group(1))
    # the header's list of forms is the table's
    comment = HEADER[HEADER.index("Every form of the device's group law"):HEADER.index("int zk_selftest_group")]
    for f in GL.FORMS.values():
        assert f.function in comment and re.search(r"\b%d\b" % f.number, comment), f
    assert sorted(f.number for f in GL.FORMS.values()) == list(range(len(GL.FORMS)))
    msm = open(os.path.join(CSRC, "msm.cuh")).read()
    assert int(re.search(r"GROUP_FORM_COUNT\s*=\s*(\d+)", msm).group(1)) == len(GL.FORMS)


def _operands(group):
    g = GL.Group(group)
    one = g.const(1)
    pt = g.gen
    return g, g.xyzz_bytes((pt[0], pt[1], one, one)), g.aff_bytes(pt)


def test_every_refusal_comes_before_the_device():
    lib = _lib.lib()
    call = lib.zk_selftest_group
    for group in (0, 1):
        g, a, q = _operands(group)
        fb = 96 if group else 48
        out = C.create_string_buffer(b"\x09" * (2 * fb), 2 * fb)
        o8 = C.cast(out, _lib._P8)
        add, madd, table, dbl, mul = (GL.FORMS[n].number for n in ("add", "madd", "madd_table", "dbl", "mul"))
        assert call(group, add, 0, None, u8(a), 1, o8) == ZK_ERR_ARG
        assert call(group, add, 0, u8(a), None, 1, o8) == ZK_ERR_ARG                 # an addition reads b
        assert call(group, mul, 0, u8(a), None, 1, o8) == ZK_ERR_ARG
        assert call(group, add, 0, u8(a), u8(a), 1, None) == ZK_ERR_ARG
        assert call(group, add, 0, u8(a), u8(a), 0, o8) == ZK_ERR_ARG                # no operands
        assert call(group, dbl, 0, None, None, 1, o8) == ZK_ERR_ARG
        for bad_group in (2, -1):
            assert call(bad_group, add, 0, u8(a), u8(a), 1, o8) == ZK_ERR_ARG
        for bad_form in (len(GL.FORMS), -1, 99):
            assert call(group, bad_form, 0, u8(a), u8(a), 1, o8) == ZK_ERR_ARG
        for bad_rep in (2, -1):
            assert call(group, add, bad_rep, u8(a), u8(a), 1, o8) == ZK_ERR_ARG
        # a coordinate >= p, in every position of a, of an XYZZ b and of an affine b (p itself and 2^384 - 1)
        for big in (P._fp_be(P.P), b"\xff" * 48):
            for k in range(len(a) // 48):
                bad = a[:48 * k] + big + a[48 * (k + 1):]
                assert call(group, add, 0, u8(bad), u8(a), 1, o8) == ZK_ERR_ARG, k
                assert call(group, add, 1, u8(a), u8(bad), 1, o8) == ZK_ERR_ARG, k
                assert call(group, dbl, 0, u8(bad), None, 1, o8) == ZK_ERR_ARG, k
            for k in range(len(q) // 48):
                bad = q[:48 * k] + big + q[48 * (k + 1):]
                assert call(group, madd, 0, u8(a), u8(bad), 1, o8) == ZK_ERR_ARG, k
        # the second of two operands is checked too
        assert call(group, add, 0, u8(a + a[:-48] + P._fp_be(P.P)), u8(a + a), 2, o8) == ZK_ERR_ARG
        # a scalar >= r: r itself, 2^256 - 1; the identity where a form's contract excludes it
        for big in (P.R.to_bytes(32, "little"), b"\xff" * 32):
            assert call(group, mul, 0, u8(a), u8(big), 1, o8) == ZK_ERR_SCALAR_RANGE
        assert call(group, mul, 0, u8(a + a), u8(P.fr_to_bytes(5) + P.R.to_bytes(32, "little")), 2, o8) == ZK_ERR_SCALAR_RANGE
        for name, f in GL.FORMS.items():
            if f.second == "table" and not (f.g2_only and group == 0):
                assert call(group, f.number, 0, u8(a), u8(bytes(len(q))), 1, o8) == ZK_ERR_ARG, name
            if f.g2_only and group == 0:
                assert call(group, f.number, 0, u8(a), u8(q), 1, o8) == ZK_ERR_ARG, name        # the parked form is built for lane pairs only
        assert out.raw == b"\x09" * (2 * fb)


@pytest.mark.skipif(_lib.lib().zk_device_count() > 0, reason="a GPU is visible: the calls run (tests/test_gpu_group_law.py)")
def test_without_a_gpu_a_valid_call_is_a_hip_error():
    lib = _lib.lib()
    for group in (0, 1):
        g, a, q = _operands(group)
        out = C.create_string_buffer(192)
        for name, f in GL.FORMS.items():
            if f.g2_only and group == 0:
                continue
            b = {"xyzz": a, "affine": q, "table": q, "scalar": P.fr_to_bytes(P.R - 1), None: None}[f.second]
            for rep in (0, 1):
                assert lib.zk_selftest_group(group, f.number, rep, u8(a), None if b is None else u8(b), 1, C.cast(out, _lib._P8)) == ZK_ERR_HIP, name


# ---- completeness of the form table
# what only calls a tested form: the non-inlined wrappers of ec.cuh, which pass their arguments to the _impl of the same name
WRAPPERS = {"xyzz_add_fn": "xyzz_add_impl", "xyzz_madd_fn": "xyzz_madd_impl", "xyzz_dbl_fn": "xyzz_dbl_impl",
            "xyzz_add": "xyzz_add_impl", "xyzz_madd": "xyzz_madd_impl", "xyzz_dbl": "xyzz_dbl_impl"}
NAME = r"(xyzz_\w*add\w*|xyzz_\w*dbl\w*|jac_\w+|xyzz_mul_scalar\w*|window_table\w*)"
# not the device's: the verifiers' CPU half is plain C++ with a Jacobian law of its own on 64-bit limbs, held to the oracle by tests/test_pairing_host.py
HOST_ONLY_UNITS = {"pairing_host.hip"}


def defined_group_law_functions():
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.cuh")) + glob.glob(os.path.join(CSRC, "*.hip"))):
        if os.path.basename(path) in HOST_ONLY_UNITS:
            continue
        text = re.sub(r"//[^\n]*", "", open(path).read())
        # a definition: [template <...>] qualifiers, a return type, the name, a parameter list, an opening brace
        for m in re.finditer(r"(?:FF_INLINE|__device__|__noinline__|static|inline)[^;{}()]*?\b%s\s*\([^;{}]*?\)\s*\{" % NAME, text):
            found.setdefault(m.group(1), set()).add(os.path.basename(path))
    return found


def test_every_group_law_function_of_csrc_is_a_row_of_the_form_table_or_a_named_wrapper():
    found = defined_group_law_functions()
    # the scan sees what it is meant to see
    for must in ("xyzz_add_impl", "xyzz_dbl_impl", "xyzz_dbl_aff", "xyzz_madd_impl", "xyzz_mmadd_impl", "xyzz_madd_equal_x", "xyzz_madd_parked", "xyzz_add_raw_mem",
                 "xyzz_add_slots", "xyzz_dbl_slots", "jac_dbl", "jac_madd", "jac_add", "xyzz_mul_scalar_endo", "window_table_affine", "xyzz_add_fn", "xyzz_dbl"):
        assert must in found, must
    assert found["xyzz_add_slots"] == {"ec_slots.cuh"} and found["jac_add"] == {"lagrange_derive.hip"} and found["xyzz_madd_parked"] == {"msm_acc.cuh"}
    assert "__global__" not in open(os.path.join(CSRC, "pairing_host.hip")).read()          # host-only indeed
    tested = {f.function for f in GL.FORMS.values()}
    for name in found:
        assert name in tested or name in WRAPPERS or name in GL.COVERED_BY, \
            "%s (%s) is a form of the group law that tests/group_law_cases.py: FORMS does not run" % (name, ", ".join(sorted(found[name])))
    for name, inner in list(WRAPPERS.items()):
        assert name in found and inner in tested, name
    for name, row in GL.COVERED_BY.items():
        assert name in found and row in GL.FORMS, name
    assert tested <= set(found)          # no row names a function that is gone
    # the wrappers do nothing but call: one statement each
    ec = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "ec.cuh")).read())
    for name in ("xyzz_add_fn", "xyzz_madd_fn", "xyzz_dbl_fn"):
        body = re.search(r"\b%s\s*\([^)]*\)\s*\{([^}]*)\}" % name, ec).group(1)
        assert body.count(";") == 1 and WRAPPERS[name] in body, name


def test_the_battery_holds_every_class_and_every_named_scalar():
    """what the GPU test asserts about its operands, without a GPU: every class in every representation, and the model's word on the scalar edges"""
    for group in (0, 1):
        g, pairs, counts = GL.battery(group, generic=12, special=3, points=6)
        assert set(counts) == {"generic", "P+P", "P-P", "O+P", "P+O", "O+O", "equal y"}
        for x in pairs:
            for q in (x.a, x.b_xyzz):
                assert q[2] * q[2] * q[2] == q[3] * q[3]                  # zz^3 = zzz^2
        assert len(GL.named_scalars(group)) >= 19
