"""zk_groth16_srs_sizes, zk_groth16_pk_specialize and zk_selftest_g1_colsum without a GPU: include/zkmi355x.h, _lib.EXPORTS,
_lib.SPECIALIZE_PROTOTYPES, the built library and the OCaml files name the same calls with the same argument lists; every argument refusal comes
before the device is touched, in the header's order, and leaves 0x5a-filled outputs as they were; a box without a GPU answers ZK_ERR_HIP; and the
names stay out of the words tests/option_cases.py routes on."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from zukelang_amd import _lib
from zukelang_amd import r1cs as RC
from zukelang_amd.groth16 import SRS, Groth16, _csr, _p
from zukelang_amd.r1cs import FR_MODULUS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import option_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zukelang_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
SIZES, CALL, HOOK = "zk_groth16_srs_sizes", "zk_groth16_pk_specialize", "zk_selftest_g1_colsum"
WANT = {
    SIZES: ["uint32_t", "ptr", "ptr", "ptr"],
    CALL: ["uint32_t", "uint32_t", "csr", "csr", "csr", "ptr", "ptr", "size_t", "ptr", "size_t", "uint32_t", "ptr", "size_t", "ptr", "size_t", "ptr", "ptr", "ptr"],
    HOOK: ["ptr", "size_t", "ptr", "ptr", "ptr", "uint32_t", "ptr"],
}
ARG, RANGE, HIP, DOMAIN = -1, -3, -5, -8


def _header_kinds(name):
    body = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, body)
    assert m, "%s is not declared in include/zkmi355x.h" % name
    out = []
    for p in m.group(1).split(","):
        p = re.sub(r"\[[^\]]*\]", "*", p)
        out.append("csr" if "zk_csr" in p else "ptr" if "*" in p else next(t for t in ("uint64_t", "uint32_t", "size_t", "int") if re.search(r"\b%s\b" % t, p)))
    return out


def test_the_calls_are_declared_exported_and_bound():
    lib = _lib.lib()
    assert set(_lib.SPECIALIZE_PROTOTYPES) == set(WANT)
    for name, want in WANT.items():
        assert _header_kinds(name) == want, name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        proto = _lib.SPECIALIZE_PROTOTYPES[name]
        assert len(proto) == len(want), name
        for k, t in zip(want, proto):
            if k == "csr":
                assert t is _lib._PCSR, name
            elif k == "ptr":
                assert issubclass(t, C._Pointer), name
            else:
                assert t is {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "size_t": C.c_size_t}[k], name
        assert getattr(lib, name).argtypes == proto and getattr(lib, name).restype is C.c_int
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    for name in WANT:
        assert 'fn "%s"' % name in ml, name
    assert ('fn "%s"\n    (uint32_t @-> uint32_t @-> ptr csr @-> ptr csr @-> ptr csr @-> ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t @-> uint32_t\n'
            '   @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> ocaml_bytes @-> ptr uint64_t @-> returning int)' % CALL) in ml
    assert "let specialize_call" in ml and "let groth16_srs_sizes" in ml
    g = open(os.path.join(ROOT, "ocaml", "groth16_mi355x.ml")).read()
    assert "let specialize" in g and "Mi355x.specialize_call" in g
    assert callable(Groth16.specialize) and callable(SRS.generate) and callable(SRS.cut) and callable(SRS.sizes)


def test_the_names_hold_no_routed_word():
    for word in OC.ROUTED_WORDS:
        for name in WANT:
            assert word not in name, (
                "tests/test_option_cases.py asks every header call whose name holds %r for a row of option_cases.ROUTES; that table is an existing test "
                "file and cannot gain a row here, so the promise behind it -- no public option changes a specialised key or its proofs -- is kept by "
                "tests/test_gpu_specialize_options.py instead, and the names must stay out of the routed words" % word)
    assert os.path.exists(os.path.join(ROOT, "tests", "test_gpu_specialize_options.py"))


def test_srs_sizes():
    lib = _lib.lib()
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    for n in (1, 2, 3, 4, 5, 1000, 1 << 24):
        assert lib.zk_groth16_srs_sizes(n, C.byref(a), C.byref(b), C.byref(c)) == 0
        assert (a.value, b.value, c.value) == (max(n + 2, 2 * n - 1), n, n + 2) == SRS.sizes(n)
    assert lib.zk_groth16_srs_sizes(5, None, None, None) == 0
    assert lib.zk_groth16_srs_sizes(0, C.byref(a), C.byref(b), C.byref(c)) == ARG
    assert lib.zk_groth16_srs_sizes((1 << 24) + 1, C.byref(a), C.byref(b), C.byref(c)) == ARG


class Args:
    """one call's arguments on the README circuit, every output 0x5a-filled; fields are replaced per case"""

    def __init__(self):
        self.cs = RC.readme_circuit(3)[0]
        n, m = self.cs.n, self.cs.m
        n1, nab, n2 = SRS.sizes(n)
        self.n, self.m = n, m
        self.L, self.R, self.O = _csr(self.cs.L), _csr(self.cs.R), _csr(self.cs.O)
        self.mid = np.ascontiguousarray(self.cs.mid, dtype=np.uint8)
        n_mid = int(self.mid.sum())
        self.s1, self.s2 = np.zeros(96 * (n1 + 2 * nab), dtype=np.uint8), np.zeros(192 * (1 + n2), dtype=np.uint8)
        self.c1, self.c2 = n1 + 2 * nab, 1 + n2
        self.form = 0
        self.k1, self.k2 = 3 + (n + 2) + (n - 1) + n_mid, 2 + (n + 2)
        self.g1, self.g2 = np.full(96 * self.k1, 0x5A, dtype=np.uint8), np.full(192 * self.k2, 0x5A, dtype=np.uint8)
        self.v1, self.v2 = np.full(96 * (1 + m - n_mid), 0x5A, dtype=np.uint8), np.full(576, 0x5A, dtype=np.uint8)
        self.h = C.c_uint64(0x5A5A)
        self.null = set()

    def call(self):
        ptr = lambda name, v: None if name in self.null else v
        return _lib.lib().zk_groth16_pk_specialize(
            self.n, self.m, ptr("L", C.byref(self.L)), ptr("R", C.byref(self.R)), ptr("O", C.byref(self.O)), ptr("mid", _p(self.mid)),
            ptr("s1", _p(self.s1)), self.c1, ptr("s2", _p(self.s2)), self.c2, self.form,
            ptr("g1", _p(self.g1)), self.k1, ptr("g2", _p(self.g2)), self.k2, ptr("v1", _p(self.v1)), ptr("v2", _p(self.v2)), ptr("h", C.byref(self.h)))

    def untouched(self):
        return all((x == 0x5A).all() for x in (self.g1, self.g2, self.v1, self.v2)) and self.h.value == 0x5A5A


def _with(**kw):
    a = Args()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _matrix(cs, which, **kw):
    """the circuit's matrix `which` with its arrays replaced"""
    M = getattr(cs, which)
    M2 = RC.Matrix(kw.get("ptr", M.ptr).copy(), kw.get("col", M.col).copy(), kw.get("val", M.val).copy())
    return M2, _csr(M2)


def test_argument_errors_come_before_the_device_in_the_headers_order():
    lib = _lib.lib()
    # 1 null pointers
    for name in ("L", "R", "O", "mid", "s1", "s2"):
        a = _with(null={name})
        assert a.call() == ARG and a.untouched(), name
        assert b"zk_groth16_pk_specialize" in lib.zk_last_error()
    # 2 form, 3 n and m -- each wins over a wrong count further on
    for kw in (dict(form=2), dict(n=0), dict(n=(1 << 24) + 1), dict(m=0)):
        a = _with(c1=1, **kw)
        assert a.call() == ARG and a.untouched(), kw
    a = _with(null={"L"}, form=7, c1=0)
    assert a.call() == ARG and b"null argument" in lib.zk_last_error()
    # 4 counts: each of the four off by one, before the matrices are looked at
    base = Args()
    for field in ("c1", "c2", "k1", "k2"):
        for d in (-1, 1):
            a = _with(**{field: getattr(base, field) + d})
            bad_ptr = base.cs.L.ptr.copy(); bad_ptr[1] = 9
            keep, a.L = _matrix(a.cs, "L", ptr=bad_ptr)
            assert a.call() == DOMAIN and a.untouched(), (field, d)
    # a key count is not looked at where its buffer is not given
    if lib.zk_device_count() == 0:
        a = _with(k1=1, k2=1, null={"g1", "g2"})
        assert a.call() == HIP and a.untouched()
    # 5 a malformed matrix, before a coefficient's range
    big = base.cs.R.val.copy(); big[:32] = np.frombuffer(int(FR_MODULUS).to_bytes(32, "little"), dtype=np.uint8)
    for which, kw in (("L", dict(ptr=np.array([0, 2, 1, 5], dtype=np.uint32))), ("O", dict(col=np.array([1, 2, 9], dtype=np.uint32)))):
        a = Args()
        keep, m_ = _matrix(a.cs, which, **kw)
        setattr(a, which, m_)
        keep2, a.R = _matrix(a.cs, "R", val=big)
        assert a.call() == ARG and a.untouched(), which
    # 6 a coefficient >= r
    for v in (FR_MODULUS, (1 << 256) - 1):
        a = Args()
        val = a.cs.O.val.copy(); val[32:64] = np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)
        keep, a.O = _matrix(a.cs, "O", val=val)
        assert a.call() == RANGE and a.untouched(), hex(v)
    # 7 nothing left to refuse without a device
    if lib.zk_device_count() == 0:
        for null in (set(), {"g1", "g2", "v1", "v2"}, {"h"}):
            a = _with(null=null)
            assert a.call() == HIP and a.untouched(), null


def test_argument_errors_of_the_hook_come_before_the_device():
    lib = _lib.lib()
    fn = getattr(lib, HOOK)
    pts, out = np.zeros(96 * 3, dtype=np.uint8), np.full(96 * 2, 0x5A, dtype=np.uint8)
    ptr = np.array([0, 1, 2], dtype=np.uint32)
    row = np.array([0, 2], dtype=np.uint32)
    coef = np.frombuffer((5).to_bytes(32, "little") + (1).to_bytes(32, "little"), dtype=np.uint8).copy()
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    assert fn(None, 3, p32(ptr), p32(row), _p(coef), 2, _p(out)) == ARG
    assert fn(_p(pts), 3, None, p32(row), _p(coef), 2, _p(out)) == ARG
    assert fn(_p(pts), 3, p32(ptr), p32(row), _p(coef), 2, None) == ARG
    assert fn(_p(pts), 0, p32(ptr), p32(row), _p(coef), 2, _p(out)) == ARG
    assert fn(_p(pts), 3, p32(ptr), p32(row), _p(coef), 0, _p(out)) == ARG
    assert fn(_p(pts), 3, p32(ptr), None, _p(coef), 2, _p(out)) == ARG
    assert fn(_p(pts), 3, p32(ptr), p32(row), None, 2, _p(out)) == ARG
    assert b"zk_selftest_g1_colsum" in lib.zk_last_error()
    assert fn(_p(pts), 3, p32(np.array([0, 2, 1], dtype=np.uint32)), p32(row), _p(coef), 2, _p(out)) == ARG
    assert fn(_p(pts), 3, p32(ptr), p32(np.array([0, 3], dtype=np.uint32)), _p(coef), 2, _p(out)) == ARG
    big = coef.copy(); big[32:] = np.frombuffer(int(FR_MODULUS).to_bytes(32, "little"), dtype=np.uint8)
    assert fn(_p(pts), 3, p32(ptr), p32(row), _p(big), 2, _p(out)) == RANGE
    if lib.zk_device_count() == 0:
        assert fn(_p(pts), 3, p32(ptr), p32(row), _p(coef), 2, _p(out)) == HIP
        assert fn(_p(pts), 3, p32(np.zeros(3, dtype=np.uint32)), None, None, 2, _p(out)) == HIP          # empty columns need no entries
    assert (out == 0x5A).all()


def test_the_python_layer_checks_lengths_before_it_calls():
    cs = RC.readme_circuit(3)[0]
    n1, nab, n2 = SRS.sizes(cs.n)
    good = SRS(np.zeros(96 * n1, dtype=np.uint8), np.zeros(96 * nab, dtype=np.uint8), np.zeros(96 * nab, dtype=np.uint8), bytes(192), np.zeros(192 * n2, dtype=np.uint8))
    for field, v in (("tau_g1", np.zeros(96 * (n1 + 1), dtype=np.uint8)), ("alpha_tau_g1", np.zeros(96 * (nab - 1), dtype=np.uint8)),
                     ("beta_g2", bytes(96)), ("tau_g2", np.zeros(192 * (n2 + 1), dtype=np.uint8))):
        bad = SRS(**dict(good.__dict__, **{field: v}))
        with pytest.raises(ValueError, match="exactly SRS.sizes"):
            Groth16.specialize(cs, bad)
    with pytest.raises(ValueError, match="SRS.cut"):
        good.cut(cs.n + 1)
    assert good.cut(cs.n).tau_g1.shape == good.tau_g1.shape
    assert (SRS.sizes(1), SRS.sizes(2), SRS.sizes(3), SRS.sizes(8)) == ((3, 1, 3), (4, 2, 4), (5, 3, 5), (15, 8, 10))


def test_the_new_kernels_live_in_their_own_unit_and_the_derivation_is_unchanged():
    """the call's own HIP is the gather, the chunked sum and the pick in specialize.hip; it reaches the derivation's kernels through host functions of
    lagrange_derive.hip and adds no group law of its own beyond the general addition the issue names"""
    text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "specialize.hip")).read())
    assert re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(", text) == ["k_colsum_gather", "k_colsum", "k_pick_points_g1"]
    assert "xyzz_add_impl(acc, q)" in text and "atomic" not in text
    assert not re.search(r"\b(jac_\w+|window_table\w*|xyzz_mul_scalar\w*|fe_inv\w*)\s*\(", text)
    for fn in ("specialize_g1_bases(", "g1_raw_tabmul(", "g1_raw_to_affine(", "transpose_csr(", "points_from_bytes_checked(", "groth16_derive_lagrange_pools("):
        assert fn in text, fn
    derive = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "lagrange_derive.hip")).read())
    body = derive[derive.index("int specialize_g1_bases("):derive.index("int g1_raw_tabmul(")]
    for k in ("derive_set<Fp>", "derive_set_enqueue<Fp>", "gntt<Fp>", "g_tabmul<Fp>", "k_tab_neg_canon", "OPT_DERIVE_SIDE_BY_SIDE"):
        assert k in body, k


def test_the_documents_point_to_the_call():
    for text in ("a phase-1 string specialised to a circuit", "TRUST", "zk_groth16_key_check", "specialize_derive", "ZK_KEY_SUBGROUP_CHECK=0"):
        assert text in HEADER, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "2s" in design and CALL in design and "profiles/specialize.json" in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert CALL in open(os.path.join(ROOT, doc)).read(), doc
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "SRS" in integ and "contribute" in integ and "check_key" in integ
    assert os.path.exists(os.path.join(ROOT, "profiles", "specialize_kernel_resources.txt"))
