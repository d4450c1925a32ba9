"""zk_groth16_srs_check and zk_groth16_srs_contribute without a GPU: include/zkmi355x.h, _lib.EXPORTS, _lib.SRS_PROTOTYPES, the built library and the
OCaml files name the same calls with the same argument lists; every argument refusal comes before the device is touched, in the header's order, and
leaves 0x5a-filled outputs as they were; a box without a GPU answers ZK_ERR_HIP; the names stay out of the words tests/option_cases.py routes on;
and the three places that said a string check is not in this library say where it is."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from zukelang_amd import _lib
from zukelang_amd import groth16 as G
from zukelang_amd.groth16 import SRS, _p
from zukelang_amd.r1cs import FR_MODULUS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import option_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zukelang_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
CHECK, CONTRIB = "zk_groth16_srs_check", "zk_groth16_srs_contribute"
WANT = {
    CHECK: ["ptr", "size_t", "size_t", "ptr", "size_t", "ptr", "ptr"],
    CONTRIB: ["ptr", "size_t", "size_t", "ptr", "size_t", "ptr", "ptr", "ptr", "ptr", "ptr"],
}
ARG, RANGE, HIP, DOMAIN = -1, -3, -5, -8


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
    assert set(_lib.SRS_PROTOTYPES) == set(WANT)
    for name, want in WANT.items():
        assert _header_kinds(name) == want, name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        proto = _lib.SRS_PROTOTYPES[name]
        assert len(proto) == len(want), name
        for k, t in zip(want, proto):
            if k == "ptr":
                assert issubclass(t, C._Pointer), name
            else:
                assert t is C.c_size_t, name
        assert getattr(lib, name).argtypes == proto and getattr(lib, name).restype is C.c_int
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    assert ('fn "%s" (ptr char @-> size_t @-> size_t @-> ptr char @-> size_t @-> ptr char @-> ptr uint32_t @-> returning int)' % CHECK) in ml
    assert ('fn "%s"\n    (ptr char @-> size_t @-> size_t @-> ptr char @-> size_t @-> ptr char @-> ptr char @-> ptr char @-> ptr char @-> ptr char @-> returning int)'
            % CONTRIB) in ml
    assert "let groth16_srs_check" in ml and "let groth16_srs_contribute" in ml and "let srschk_names" in ml
    g = open(os.path.join(ROOT, "ocaml", "groth16_mi355x.ml")).read()
    assert "let srs_check" in g and "let srs_contribute" in g and "Mi355x.groth16_srs_check" in g and "Mi355x.groth16_srs_contribute" in g
    assert callable(SRS.check) and callable(SRS.contribute) and callable(G.verify_srs_contributions)


def test_the_mask_bits_have_one_spelling():
    bits = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define ZK_SRSCHK_(\w+)\s+(\d+)u", HEADER)}
    assert bits == _lib.SRSCHK_BITS == {"generators": 1, "tau_g1": 2, "tau_g2": 4, "alpha": 8, "beta": 16, "trivial": 32}
    assert list(_lib.SRSCHK_BITS.values()) == sorted(_lib.SRSCHK_BITS.values())
    ml = open(os.path.join(ROOT, "ocaml", "mi355x.ml")).read()
    for name, bit in bits.items():
        assert '("%s", %d)' % (name, bit) in ml[ml.index("let srschk_names"):], name
    v = G.SRSCheck(2 | 16)
    assert (v.ok, v.failed, v.names, bool(v)) == (False, 18, ["tau_g1", "beta"], False) and G.SRSCheck(0).ok and repr(G.SRSCheck(0)) == "SRSCheck(ok)"


def test_the_names_hold_no_routed_word():
    for word in OC.ROUTED_WORDS:
        for name in WANT:
            assert word not in name, (
                "tests/test_option_cases.py asks every header call whose name holds %r for a row of option_cases.ROUTES; that table is an existing test "
                "file and cannot gain a row here, so the promise behind it -- no public option changes a string's verdict or a contributed string -- is "
                "kept by tests/test_gpu_srs_options.py instead, and the names must stay out of the routed words" % word)
    assert os.path.exists(os.path.join(ROOT, "tests", "test_gpu_srs_options.py"))


class Args:
    """one string of (N1, NAB, N2) = (5, 3, 4) zero points and the outputs of both calls, 0x5a-filled; fields are replaced per case"""

    def __init__(self):
        self.n1, self.nab, self.n2 = 5, 3, 4
        self.s1, self.s2 = np.zeros(96 * (1 << 6), dtype=np.uint8), np.zeros(192 * (1 << 6), dtype=np.uint8)          # room for the off-by-one lengths
        self.seed = np.arange(32, dtype=np.uint8)
        self.failed = C.c_uint32(0x5A5A5A5A)
        self.mul = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in (3, 5, 7)), dtype=np.uint8).copy()
        self.o1, self.o2 = np.full(96 * (1 << 6), 0x5A, dtype=np.uint8), np.full(192 * (1 << 6), 0x5A, dtype=np.uint8)
        self.l1, self.l2 = np.full(6 * 96, 0x5A, dtype=np.uint8), np.full(3 * 192, 0x5A, dtype=np.uint8)
        self.null = set()

    def ptr(self, name, v):
        return None if name in self.null else v

    def check(self):
        return _lib.lib().zk_groth16_srs_check(self.ptr("s1", _p(self.s1)), self.n1, self.nab, self.ptr("s2", _p(self.s2)), self.n2, self.ptr("seed", _p(self.seed)),
                                               self.ptr("failed", C.byref(self.failed)))

    def contribute(self):
        return _lib.lib().zk_groth16_srs_contribute(self.ptr("s1", _p(self.s1)), self.n1, self.nab, self.ptr("s2", _p(self.s2)), self.n2, self.ptr("mul", _p(self.mul)),
                                                    self.ptr("o1", _p(self.o1)), self.ptr("o2", _p(self.o2)), self.ptr("l1", _p(self.l1)), self.ptr("l2", _p(self.l2)))

    def untouched(self):
        return all((x == 0x5A).all() for x in (self.o1, self.o2, self.l1, self.l2)) and self.failed.value == 0x5A5A5A5A


def _with(**kw):
    a = Args()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _mul(*xs):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint8).copy()


# lengths the header refuses, with the code: the minima (ARG) come before the comparisons (DOMAIN)
BAD_LENGTHS = [
    (dict(n1=1), ARG), (dict(n1=0), ARG), (dict(nab=0), ARG), (dict(n2=1), ARG), (dict(n2=0), ARG),
    (dict(n1=1, nab=9, n2=9), ARG),                      # below a minimum AND out of proportion: the minimum decides
    (dict(n1=(1 << 25) + 1, nab=0), ARG),
    (dict(nab=6), DOMAIN), (dict(n2=6), DOMAIN), (dict(n1=(1 << 25) + 1), DOMAIN), (dict(n1=2, nab=1, n2=3), DOMAIN),
]


def test_the_checks_argument_errors_come_before_the_device_in_the_headers_order():
    lib = _lib.lib()
    for name in ("s1", "s2", "failed"):
        a = _with(null={name})
        assert a.check() == ARG and a.untouched(), name
        assert b"zk_groth16_srs_check" in lib.zk_last_error()
    a = _with(null={"s1"}, nab=99)          # a null pointer wins over a length
    assert a.check() == ARG and b"null argument" in lib.zk_last_error()
    for kw, code in BAD_LENGTHS:
        a = _with(**kw)
        assert a.check() == code and a.untouched(), kw
        assert b"zk_groth16_srs_check" in lib.zk_last_error()
    if lib.zk_device_count() == 0:
        for kw in (dict(), dict(null={"seed"}), dict(n1=2, nab=1, n2=2), dict(n1=5, nab=5, n2=5)):
            a = _with(**kw)
            assert a.check() == HIP and a.untouched(), kw


def test_the_contributions_argument_errors_come_before_the_device_in_the_headers_order():
    lib = _lib.lib()
    for name in ("s1", "s2", "mul", "o1", "o2"):
        a = _with(null={name})
        assert a.contribute() == ARG and a.untouched(), name
        assert b"zk_groth16_srs_contribute" in lib.zk_last_error()
    for kw, code in BAD_LENGTHS:
        a = _with(mul=_mul(0, FR_MODULUS, 1), **kw)          # a length wins over a factor
        assert a.contribute() == code and a.untouched(), kw
    r = FR_MODULUS
    for mul, code in (((0, 1, 1), ARG), ((1, 0, 1), ARG), ((1, 1, 0), ARG), ((r, 1, 1), RANGE), ((1, r, 1), RANGE), ((1, 1, r), RANGE),
                      ((1, 1, (1 << 256) - 1), RANGE), ((r + 1, 1, 1), RANGE), ((r, 0, 1), RANGE), ((0, r, 1), ARG)):
        a = _with(mul=_mul(*mul))
        assert a.contribute() == code and a.untouched(), mul
    if lib.zk_device_count() == 0:
        for kw in (dict(), dict(null={"l1", "l2"}), dict(mul=_mul(r - 1, r - 1, r - 1)), dict(n1=2, nab=1, n2=2)):
            a = _with(**kw)
            assert a.contribute() == HIP and a.untouched(), kw


def test_the_python_layer_checks_shapes_before_it_calls():
    z = lambda k, b: np.zeros(b * k, dtype=np.uint8)
    good = SRS(z(5, 96), z(3, 96), z(3, 96), bytes(192), z(4, 192))
    for field, v in (("tau_g1", z(1, 95)), ("alpha_tau_g1", z(2, 96)), ("beta_g2", bytes(96)), ("tau_g2", z(1, 100))):
        bad = SRS(**dict(good.__dict__, **{field: v}))
        with pytest.raises(ValueError, match="whole uncompressed points"):
            bad.check()
        with pytest.raises(ValueError, match="whole uncompressed points"):
            bad.contribute((1, 2, 3))
    with pytest.raises(ValueError, match="32 bytes"):
        good.check(seed=b"short")
    for mul in ((1, 2), (1, 2, -3), (1, 2, 1 << 256)):
        with pytest.raises(ValueError, match="three elements of Fr"):
            good.contribute(mul)
    assert good.link_points() == (bytes(96), bytes(96), bytes(96))
    # a chain is refused on shape and on identities before any pairing
    assert not G.verify_srs_contributions(good, [], good)                          # the identity starts no chain
    pt = bytes([1]) + bytes(95)
    assert not G.verify_srs_contributions((pt, pt), [], (pt, pt))
    assert G.verify_srs_contributions((pt, pt, pt), [], (pt, pt, pt))              # an empty chain: first == last
    assert not G.verify_srs_contributions((pt, pt, pt), [], (pt, pt, bytes([2]) + bytes(95)))


def test_the_new_unit_reuses_the_existing_kernels():
    """the call's own HIP is the coefficient kernel and the three-scalar conversion; the expansion is key_check.hip's, factored out and not copied; the
    sums, the subgroup test, the power scan, the multiplications and the pairings are reached through the existing host functions"""
    text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "srs.hip")).read())
    assert re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(", text) == ["k_srs_coefficients", "k_srs_factors_to_mont"]
    for fn in ("points_subgroup_verdicts(", "SUBGROUP_ENDO", "msm_sort_accumulate_many(", "msm_reduce(", "keychk_pairing_products(", "power_run(", "points_scale_tabmul(",
               "fixed_base_mul(", "seed_expand_at(", "seed_take("):
        assert fn in text, fn
    assert "0x9E3779B97F4A7C15" not in text and "atomic" not in text
    assert not re.search(r"\b(jac_\w+|window_table\w*|xyzz_mul_scalar\w*|xyzz_add\w*|fe_inv\w*)\s*\(", text)
    kc = open(os.path.join(CSRC, "key_check.hip")).read()
    assert "0x9E3779B97F4A7C15" not in kc and "seed_expand_at(seed, i)" in kc and '#include "seed_expand.cuh"' in kc
    assert open(os.path.join(CSRC, "seed_expand.cuh")).read().count("0x9E3779B97F4A7C15") == 1
    keygen = open(os.path.join(CSRC, "keygen.hip")).read()
    assert len(re.findall(r"__global__ void k_power_run\(", keygen)) == 1
    # the check's subgroup test does not read the option; the contribution's does
    chk = text[text.index("static int srs_check_run("):text.index("static constexpr uint64_t SRS_SCALE_SLAB")]
    con = text[text.index("static int srs_contribute_run("):]
    assert "key_subgroup_check()" not in chk and "OPT_" not in chk and 'srs_decode(srs_g1, srs_g2, n1, nab, n2, true, "srs_check"' in chk
    assert "key_subgroup_check()" in con


def test_the_documents_point_to_the_calls():
    for text in ("a phase-1 string as a whole", "ZK_SRSCHK_TRIVIAL", "whatever ZK_KEY_SUBGROUP_CHECK says", "srs_contribute", "is zk_groth16_srs_check below"):
        assert text in HEADER, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for doc, text in (("header", HEADER), ("DESIGN.md", design), ("README.md", readme)):
        assert "not part of this library" not in text, doc
    assert "2t" in design and CHECK in design and CONTRIB in design and "profiles/srs_ab.json" in design
    for doc in (readme, integ):
        assert CHECK in doc and CONTRIB in doc
    assert "from a ceremony's string to a proof" in integ
    for f in ("srs_kernel_resources.txt", "srs_ab.json", "srs.json"):
        assert os.path.exists(os.path.join(ROOT, "profiles", f)), f
