"""GPU parity at constraint counts that are no power of two and no longer fit one LDS tile (tests/nonpow2_cases.py: the sizes and why those;
tests/test_nonpow2_plan.py holds each size to its reason without a GPU).  One parametrized test per layer, so that a failure names its layer:

  a. the Fr stage alone (csrc/frstage.hip: Z through tree_convert, the unfused tree levels, the padded windows of the quotient), tau-power and
     Lagrange-form key: every coefficient against the literal QAP.eval at 1025, and at every size the evaluations of v, w, h against the interpolants
     of the sparse products in Python integers (nonpow2_cases.eval_by_values: the product formula, never the library's own _lagrange_at);
  b. Groth16 proofs, tau-power / Lagrange-form / derived key (k_zt, k_lag_scale, k_lag_h; csrc/lagrange_derive.hip), against the trapdoor oracle;
  c. Pinocchio with the compact h pool and without (frstage_leading_coeffs: 40000 reaches the ragged second trip of k_lead_partial), as uploaded and derived;
  d. key generation on the device (csrc/keygen.hip), through the helpers of tests/test_gpu_keygen.py;
  e. six degenerate witnesses (h = 0, h = 1, every scalar of every product zero, ...) through ONE key per size, protocol and form;
  f. the residue-number-system engine (ZK_FR_RNS=1) with tree levels 11 and 12 at n != n2.

Every comparison is of exact bytes or exact integers.  Measured on an MI355X in one run with tests/test_gpu_groth16.py: the slowest case here 1.60 s
(Pinocchio, 40000, compact pool), every other at most 1.50 s, all 51 together 28 s; the bound, test_iterated_cubic_matches_oracle[2048] plus
test_lagrange_bases_derived_in_the_exponent at 1024, is 2.20 + 0.76 s."""
import os

import pytest

import nonpow2_cases as NP
import oracle_lib as O
from oracle import pyref as P
from test_gpu_keygen import check_groth16, check_pinocchio, trapdoors
from zukelang_amd import _lib
from zukelang_amd import pinocchio as PIN
from zukelang_amd import r1cs as RC
from zukelang_amd.curve import G1, G2
from zukelang_amd.groth16 import Groth16, PKey

pytestmark = pytest.mark.gpu

R = RC.FR_MODULUS
frb = P.fr_to_bytes
frs = lambda xs: bytes(RC.fr_bytes(xs))
csrs = lambda cs: [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
SIZES = sorted(NP.SIZES)
ZERO_G1 = bytes([0x40]) + bytes(95)


def _set_option(name, value):
    _lib.check(_lib.lib().zk_set_option(name.encode(), None if value is None else str(value).encode()))


# ---- circuits, witnesses and keys: made once per size, shared, never changed
_circuits, _g16_keys, _pin_keys = {}, {}, {}


def circuit(n):
    """(cs, w, (a, b, c) = the sparse products in Python integers, index of a witness value whose change breaks a row)"""
    if n not in _circuits:
        cs, w = RC.iterated_cubic(n, 0xC0FFEE + n) if n % 2 == 0 else RC.random_r1cs(n, n + n // 4, 0x0DD0 + n, nnz=(1, 4))
        abc = NP.sparse_products(cs, w)
        assert all(x * y % R == z for x, y, z in zip(*abc))
        val = RC.fr_ints(cs.O.val)
        k = int(cs.O.col[next(e for e in range(len(val)) if val[e])])          # a variable with a non-zero coefficient in a row of O: its change breaks that row
        bad = list(w)
        bad[k] = (bad[k] + 1) % R
        assert any(x * y % R != z for x, y, z in zip(*NP.sparse_products(cs, bad)))
        _circuits[n] = (cs, w, abc, k)
    return _circuits[n]


def g16_key(n, cs=None):
    """toxic waste, and the key in both forms from the keygen that knows tau"""
    key = (n, cs is not None)
    if key not in _g16_keys:
        cs = cs or circuit(n)[0]
        st = P.fr_stream(0x5EED1600 + n + (1 << 20) * key[1])
        tox = [next(st) for _ in range(5)]
        it = iter(tox)
        pk, vk = Groth16.keygen(lambda: next(it), cs, lagrange=True)
        _g16_keys[key] = (tox, pk, vk)
    return _g16_keys[key]


def pin_key(n, cs=None):
    key = (n, cs is not None)
    if key not in _pin_keys:
        cs = cs or circuit(n)[0]
        st = P.fr_stream(0x5EED9100 + n + (1 << 20) * key[1])
        tox = [next(st) for _ in range(8)]
        it = iter(tox)
        pk, _vk = PIN.ZK.keygen(lambda: next(it), cs)
        _pin_keys[key] = (tox, pk)
    return _pin_keys[key]


def bad_witness(n):
    cs, w, _, k = circuit(n)
    bad = list(w)
    bad[k] = (bad[k] + 1) % R
    return bad


def g16_trapdoor(cs, w, tox, r, s):
    return O.groth16_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, frs(w), frs(tox), frb(r), frb(s))


def pin_trapdoor(cs, w, tox, d):
    return O.pinocchio_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, frs(w), frs(tox), *(frb(x) for x in d))


def abc_of(p):
    return (p.a, p.b, p.c)


# ---- a. the Fr stage alone
def check_evaluations(n, abc, v, ww, h, seed):
    """v, w, h as coefficient vectors (bytes) against the interpolants of a, b, c by values: lengths, range, two points x from a fixed seed (a wrong
    vector of degree below n survives one point with probability below n / r), and v at three points of the domain."""
    a, b, c = abc
    assert len(bytes(v)) == len(bytes(ww)) == 32 * n and len(bytes(h)) == 32 * (n - 1)
    vi, wi, hi = RC.fr_ints(v), RC.fr_ints(ww), RC.fr_ints(h)
    assert all(x < R for x in vi) and all(x < R for x in wi) and all(x < R for x in hi)
    st = P.fr_stream(seed)
    for x in (next(st), next(st)):
        vx, wx = NP.horner(vi, x), NP.horner(wi, x)
        assert vx == NP.eval_by_values(a, x), "v(x)"
        assert wx == NP.eval_by_values(b, x), "w(x)"
        assert NP.horner(hi, x) * NP.vanishing_at(n, x) % R == (vx * wx - NP.eval_by_values(c, x)) % R, "h(x) Z(x) = v(x) w(x) - y(x)"
    for i in (0, n // 2, n - 1):
        assert NP.horner(vi, i) == a[i] and NP.horner(wi, i) == b[i], i


def check_literal(cs, w, v, ww, h):
    """every coefficient against QAP.eval (QAP.ml:120-135), as tests/test_gpu_groth16.py: test_iterated_cubic_matches_oracle does"""
    q = O.QAP(cs.n, cs.m, *csrs(cs))
    rc, _p_ref, h_ref = q.eval(frs(w))
    assert rc == 0
    v_ref, w_ref, _ = q.eval_vwy(frs(w))
    assert bytes(v) == v_ref and bytes(ww) == w_ref
    assert bytes(h)[:len(h_ref)] == h_ref and not any(bytes(h)[len(h_ref):])


@pytest.mark.parametrize("n", SIZES)
def test_fr_stage_alone(n):
    cs, w, abc, _ = circuit(n)
    st = P.fr_stream(0x5EEDA000 + n)
    tox = [next(st) for _ in range(5)]
    e1, e2, _eio = O.groth16_setup_exponents(cs.n, cs.m, *csrs(cs), cs.mid, frs(tox), want_io=False)
    prover = Groth16(cs, PKey(G1.of_Fr(e1), G2.of_Fr(e2)))
    try:
        v, ww, h = prover.qap_eval(w)
        check_evaluations(n, abc, v, ww, h, 0xE7A1 + n)
        if n == 1025:
            check_literal(cs, w, v, ww, h)
        with pytest.raises(AssertionError):
            prover.qap_eval(bad_witness(n))
    finally:
        prover.close()
    if n in (1025, 3000):                                       # QAP.eval on a Lagrange-form key runs the basis conversion (tests/test_gpu_api_errors.py)
        _tox, pk, _vk = g16_key(n)
        lag = Groth16(cs, pk, lagrange=True)
        try:
            v1, w1, h1 = lag.qap_eval(w)
            check_evaluations(n, abc, v1, w1, h1, 0xE7A2 + n)
            assert (bytes(v1), bytes(w1), bytes(h1)) == (bytes(v), bytes(ww), bytes(h))
        finally:
            lag.close()


# ---- b. Groth16 proofs
def lone_and_pipelined(prover, w, rs, exp, tag):
    got = prover.prove_rs(w, *rs[0])
    assert abc_of(got) == exp[0], tag + ", lone"
    prover.set_witness(w)
    for slot, (r, s) in enumerate(rs):
        prover.prove_async(None, r, s, slot)
    for slot in range(len(rs)):
        assert abc_of(prover.prove_wait(slot)) == exp[slot], tag + ", slot %d" % slot
    return got


@pytest.mark.parametrize("n", SIZES)
def test_groth16_proofs_match_the_trapdoor_oracle(n):
    cs, w, _, _ = circuit(n)
    tox, pk, vk = g16_key(n)
    st = P.fr_stream(0x5EEDB000 + n)
    rs = [(next(st), next(st)) for _ in range(2)]
    exp = [g16_trapdoor(cs, w, tox, r, s) for r, s in rs]
    bad = bad_witness(n)
    std, lag = Groth16(cs, pk), None
    try:
        first = lone_and_pipelined(std, w, rs, exp, "tau-power key")
        with pytest.raises(AssertionError):
            std.prove_rs(bad, *rs[0])
        lag = Groth16(cs, pk, lagrange=True)
        lone_and_pipelined(lag, w, rs, exp, "Lagrange-form key")
        with pytest.raises(AssertionError):
            lag.prove_rs(bad, *rs[0])
        if n == 1025:
            assert Groth16.verify([w[k] for k in range(cs.m) if not cs.mid[k]], vk, first)
        if n <= 8193:                                           # NTTs in the exponent over n2 leaves of which n are points: the pools of the keygen that knows tau
            std.derive_lagrange()
            g1 = std.pool_points(1)
            assert g1.shape == pk.lag_g1.shape and bool((g1 == pk.lag_g1).all())
            g2 = std.pool_points(2)
            assert g2.shape == pk.lag_g2.shape and bool((g2 == pk.lag_g2).all())
            lone_and_pipelined(std, w, rs, exp, "derived key")
            with pytest.raises(AssertionError):
                std.prove_rs(bad, *rs[0])
    finally:
        std.close()
        if lag is not None:
            lag.close()


# ---- c. Pinocchio
@pytest.mark.parametrize("n,compact", [(n, c) for n in (1025, 3000, 40000) for c in (True, False)])
def test_pinocchio_proofs_match_the_trapdoor_oracle(n, compact):
    cs, w, _, _ = circuit(n)
    tox, pk = pin_key(n)
    st = P.fr_stream(0x5EEDC000 + n)
    ds = [[next(st) for _ in range(3)] for _ in range(3)] + [[0, 0, 0]]           # three blindings, and NonZK = all zero
    exp = [pin_trapdoor(cs, w, tox, d) for d in ds]
    _set_option("ZK_PIN_COMPACT_H", None if compact else "0")
    try:
        prover = PIN.ZK(cs, pk)
    finally:
        _set_option("ZK_PIN_COMPACT_H", None)
    try:
        assert prover.pool_size(5) == (n + 1 if compact else n + 1 + 2 * cs.m)
        for d, e in zip(ds, exp):
            assert prover.prove_with(w, *d).to_bytes() == e, "as uploaded, blinding %r" % (d[:1],)
        with pytest.raises(AssertionError):
            prover.prove_with(bad_witness(n), *ds[0])
        prover.derive_lagrange()
        assert prover.pool_size(5) == (n + 2 if compact else n + 1 + 2 * cs.m)
        for d, e in zip(ds, exp):
            assert prover.prove_with(w, *d).to_bytes() == e, "derived, blinding %r" % (d[:1],)
        with pytest.raises(AssertionError):
            prover.prove_with(bad_witness(n), *ds[0])
    finally:
        prover.close()


# ---- d. key generation on the device
@pytest.mark.parametrize("n", [1025, 3000, 8193])
def test_groth16_keygen_on_the_device(n):
    cs, w, _, _ = circuit(n)
    check_groth16(cs, w, trapdoors(0x77D0 + n, cs, 5, False), cross_check=True)


@pytest.mark.parametrize("n,compact", [(n, c) for n in (1025, 3000, 8193) for c in (True, False)])
def test_pinocchio_keygen_on_the_device(n, compact):
    cs, w, _, _ = circuit(n)
    check_pinocchio(cs, w, trapdoors(0x88D0 + n, cs, 8, False), cross_check=True, compact=compact)


# ---- e. degenerate witnesses: one key per (n, protocol, form), the six witnesses go through it one after another
class _Held:
    """the provers of ONE size of the free circuit, kept from one case to the next: a proof whose scalars are all zero must leave nothing behind"""
    n = None
    provers = {}

    @classmethod
    def get(cls, n):
        if cls.n != n:
            cls.release()
            cs = NP.free_circuit(n)
            tox, pk, vk = g16_key(n, cs)
            ptox, ppk = pin_key(n, cs)
            p = cls.provers
            cls.n = n
            p["tau"] = Groth16(cs, pk)
            p["lagrange"] = Groth16(cs, pk, lagrange=True)
            p["derived"] = Groth16(cs, pk)
            p["derived"].derive_lagrange()
            p["compact"] = PIN.ZK(cs, ppk)
            _set_option("ZK_PIN_COMPACT_H", "0")
            try:
                p["full"] = PIN.ZK(cs, ppk)
            finally:
                _set_option("ZK_PIN_COMPACT_H", None)
            assert p["compact"].pool_size(5) == n + 1 and p["full"].pool_size(5) == n + 1 + 2 * cs.m
        return cls.provers

    @classmethod
    def release(cls):
        for p in cls.provers.values():
            p.close()
        cls.provers, cls.n = {}, None


@pytest.fixture(scope="module", autouse=True)
def _no_handle_outlives_this_module():
    yield
    _Held.release()          # a live key pins the device list: the files after this one change it


def check_degenerate_fr_stage(prover, cs, w, kind, name):
    n = cs.n
    v, ww, h = prover.qap_eval(w)
    if n <= 33:
        check_literal(cs, w, v, ww, h)
    else:
        check_evaluations(n, (w[1:1 + n], w[1 + n:1 + 2 * n], w[1 + 2 * n:]), v, ww, h, 0xE7A3 + n)
    if kind == "zero":
        assert not any(bytes(h)), name
    if kind == "one":
        assert bytes(h) == frs([1]) + bytes(32 * (n - 2)), name
    if kind == "full":
        assert all(RC.fr_ints(h)), name
    if name == "zero":
        assert not any(bytes(v)) and not any(bytes(ww))
    return bytes(v), bytes(ww), bytes(h)


@pytest.mark.parametrize("n,name", [(n, name) for n in (8, 33, 1025, 3000) for name in NP.DEGENERATE])
def test_degenerate_witnesses(n, name):
    cs = NP.free_circuit(n)
    w, kind = NP.degenerate_witness(name, n)
    tox, _pk, vk = g16_key(n, cs)
    ptox, _ppk = pin_key(n, cs)
    held = _Held.get(n)
    check_degenerate_fr_stage(held["tau"], cs, w, kind, name)
    st = P.fr_stream(0x5EEDE000 + n + 64 * len(name))
    r, s = next(st), next(st)
    exp = g16_trapdoor(cs, w, tox, r, s)
    for form in ("tau", "lagrange", "derived"):
        got = held[form].prove_rs(w, r, s)
        assert abc_of(got) == exp, "Groth16, %s key" % form
    ds = [[next(st) for _ in range(3)], [0, 0, 0]]
    pexp = [pin_trapdoor(cs, w, ptox, d) for d in ds]
    for form in ("compact", "full"):
        for d, e in zip(ds, pexp):
            assert held[form].prove_with(w, *d).to_bytes() == e, "Pinocchio, %s h pool, %s" % (form, "ZK" if any(d) else "NonZK")
    if name == "zero":
        assert pexp[1][:96] == ZERO_G1 and pexp[1][384:480] == ZERO_G1          # NonZK on the zero witness: every product is the empty sum
        assert Groth16.verify([0, 0], vk, got)
        bad = list(w)
        bad[1 + 2 * n + n // 2] = 1                                           # one c_i = 1 where a_i b_i = 0
        for form in ("tau", "lagrange", "derived"):
            with pytest.raises(AssertionError):
                held[form].prove_rs(bad, r, s)
        for form in ("compact", "full"):
            with pytest.raises(AssertionError):
                held[form].prove_with(bad, *ds[0])


# ---- f. the residue-number-system engine
@pytest.mark.parametrize("n", [1025, 3000])
def test_rns_engine_at_n_below_n2(n):
    """ZK_FR_RNS=1 (read when a key is uploaded and per proof; csrc/rns_ntt.hip): the tree levels from rns_first_level = 11 up through the residues
    with n != n2 (3000: levels 11 and 12), the RNS_OUT_RANGE windows at offsets n and n - 1."""
    cs, w, abc, _ = circuit(n)
    tox, pk, _vk = g16_key(n)
    st = P.fr_stream(0x5EEDF000 + n)
    r, s = next(st), next(st)
    exp = g16_trapdoor(cs, w, tox, r, s)
    cases = [(cs, w, tox, pk, exp, "the circuit")]
    if n == 3000:
        fc = NP.free_circuit(n)
        ftox, fpk, _ = g16_key(n, fc)
        for name in ("h_one", "zero"):
            fw, _kind = NP.degenerate_witness(name, n)
            cases.append((fc, fw, ftox, fpk, g16_trapdoor(fc, fw, ftox, r, s), name))
    old = os.environ.get("ZK_FR_RNS")
    os.environ["ZK_FR_RNS"] = "1"
    provers = {}
    try:
        for c, wit, _t, key, e, tag in cases:
            if id(c) not in provers:
                provers[id(c)] = (Groth16(c, key), Groth16(c, key, lagrange=True))
            std, lag = provers[id(c)]
            os.environ["ZK_FR_RNS"] = "0"
            ref = [bytes(x) for x in std.qap_eval(wit)]                       # the SAME key through the Fr transforms
            os.environ["ZK_FR_RNS"] = "1"
            got = [bytes(x) for x in std.qap_eval(wit)]
            assert got == ref, tag
            if tag == "h_one":
                assert got[2] == frs([1]) + bytes(32 * (n - 2))
            if tag == "zero":
                assert not any(got[0]) and not any(got[1]) and not any(got[2])
            assert abc_of(std.prove_rs(wit, r, s)) == e, tag + ", tau-power key"
            assert abc_of(lag.prove_rs(wit, r, s)) == e, tag + ", Lagrange-form key"
        check_evaluations(n, abc, *provers[id(cs)][0].qap_eval(w), 0xE7A4 + n)
        with pytest.raises(AssertionError):
            provers[id(cs)][1].prove_rs(bad_witness(n), r, s)
    finally:
        for pair in provers.values():
            for p in pair:
                p.close()
        if old is None:
            os.environ.pop("ZK_FR_RNS", None)
        else:
            os.environ["ZK_FR_RNS"] = old

