"""zk_groth16_pk_specialize on the device against the oracle's setup for the trapdoor (alpha, beta, 1, 1, tau).

The string is [exponent] G through the oracle's point multiplication, never through the library under test.  What is expected:
  * key and verification-key bytes: [e] G for the exponents of the oracle's setup (tests/oracle_lib.py: groth16_setup_exponents);
  * pools: those bytes in the reference's format; the Lagrange-form pools of the host keygen (Groth16.keygen(lagrange=True): exponents in Python
    integers), whose tau-power pools are asserted equal to the oracle's -- and, as the issue asks, the pools of a zk_groth16_keygen handle;
  * proofs: the trapdoor oracle with fixed r, s; on degenerate strings the oracle's literal prover on the key's bytes;
  * masks and the bytes of crafted strings: the integer models (tests/specialize_model.py, tests/key_check_model.py)."""
import ctypes as C
import functools
import json
import os
from collections import namedtuple

import numpy as np
import pytest

import key_check_model as KM
import oracle_lib as O
import specialize_cases as SC
import specialize_model as SM
import test_gpu_options as T
from oracle import pyref as P
from zukelang_amd import _lib
from zukelang_amd.groth16 import SRS, Groth16, _csr, _p

pytestmark = pytest.mark.gpu

R = P.R
ARG, NOT_ON_CURVE, DOMAIN = -1, -2, -8
DMUL = 0x5DE17A00000000000000000000000000000000000000000C0FFEE0003 % R
BLIND = (0x0A11CE + (7 << 180), 0x0B0B + (5 << 222))
SEED = bytes(range(32))
FORMS = ("tau_powers", "lagrange")
CIRCUITS = ["readme"] + ["cubic%d" % n for n in (1, 2, 3, 5, 8, 64, 257)] + ["random256"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def _init_and_leave_nothing_behind():
    _lib.check(_lib.lib().zk_init(0))
    yield
    _lib.set_device_list([0])


World = namedtuple("World", "cs w tox pk1 pk2 vk1 vk2 lag1 lag2 proof")


@functools.lru_cache(maxsize=None)
def world(name, delta=1, alpha=SC.ALPHA, beta=SC.BETA, tau=SC.TAU, literal=False):
    """the key of (alpha, beta, 1, delta, tau) on the circuit: the oracle's bytes, the host keygen's Lagrange pools, the oracle's proof for BLIND"""
    cs, w = SC.circuit(name)
    tox = SC.toxic(alpha, beta, tau, delta)
    e1, e2, eio = O.groth16_setup_exponents(cs.n, cs.m, *SC.csrs(cs), cs.mid, SC.frs(tox))
    pk1, pk2 = O.points_of_exponents_g1(e1), O.points_of_exponents_g2(e2)
    vk1 = O.g1_generator() + O.points_of_exponents_g1(eio)
    vk2 = O.g2_generator() * 2 + O.g2_mul(O.g2_generator(), P.fr_to_bytes(tox[3]))
    it = iter(tox)
    hk, _ = Groth16.keygen(lambda: next(it), cs, lagrange=True)
    assert (bytes(hk.g1), bytes(hk.g2)) == (pk1, pk2), "the host keygen is the oracle's setup"
    r, s = (P.fr_to_bytes(x) for x in BLIND)
    if literal:          # a trapdoor the oracle's trapdoor form does not serve (Z(tau) = 0): its literal prover on the key's bytes
        rc, a, b, c = O.QAP(cs.n, cs.m, *SC.csrs(cs)).groth16_prove(pk1, pk2, cs.mid, SC.frs(w), r, s, 1)
        assert rc == 0
        proof = (a, b, c)
    else:
        proof = O.groth16_prove_trapdoor(cs.n, cs.m, *SC.csrs(cs), cs.mid, SC.frs(w), SC.frs(tox), r, s)
    return World(cs, w, tox, pk1, pk2, vk1, vk2, bytes(hk.lag_g1), bytes(hk.lag_g2), proof)


def pools(wd, form):
    return (wd.lag1, wd.lag2) if form == "lagrange" else (wd.pk1, wd.pk2)


def is_key(pr, wd, form, tag):
    assert (bytes(pr.pool_points(1)), bytes(pr.pool_points(2))) == pools(wd, form), (tag, "pools")
    got = pr.prove_rs(wd.w, *BLIND)
    assert (got.a, got.b, got.c) == wd.proof, (tag, "proof")
    return got


def vk_bytes(vk):
    return bytes(vk.one1) + bytes(vk.ltgm_io), bytes(vk.one2) + bytes(vk.gm) + bytes(vk.d)


def check(pr, form, vkey):
    return (pr.check_lagrange_key if form == "lagrange" else pr.check_key)(vkey, seed=SEED)


def raw(cs, srs, form, bytes_out=True, handle=True, counts=None):
    """the C call itself: (status, pk_g1, pk_g2, vk_g1, vk_g2, handle value), every output filled with 0x5a beforehand"""
    n, m = cs.n, cs.m
    s1 = np.ascontiguousarray(np.concatenate([np.frombuffer(bytes(x), dtype=np.uint8) for x in (srs.tau_g1, srs.alpha_tau_g1, srs.beta_tau_g1)]))
    s2 = np.ascontiguousarray(np.concatenate([np.frombuffer(bytes(x), dtype=np.uint8) for x in (srs.beta_g2, srs.tau_g2)]))
    mid = np.ascontiguousarray(cs.mid, dtype=np.uint8)
    n_mid = int(np.count_nonzero(mid))
    sizes = [len(s1) // 96, len(s2) // 192, 3 + (n + 2) + (n - 1) + n_mid, 2 + (n + 2)]
    g1, g2 = np.full(96 * sizes[2], 0x5A, dtype=np.uint8), np.full(192 * sizes[3], 0x5A, dtype=np.uint8)
    v1, v2 = np.full(96 * (1 + m - n_mid), 0x5A, dtype=np.uint8), np.full(576, 0x5A, dtype=np.uint8)
    for k, v in (counts or {}).items():
        sizes[k] += v
    L, Rm, Om = _csr(cs.L), _csr(cs.R), _csr(cs.O)
    h = C.c_uint64(0)
    o = (lambda a: _p(a)) if bytes_out else (lambda a: None)
    rc = _lib.lib().zk_groth16_pk_specialize(n, m, C.byref(L), C.byref(Rm), C.byref(Om), _p(mid), _p(s1), sizes[0], _p(s2), sizes[1], _lib.KEY_FORMS[form],
                                             o(g1), sizes[2], o(g2), sizes[3], o(v1), o(v2), C.byref(h) if handle else None)
    return rc, bytes(g1), bytes(g2), bytes(v1), bytes(v2), h.value


# ---------------------------------------------------------------- honest strings
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", CIRCUITS)
def test_a_well_formed_string_gives_the_oracles_key(name, form):
    wd, new = world(name), world(name, DMUL)
    cs = wd.cs
    pr, pk, vk = Groth16.specialize(cs, SC.honest_srs(cs.n), form=form)
    try:
        assert (bytes(pk.g1), bytes(pk.g2)) == (wd.pk1, wd.pk2), "key bytes"
        assert vk_bytes(vk) == (wd.vk1, wd.vk2), "verification key"
        it = iter(wd.tox)
        gen = Groth16.generate(lambda: next(it), cs, form=form)[0]
        try:
            assert (bytes(pr.pool_points(1)), bytes(pr.pool_points(2))) == (bytes(gen.pool_points(1)), bytes(gen.pool_points(2))), "the keygen handle's pools"
        finally:
            gen.close()
        proof = is_key(pr, wd, form, (name, form))
        io = [wd.w[k] for k in range(cs.m) if not cs.mid[k]]
        assert Groth16.verify(io, vk, proof)
        assert check(pr, form, vk).failed == 0 and check(pr, form, None).failed == 0
        c = pr.contribute(DMUL)
        proof = is_key(pr, new, form, (name, form, "contributed"))
        assert c.vk_d == new.vk2[384:]
        assert check(pr, form, vk.with_delta(c.vk_d)).failed == 0
        assert check(pr, form, vk).failed != 0          # the old d is not this key's
        assert Groth16.verify(io, vk.with_delta(c.vk_d), proof)
    finally:
        pr.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["cubic1", "cubic5", "random256"])
def test_handle_alone_and_bytes_alone_are_the_same_key(name, form):
    wd = world(name)
    cs, srs = wd.cs, SC.honest_srs(wd.cs.n)
    rc, g1, g2, v1, v2, h = raw(cs, srs, form, bytes_out=False, handle=True)
    assert rc == 0 and h != 0 and g1 == b"\x5a" * len(g1) and v2 == b"\x5a" * 576
    pr = Groth16.__new__(Groth16)
    pr.circuit, pr.rank, pr.world, pr._keep, pr.handle = cs, 0, 1, (cs,), C.c_uint64(h)
    try:
        is_key(pr, wd, form, (name, form, "handle alone"))
    finally:
        pr.close()
    rc, g1, g2, v1, v2, h = raw(cs, srs, form, bytes_out=True, handle=False)
    assert (rc, h) == (0, 0) and (g1, g2, v1, v2) == (wd.pk1, wd.pk2, wd.vk1, wd.vk2)


def test_srs_generate_draws_alpha_beta_tau_and_cut_serves_a_smaller_circuit():
    it = iter([SC.ALPHA, SC.BETA, SC.TAU])
    srs = SRS.generate(lambda: next(it), 8)
    want = SC.honest_srs(8)
    assert [bytes(x) for x in (srs.tau_g1, srs.alpha_tau_g1, srs.beta_tau_g1, srs.beta_g2, srs.tau_g2)] == \
           [bytes(x) for x in (want.tau_g1, want.alpha_tau_g1, want.beta_tau_g1, want.beta_g2, want.tau_g2)]
    wd = world("cubic5")
    pr, pk, vk = Groth16.specialize(wd.cs, srs.cut(5), form="tau_powers")
    try:
        assert (bytes(pk.g1), bytes(pk.g2)) == (wd.pk1, wd.pk2) and vk_bytes(vk) == (wd.vk1, wd.vk2)
    finally:
        pr.close()
    with pytest.raises(ValueError, match="exactly SRS.sizes"):
        Groth16.specialize(wd.cs, srs)


# ---------------------------------------------------------------- degenerate strings: n = 8
DEGENERATE = {"tau=3": dict(tau=3), "tau=0": dict(tau=0), "alpha=0": dict(alpha=0), "beta=0": dict(beta=0)}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("label", list(DEGENERATE))
def test_degenerate_strings_are_served_like_any_other(label, form):
    """tau = 3: the l_i are a unit vector, all three derived lists hold identities, tiztd is all the identity; tau = 0: the powers are the generator
    and identities; alpha = 0, beta = 0: a whole list of identities"""
    kw = dict(dict(alpha=SC.ALPHA, beta=SC.BETA, tau=SC.TAU), **DEGENERATE[label])
    wd = world("cubic8", 1, kw["alpha"], kw["beta"], kw["tau"], True)
    ident = P.g1_to_bytes(None)
    if label == "tau=3":
        assert wd.pk1[96 * 13:96 * 20] == ident * 7
    pr, pk, vk = Groth16.specialize(wd.cs, SC.honest_srs(8, kw["alpha"], kw["beta"], kw["tau"]), form=form)
    try:
        assert (bytes(pk.g1), bytes(pk.g2)) == (wd.pk1, wd.pk2) and vk_bytes(vk) == (wd.vk1, wd.vk2)
        is_key(pr, wd, form, (label, form))
    finally:
        pr.close()


def test_an_all_zero_string_is_a_string_of_identities():
    """Ninety-six zero bytes are how this library's affine format spells the identity, and a key upload reads them so (csrc/msm_points.hip:
    ZERO_IS_IDENTITY); the call checks its points as an upload does.  It therefore serves the string -- the linear map of identities -- and the
    refusal is the key check's: ti1[0] is not the generator."""
    cs, _ = SC.circuit("cubic8")
    n1, nab, n2 = SRS.sizes(8)
    srs = SRS(np.zeros(96 * n1, dtype=np.uint8), np.zeros(96 * nab, dtype=np.uint8), np.zeros(96 * nab, dtype=np.uint8), bytes(192), np.zeros(192 * n2, dtype=np.uint8))
    ex1, ex2, vkm = SM.specialize_exponents(cs, [0] * n1, [0] * nab, [0] * nab, 0, [0] * n2)
    pr, pk, vk = Groth16.specialize(cs, srs, form="tau_powers")
    try:
        assert bytes(pk.g1) == O.points_of_exponents_g1(SC.frs(ex1)) and bytes(pk.g2) == O.points_of_exponents_g2(SC.frs(ex2))
        want = KM.key_check_mask(cs, ex1, ex2, vkm)
        assert want & KM.GENERATORS
        assert pr.check_key(vk, seed=SEED).failed & 0xFF == want
    finally:
        pr.close()


# ---------------------------------------------------------------- crafted strings: the call succeeds, the key check tells
@pytest.mark.parametrize("which", ["alpha", "high_power"])
def test_a_crafted_string_gives_the_models_key_and_the_models_mask(which):
    cs, _ = SC.circuit("cubic8")
    craft = SM.crafted_alpha if which == "alpha" else SM.crafted_high_power
    ex = craft(8, SC.ALPHA % R, SC.BETA % R, SC.TAU % R)
    ex1, ex2, vkm = SM.specialize_exponents(cs, *ex)
    pr, pk, vk = Groth16.specialize(cs, SC.srs_of_exponents(*ex), form="tau_powers")
    try:
        assert bytes(pk.g1) == O.points_of_exponents_g1(SC.frs(ex1)), "pk_g1 = [model exponent] G"
        assert bytes(pk.g2) == O.points_of_exponents_g2(SC.frs(ex2))
        assert vk_bytes(vk)[0] == O.g1_generator() + O.points_of_exponents_g1(SC.frs(vkm["ltgm_io"]))
        want = KM.key_check_mask(cs, ex1, ex2, vkm)
        assert want == (KM.L if which == "alpha" else KM.H_BASES)
        assert pr.check_key(vk, seed=SEED).failed == want
        assert pr.check_key(None, seed=SEED).failed == KM.key_check_mask(cs, ex1, ex2)
    finally:
        pr.close()


# ---------------------------------------------------------------- refusals
def _fixture_points(group, what):
    pts = json.load(open(os.path.join(GOLDEN, "torsion_points.json")))["points"]
    return [bytes.fromhex(t["hex"]) for t in pts if t["group"] == group and t["what"] == what]


LISTS = ("tau_g1", "alpha_tau_g1", "beta_tau_g1", "beta_g2", "tau_g2")


def _with_point(srs, which, pt, at=-1):
    """a copy of the string with one point of list `which` replaced (`at`: index, the last by default)"""
    parts = {k: (bytearray(bytes(getattr(srs, k)))) for k in LISTS}
    size = 96 if which.endswith("g1") else 192
    buf = parts[which]
    i = (len(buf) // size + at) if at < 0 else at
    buf[size * i:size * (i + 1)] = pt
    arr = lambda b: np.frombuffer(bytes(b), dtype=np.uint8).copy()
    return SRS(arr(parts["tau_g1"]), arr(parts["alpha_tau_g1"]), arr(parts["beta_tau_g1"]), bytes(parts["beta_g2"]), arr(parts["tau_g2"]))


def _bad(which, kind):
    g1 = which.endswith("g1")
    good = (O.g1_generator() if g1 else O.g2_generator())
    if kind == "curve":
        b = bytearray(good); b[-1] ^= 1
        return bytes(b)
    if kind == "encoding":
        return b"\x1f" + b"\xff" * 47 + good[48:]          # a coordinate >= p
    return _fixture_points(0 if g1 else 1, "random curve point")[0]          # on the curve, outside the subgroup


@pytest.mark.parametrize("which", LISTS)
def test_a_bad_point_in_any_list_refuses_the_call_and_writes_nothing(which):
    cs, _ = SC.circuit("cubic5")
    srs = SC.honest_srs(5)
    for kind, want in (("curve", NOT_ON_CURVE), ("torsion", NOT_ON_CURVE), ("encoding", ARG)):
        for at in (0, -1):
            rc, g1, g2, v1, v2, h = raw(cs, _with_point(srs, which, _bad(which, kind), at), "tau_powers")
            assert rc == want, (which, kind, at, rc)
            assert h == 0 and set(g1 + g2 + v1 + v2) == {0x5A}, (which, kind, "a refused call writes nothing and leaves no handle")
    with pytest.raises(ValueError):
        Groth16.specialize(cs, _with_point(srs, which, _bad(which, "curve")))


def test_the_first_bad_list_decides():
    cs, _ = SC.circuit("cubic5")
    srs = SC.honest_srs(5)
    for i in range(len(LISTS)):
        for j in range(i + 1, len(LISTS)):
            a = _with_point(_with_point(srs, LISTS[i], _bad(LISTS[i], "curve")), LISTS[j], _bad(LISTS[j], "encoding"))
            assert raw(cs, a, "lagrange")[0] == NOT_ON_CURVE, (LISTS[i], LISTS[j])
            b = _with_point(_with_point(srs, LISTS[i], _bad(LISTS[i], "encoding")), LISTS[j], _bad(LISTS[j], "torsion"))
            assert raw(cs, b, "lagrange")[0] == ARG, (LISTS[i], LISTS[j])


def test_counts_off_by_one_and_a_device_list_of_two():
    cs, _ = SC.circuit("cubic5")
    srs = SC.honest_srs(5)
    for k in range(4):
        for d in (-1, 1):
            rc, g1, g2, v1, v2, h = raw(cs, srs, "tau_powers", counts={k: d})
            assert rc == DOMAIN and h == 0 and set(g1 + g2 + v1 + v2) == {0x5A}, (k, d, rc)
    wd = world("cubic5")
    with T.device_list([0, 0]):
        rc, g1, g2, v1, v2, h = raw(cs, srs, "tau_powers")
        assert rc == ARG and h == 0 and set(g1 + g2 + v1 + v2) == {0x5A}
        rc, g1, g2, v1, v2, h = raw(cs, srs, "tau_powers", handle=False)          # the bytes can be had on any list
        assert rc == 0 and (g1, g2, v1, v2) == (wd.pk1, wd.pk2, wd.vk1, wd.vk2)


@pytest.mark.parametrize("form", FORMS)
def test_without_the_subgroup_check_a_torsion_point_passes_and_the_key_check_refuses_the_handle(form):
    cs, _ = SC.circuit("cubic5")
    srs = _with_point(SC.honest_srs(5), "tau_g1", _bad("tau_g1", "torsion"))
    with T.options({"ZK_KEY_SUBGROUP_CHECK": "0"}):
        pr, pk, vk = Groth16.specialize(cs, srs, form=form)
    try:
        with pytest.raises(_lib.ZkError) as e:
            check(pr, form, None)
        assert e.value.code == ARG and "ZK_KEY_SUBGROUP_CHECK=0" in str(e.value)
        with pytest.raises((ValueError, _lib.ZkError)):
            check(pr, form, vk)
    finally:
        pr.close()
    # an honest string under the same setting: served, same bytes, and refused by the check all the same -- the handle remembers how it was made
    wd = world("cubic5")
    with T.options({"ZK_KEY_SUBGROUP_CHECK": "0"}):
        pr, pk, vk = Groth16.specialize(cs, SC.honest_srs(5), form=form)
    try:
        is_key(pr, wd, form, ("unchecked", form))
        with pytest.raises(_lib.ZkError):
            check(pr, form, None)
    finally:
        pr.close()
