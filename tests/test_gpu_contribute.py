"""zk_groth16_pk_contribute and the multiplication of its tail on the device against what a host setup gives for the trapdoor with delta * delta'.

A contribution multiplies d1 and d2 by delta' and the tail of the G1 pool by 1 / delta'; the handle must then be the one an upload of the contributed
key's bytes gives.  What is expected never comes from the library at its defaults:
  * key bytes: the oracle's setup (tests/oracle_lib.py: QAP.groth16_setup) for (alpha, beta, gamma, delta delta', tau) on the small circuits; at
    n = 1025, and for the Lagrange-form pools at every size, the host keygen (Groth16.keygen(lagrange=True): exponents in Python integers), whose
    tau-power pools are asserted equal to the oracle's on the small circuits -- as tests/test_gpu_options_routes.py takes them;
  * proofs: the trapdoor oracle under that trapdoor with fixed r, s;
  * [delta']_2 and the hook's products: the oracle's point multiplication;
  * masks: tests/key_check_model.py and tests/key_check_lagrange_model.py on the exponents."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import pytest

import key_check_lagrange_model as LM
import key_check_model as KM
import oracle_lib as O
import test_gpu_options as T
from oracle import pyref as P
from test_gpu_prove_many import G16_WIRE, compress
from zukelang_amd import _lib, pinocchio as PIN, r1cs as RC
from zukelang_amd import groth16 as G16
from zukelang_amd.curve import G1, G2
from zukelang_amd.groth16 import Contribution, Groth16

pytestmark = pytest.mark.gpu

R = P.R
LAMBDA = P.BLS_X ** 2 - 1                      # the eigenvalue of the G1 endomorphism the multiplication splits through
TOX = [0x1111 + 7919 * i + (i << 200) for i in range(1, 6)]          # alpha beta gamma delta tau
D1 = 0x5DE17A0000000000000000000000000000000000000000000000000C0FFEE0001 % R
D2 = (R - 0x1234567) % R
BLINDS = [(0x0A11CE + (7 << 180), 0x0B0B + (5 << 222)), (R - 2, 3)]
ARG, HANDLE = -1, -7
SEED = bytes(range(32))
IDENT = P.g1_to_bytes(None)          # the identity as the library writes it; its decoders also read all zeros


def no_row_circuit():
    """hand-built: variable 5 is a mid variable that occurs in no row (its ltd_mid is the identity, and stays it); gate 1 has an all-zero row"""
    L = RC.Matrix.from_rows([{3: 1}, {}, {2: 1, 3: 1, 0: 3}, {1: 2}])
    Rm = RC.Matrix.from_rows([{3: 1}, {3: 1}, {0: 1}, {0: 1}])
    Om = RC.Matrix.from_rows([{1: 1}, {}, {4: 1}, {2: 1}])
    cs = RC.R1CS(4, 6, L, Rm, Om, np.array([0, 1, 1, 1, 0, 1], dtype=np.uint8))
    x = 11
    w = [1, x * x, 2 * x * x, x, 2 * x * x + x + 3, 7]
    assert cs.check(w)
    return cs, w


CIRCUITS = {
    "readme": lambda: RC.readme_circuit(3),
    "one_row": lambda: RC.random_r1cs(1, 4, 9, nnz=(1, 2)),                   # n = 1: tiztd is empty, the tail is ltd_mid alone
    "no_row": no_row_circuit,
    "n1025": lambda: RC.random_r1cs(1025, 1100, 5, nnz=(8, 8)),               # the n1025 of the key-check tests
}
FORMS = ("tau_powers", "lagrange")
ROUTES = {"tau_powers": ("upload", "compressed", "keygen"), "lagrange": ("upload", "compressed", "keygen", "derived")}


@functools.lru_cache(maxsize=None)
def circuit(name):
    cs, w = CIRCUITS[name]()
    return cs, [int(x) for x in w]


def contributed(tox, d):
    return [tox[0], tox[1], tox[2], tox[3] * d % R, tox[4]]


World = namedtuple("World", "cs w tox pk vk exp wire")


@functools.lru_cache(maxsize=None)
def world(name, d):
    """the key of TOX with delta * d, its verification key, and the oracle's proofs under it for BLINDS"""
    cs, w = circuit(name)
    tox = contributed(TOX, d)
    it = iter(tox)
    pk, vk = Groth16.keygen(lambda: next(it), cs, lagrange=True)
    csr = T._csrs(cs)
    if name != "n1025":          # the dense QAP of the oracle's setup is for small circuits
        pk1, pk2, vk1, vk2 = O.QAP(cs.n, cs.m, *csr).groth16_setup(T.frs(tox), cs.mid)
        assert (bytes(pk.g1), bytes(pk.g2)) == (pk1, pk2), "the host keygen is the oracle's setup"
        assert bytes(vk.one1) + bytes(vk.ltgm_io) == vk1 and bytes(vk.one2) + bytes(vk.gm) + bytes(vk.d) == vk2
    exp = [O.groth16_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, T.frs(w), T.frs(tox), P.fr_to_bytes(r), P.fr_to_bytes(s)) for r, s in BLINDS]
    return World(cs, w, tox, pk, vk, exp, [compress(b"".join(e), G16_WIRE) for e in exp])


def pools(wd, form):
    return (bytes(wd.pk.lag_g1), bytes(wd.pk.lag_g2)) if form == "lagrange" else (bytes(wd.pk.g1), bytes(wd.pk.g2))


def make(wd, form, route):
    """a handle of wd's key in `form`, by `route`"""
    lag = form == "lagrange"
    if route == "upload":
        return Groth16(wd.cs, wd.pk, lagrange=lag)
    if route == "compressed":
        g1, g2 = pools(wd, form)
        return Groth16.from_compressed(wd.cs, G1.to_compressed_bytes_many(g1), G2.to_compressed_bytes_many(g2), lagrange=lag)
    if route == "keygen":
        it = iter(wd.tox)
        return Groth16.generate(lambda: next(it), wd.cs, form=form)[0]
    assert route == "derived" and lag
    pr = Groth16(wd.cs, wd.pk)
    pr.derive_lagrange()
    return pr


def is_key(pr, wd, form, tag):
    """the handle holds wd's key: pool bytes of both groups, in both encodings' source, and a lone proof per blind"""
    assert (bytes(pr.pool_points(1)), bytes(pr.pool_points(2))) == pools(wd, form), (tag, "pools")
    for (r, s), want in zip(BLINDS, wd.exp):
        got = pr.prove_rs(wd.w, r, s)
        assert (got.a, got.b, got.c) == want, (tag, "proof")


def is_link(c, old, new, d, tag):
    assert isinstance(c, Contribution)
    assert c.d1_before == bytes(old.pk.g1[96:192]) and c.d1_after == bytes(new.pk.g1[96:192]), (tag, "d1 pair")
    assert c.vk_d == bytes(new.vk.d) == bytes(new.pk.g2[192:384]), (tag, "vk_d")
    assert c.dmul_g2 == O.g2_mul(O.g2_generator(), P.fr_to_bytes(d)), (tag, "[delta']_2")


@functools.lru_cache(maxsize=None)
def old_vkey_masks(name, form):
    """the model's verdict on the CONTRIBUTED key under the OLD verification key: (without a vkey, with it)"""
    cs, _ = circuit(name)
    if form == "tau_powers":
        ex1, ex2, _ = KM.honest_exponents(cs, contributed(TOX, D1))
        _, _, vk_old = KM.honest_exponents(cs, TOX)
        return KM.key_check_mask(cs, ex1, ex2), KM.key_check_mask(cs, ex1, ex2, vk_old)
    lx1, lx2, _ = LM.honest_lagrange_exponents(cs, contributed(TOX, D1))
    _, _, vk_old = LM.honest_lagrange_exponents(cs, TOX)
    return LM.lagrange_mask(cs, lx1, lx2), LM.lagrange_mask(cs, lx1, lx2, vk_old)


@pytest.fixture(autouse=True)
def _init_and_leave_nothing_behind():
    _lib.check(_lib.lib().zk_init(0))
    yield
    _lib.set_device_list([0])          # ZK_ERR_ARG while any key handle is alive


# ---------------------------------------------------------------- the tail's multiplication on bare points (zk_selftest_g1_scale)
def _p8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def scale(pts, k, slab):
    a = np.frombuffer(pts, dtype=np.uint8)
    out = np.zeros(len(a), dtype=np.uint8)
    kb = np.frombuffer(P.fr_to_bytes(k), dtype=np.uint8)
    _lib.check(_lib.lib().zk_selftest_g1_scale(_p8(a), len(a) // 96, _p8(kb), slab, _p8(out)))
    return bytes(out)


@functools.lru_cache(maxsize=None)
def battery():
    """301 points: random subgroup points; the identity first, in the middle and last; P and -P side by side; the generator"""
    st = P.fr_stream(0x5EED0C01)
    g = O.g1_generator()
    pts = [O.g1_mul(g, P.fr_to_bytes(next(st))) for _ in range(301)]
    pts[0] = pts[300] = IDENT
    pts[150] = bytes(96)
    pts[63], pts[64] = pts[62], P.g1_to_bytes(P.pt_neg(P.g1_from_bytes(pts[62])))          # across the end of the first slab at slab = 64
    pts[127] = g
    return pts


SCALARS = [1, 2, R - 1, LAMBDA, LAMBDA + 1, (1 << 128) - 1, 1 << 128, R - LAMBDA] + [next(P.fr_stream(0x5EED0C02 + i)) for i in range(3)]


@pytest.mark.parametrize("k", SCALARS, ids=lambda k: hex(k)[:14])
def test_one_scalar_times_a_list_against_the_oracle_point_by_point(k):
    pts = battery()
    kb = P.fr_to_bytes(k)
    want = b"".join(IDENT if p in (IDENT, bytes(96)) else O.g1_mul(p, kb) for p in pts)
    assert want[:96] == want[96 * 150:96 * 151] == want[96 * 300:] == IDENT
    for slab in (64, 0):          # 64: five chains of launches, each a half-filled workgroup, the last with 45 points; 0: one chain, its third workgroup ends mid-list
        got = scale(b"".join(pts), k, slab)
        bad = [i for i in range(len(pts)) if got[96 * i:96 * i + 96] != want[96 * i:96 * i + 96]]
        assert not bad, (hex(k), slab, bad[:8])


@pytest.mark.parametrize("n", [1, 129])
def test_one_point_and_one_past_a_workgroup(n):
    pts = battery()[1:1 + n]
    for k in (SCALARS[2], SCALARS[-1], 0):
        kb = P.fr_to_bytes(k)
        want = b"".join(O.g1_mul(p, kb) if k else IDENT for p in pts)
        for slab in (0, 128):
            assert scale(b"".join(pts), k, slab) == want, (n, hex(k), slab)


def test_the_hook_refuses_points_that_are_not_points():
    g = bytearray(O.g1_generator())
    g[95] ^= 1
    with pytest.raises(_lib.ZkError) as e:
        scale(bytes(g), 5, 0)
    assert e.value.code == -2


# ---------------------------------------------------------------- the call on every circuit, form and route
@pytest.mark.parametrize("form,route", [(f, r) for f in FORMS for r in ROUTES[f]])
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_a_contributed_handle_is_the_contributed_key(name, form, route):
    old, new = world(name, 1), world(name, D1)
    tag = (name, form, route)
    if name == "no_row":          # the variable no row holds: its point is the identity before and after
        assert bytes(old.pk.g1[-96:]) == IDENT == bytes(new.pk.g1[-96:])
    pr = make(old, form, route)
    try:
        is_key(pr, old, form, (tag, "before"))
        c = pr.contribute(D1)
        is_link(c, old, new, D1, tag)
        is_key(pr, new, form, (tag, "after"))
        assert pr.prove_many(BLINDS, [new.w] * 2, in_flight=2) == new.wire, (tag, "prove_many")
        g1w, g2w = pools(new, form)
        assert bytes(pr.pool_points(1, compressed=True)) == G1.to_compressed_bytes_many(g1w), (tag, "wire pool 1")
        assert bytes(pr.pool_points(2, compressed=True)) == G2.to_compressed_bytes_many(g2w), (tag, "wire pool 2")
        check = pr.check_lagrange_key if form == "lagrange" else pr.check_key
        new_vk = old.vk.with_delta(c.vk_d)
        assert (new_vk.d, bytes(new_vk.gm), bytes(new_vk.ltgm_io), new_vk.ab) == (bytes(new.vk.d), bytes(new.vk.gm), bytes(new.vk.ltgm_io), new.vk.ab)
        assert (check(seed=SEED).failed, check(new_vk, seed=SEED).failed) == (0, 0), (tag, "the new verification key")
        want = old_vkey_masks(name, form)
        assert want == (0, KM.DELTA), "under the old verification key the model fails DELTA alone"
        assert (check(seed=SEED).failed, check(old.vk, seed=SEED).failed) == want, (tag, "the old verification key")
    finally:
        pr.close()


@pytest.mark.parametrize("form", FORMS)
def test_delta_one_changes_no_byte(form):
    old = world("readme", 1)
    pr = make(old, form, "upload")
    try:
        c = pr.contribute(1)
        is_link(c, old, old, 1, form)
        assert c.d1_before == c.d1_after and c.dmul_g2 == O.g2_generator()
        is_key(pr, old, form, (form, "after delta' = 1"))
    finally:
        pr.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["readme", "n1025"])
def test_two_contributions_are_one_with_the_product(name, form):
    old, mid, new = world(name, 1), world(name, D1), world(name, D1 * D2 % R)
    one, two = make(old, form, "upload"), make(old, form, "upload")
    try:
        c1 = one.contribute(D1)
        c2 = one.contribute(D2)
        is_link(c1, old, mid, D1, (name, form, 1))
        is_link(c2, mid, new, D2, (name, form, 2))
        c = two.contribute(D1 * D2 % R)
        is_link(c, old, new, D1 * D2 % R, (name, form, "product"))
        is_key(one, new, form, (name, form, "two calls"))
        is_key(two, new, form, (name, form, "one call"))
    finally:
        one.close()
        two.close()


@pytest.mark.parametrize("name", ["readme", "one_row", "n1025"])
def test_contribute_and_derive_commute(name):
    """contribute then derive = derive then contribute = the Lagrange keygen of the new trapdoor"""
    old, new = world(name, 1), world(name, D1)
    a, b = make(old, "tau_powers", "upload"), make(old, "tau_powers", "upload")
    try:
        a.contribute(D1)
        a.derive_lagrange()
        b.derive_lagrange()
        b.contribute(D1)
        is_key(a, new, "lagrange", (name, "contribute, derive"))
        is_key(b, new, "lagrange", (name, "derive, contribute"))
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- what the handle cached over the old tables
@pytest.mark.parametrize("graph", ["0", "1"])
@pytest.mark.parametrize("form", FORMS)
def test_slots_used_before_the_call_prove_under_the_new_key(form, graph):
    old, new = world("n1025", 1), world("n1025", D1)
    with T.options({"ZK_GRAPH": graph}):
        pr = make(old, form, "upload")
        try:
            assert pr.prove_many(BLINDS, [old.w] * 2, in_flight=2) == old.wire          # slots 0 and 1: workspaces, and with graph = 1 captured proofs
            pr.contribute(D1)
            for slot, (r, s) in enumerate(BLINDS):
                pr.prove_async(new.w, r, s, slot)
            got = [pr.prove_wait(slot) for slot in range(2)]
            assert [(g.a, g.b, g.c) for g in got] == new.exp, (form, graph, "the same slots")
            assert pr.prove_many(BLINDS, [new.w] * 2, in_flight=2) == new.wire, (form, graph, "prove_many again")
        finally:
            pr.close()


# ---------------------------------------------------------------- refusals on the device: the handle proves as before
def _raw_contribute(handle, d=D1):
    kb = np.frombuffer(P.fr_to_bytes(d), dtype=np.uint8)
    return _lib.lib().zk_groth16_pk_contribute(handle, _p8(kb), None, None, None)


def test_a_proof_in_flight_refuses_the_call():
    old = world("readme", 1)
    pr = make(old, "tau_powers", "upload")
    try:
        r, s = BLINDS[0]
        pr.prove_async(old.w, r, s, 1)
        with pytest.raises(_lib.ZkError) as e:
            pr.contribute(D1)
        assert e.value.code == ARG and "in flight" in str(e.value)
        g = pr.prove_wait(1)
        assert (g.a, g.b, g.c) == old.exp[0]
        is_key(pr, old, "tau_powers", "after the refusal")
    finally:
        pr.close()


def test_a_shard_refuses_the_call():
    old = world("readme", 1)
    shards = [Groth16(old.cs, old.pk, rank=k, world=2) for k in range(2)]
    try:
        assert _raw_contribute(shards[0].handle) == ARG and b"shard" in _lib.lib().zk_last_error()
        r, s = BLINDS[0]
        w, rb, sb = (np.frombuffer(x, dtype=np.uint8) for x in (T.frs(old.w), P.fr_to_bytes(r), P.fr_to_bytes(s)))
        parts = np.concatenate([sh.prove_partial(w, rb, sb) for sh in shards])
        out = np.zeros(384, dtype=np.uint8)
        _lib.check(_lib.lib().zk_groth16_combine(_p8(parts), C.c_uint32(2), _p8(out)))
        assert (bytes(out[:96]), bytes(out[96:288]), bytes(out[288:])) == old.exp[0]
    finally:
        for sh in shards:
            sh.close()


def test_a_multi_device_handle_refuses_the_call():
    old = world("readme", 1)
    with T.device_list([0, 0]):
        pr = make(old, "tau_powers", "upload")
        try:
            assert _raw_contribute(pr.handle) == ARG and b"multi-device" in _lib.lib().zk_last_error()
            got = pr.prove_rs(old.w, *BLINDS[0])
            assert (got.a, got.b, got.c) == old.exp[0]
        finally:
            pr.close()


def test_a_pinocchio_handle_and_a_freed_handle_are_no_handles():
    old = world("readme", 1)
    st = P.fr_stream(0x5EED0C03)
    tox = [next(st) for _ in range(8)]
    it = iter(tox)
    ppk, _ = PIN.ZK.keygen(lambda: next(it), old.cs)
    pin = PIN.ZK(old.cs, ppk)
    ds = [next(st) for _ in range(3)]
    want = O.pinocchio_prove_trapdoor(old.cs.n, old.cs.m, *T._csrs(old.cs), old.cs.mid, T.frs(old.w), T.frs(tox), *(P.fr_to_bytes(x) for x in ds))
    try:
        assert _raw_contribute(pin.handle) == HANDLE
        assert pin.prove_with(old.w, *ds).to_bytes() == want
    finally:
        pin.close()
    pr = make(old, "tau_powers", "upload")
    h = C.c_uint64(pr.handle.value)
    pr.close()
    assert _raw_contribute(h) == HANDLE
    assert _raw_contribute(C.c_uint64(0x7777)) == HANDLE


# ---------------------------------------------------------------- the links, and the verifier's view
def test_verify_contributions_and_the_verifier():
    old, mid, new = world("readme", 1), world("readme", D1), world("readme", D1 * D2 % R)
    pr = make(old, "tau_powers", "upload")
    try:
        c1 = pr.contribute(D1)
        c2 = pr.contribute(D2)
        last = bytes(pr.pool_points(1)[96:192])
        proof = pr.prove_rs(new.w, *BLINDS[0])
    finally:
        pr.close()
    first = bytes(old.pk.g1[96:192])
    assert last == c2.d1_after == bytes(new.pk.g1[96:192])
    l1, l2 = (c1.d1_before, c1.d1_after, c1.dmul_g2), (c2.d1_before, c2.d1_after, c2.dmul_g2)
    assert G16.verify_contributions(first, [c1, c2], last) and G16.verify_contributions(first, [l1, l2], last)
    assert G16.verify_contributions(first, [l1], c1.d1_after) and G16.verify_contributions(c1.d1_after, [l2], last)
    assert not G16.verify_contributions(first, [l2, l1], last), "swapped links"
    other = O.g2_mul(O.g2_generator(), P.fr_to_bytes(D1 + 1))
    assert not G16.verify_contributions(first, [(l1[0], l1[1], other), l2], last), "[delta']_2 of another scalar"
    assert not G16.verify_contributions(first, [l1, (l2[0], l2[1], l1[2])], last), "[delta']_2 of the other link"
    assert not G16.verify_contributions(first, [l1], last), "a chain that stops short of the key's d1"
    assert not G16.verify_contributions(first, [l1, l2], bytes(mid.pk.g1[96:192])), "a chain that does not end at the key's d1"
    assert not G16.verify_contributions(first, [l1, l2, (last, last, P.g2_to_bytes(None))], last), "delta' = identity"
    # the contributed proofs verify under with_delta and not under the old verification key (host path)
    io = [new.w[k] for k in range(new.cs.m) if not new.cs.mid[k]]
    new_vk = old.vk.with_delta(c2.vk_d)
    assert (proof.a, proof.b, proof.c) == new.exp[0]
    assert Groth16.verify(io, new_vk, proof) is True
    assert Groth16.verify(io, old.vk, proof) is False
    assert Groth16.verify(io, old.vk.with_delta(c1.vk_d), proof) is False
