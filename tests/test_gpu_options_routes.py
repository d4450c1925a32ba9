"""GPU parity under every public option ON EVERY ROUTE TO A HANDLE (tests/option_cases.py: ROUTES).  tests/test_gpu_options.py holds the promise of
include/zkmi355x.h -- no knob of zk_set_option changes a result -- through the uncompressed upload; the wire decoder, the generated pools, the key
cache, the key checks, the uploaded h bases and the resident MSM bases build their tables, workspaces and sorts on paths of their own and read the
same options.  Here every live setting of CASES, every cached group and the named interactions run through each of them.

What is expected never comes from the library at its default options: proofs from the trapdoor oracles (the setups of tests/test_gpu_options.py,
computed once per session), their wire form through the oracle's compressor, sums from the oracle's naive fold, masks from the integer models
(asserted equal to the hand-derived BITS), key bytes from the host keygen.  The one exception: the Lagrange pools a derived handle hands out are
compared with keygen(lagrange=True)'s, as tests/test_gpu_key_wire.py does."""
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

import key_check_cases as KC
import key_check_lagrange_cases as LC
import key_check_model as KM
import oracle_lib as O
import test_gpu_key_check as TK
import test_gpu_key_check_lagrange as TL
import test_gpu_msm_resident as TR
import test_gpu_options as T
from option_cases import CACHED_GROUPS, FLIPS, ROUTES, live_runs, route_settings
from test_gpu_keygen import raw_keygen
from test_gpu_prove_many import G16_WIRE, PIN_WIRE, compress
from zukelang_amd import _lib
from zukelang_amd import pinocchio as PIN
from zukelang_amd.curve import G1, G2
from zukelang_amd.groth16 import Groth16, _lagrange_at
from zukelang_amd.r1cs import FR_MODULUS, fr_bytes

pytestmark = pytest.mark.gpu

FORMS = ("lagrange", "tau_powers")
SEED = TK.SEEDS[0]
# one crafted key per region of the pools, so that every product of the check has a verdict to flip (tests/key_check_cases.py, key_check_lagrange_cases.py)
TAU_KEYS = ("honest", "ti1_middle", "ti2_other_tau", "b2_other_beta", "tiztd_one", "ltd_mid_opposite")
LAG_KEYS = ("honest", "l1_opposite", "l2_one", "b1_other", "hl_opposite", "ltd_mid_opposite")
FLIP_KEYS = ("honest", "ltd_mid_opposite")
RESIDENT_SIZES = (300, 2000)

Wire = namedtuple("Wire", "g16_w g16_w3 g16_exp g1w g2w lag_g1 lag_g2 lag_g1w lag_g2w pin_w pin_w3 pin_exp q1w q2w hl hlw")
_wires = {}


def wires(size):
    """What the routes need beside the setups of tests/test_gpu_options.py, per size and once per module: the witnesses as bytes, the oracle's proofs
    in wire form, the keys' wire bytes, the Lagrange-form pools of the Groth16 key and the h bases [lambda_t(s)] (n-1) | [Z(s)] of the Pinocchio key
    from its trapdoor.  Called before any option is set."""
    if size in _wires:
        return _wires[size]
    g16, pin = T.setups(size)
    it = iter(g16.toxic)
    lag, _ = Groth16.keygen(lambda: next(it), g16.cs, lagrange=True)
    assert bytes(lag.g1) == bytes(g16.pk.g1) and bytes(lag.g2) == bytes(g16.pk.g2)
    n, s = pin.cs.n, pin.toxic[2] % FR_MODULUS                    # keygen draws rv, rw, s, ...
    lam, _ = _lagrange_at(n - 1, (s - n) % FR_MODULUS)           # the basis of the points n .. 2n-2 at s
    _, zs = _lagrange_at(n, s)
    hl = bytes(G1.of_Fr(fr_bytes(lam + [zs])))
    gw, pw = np.frombuffer(T.frs(g16.w), dtype=np.uint8), np.frombuffer(T.frs(pin.w), dtype=np.uint8)
    c1, c2 = G1.to_compressed_bytes_many, G2.to_compressed_bytes_many
    _wires[size] = Wire(gw, np.tile(gw, (3, 1)), [compress(b"".join(e), G16_WIRE) for e in g16.exp], c1(g16.pk.g1), c2(g16.pk.g2),
                        bytes(lag.lag_g1), bytes(lag.lag_g2), c1(lag.lag_g1), c2(lag.lag_g2),
                        pw, np.tile(pw, (3, 1)), [compress(e, PIN_WIRE) for e in pin.exp], c1(pin.pk.g1), c2(pin.pk.g2), hl, c1(hl))
    return _wires[size]


# ---- the proving routes: one lone proof, then three witnesses in one call with two in flight (slot 1 is allocated after the first proof)
def g16_lone(pr, s, wr, tag):
    got = pr.prove_rs(wr.g16_w, *s.blind[0])
    assert (got.a, got.b, got.c) == s.exp[0], (tag, "lone")


def g16_many(pr, s, wr, tag):
    assert pr.prove_many(s.blind, wr.g16_w3, in_flight=2) == wr.g16_exp, (tag, "prove_many")


def pin_lone(pr, s, wr, tag):
    assert pr.prove_with(wr.pin_w, *s.blind[0]).to_bytes() == s.exp[0], (tag, "ZK")
    assert PIN.NonZK.prove(pr, None, wr.pin_w).to_bytes() == s.exp[3], (tag, "NonZK")


def pin_many(pr, s, wr, tag):
    assert pr.prove_many(s.blind[:3], wr.pin_w3, in_flight=2) == wr.pin_exp[:3], (tag, "prove_many")


def _generate(cls, s, form):
    it = iter(s.toxic)
    return cls.generate(lambda: next(it), s.cs, form=form)


def _same_key(pk, s, tag):
    assert bytes(pk.g1) == bytes(s.pk.g1) and bytes(pk.g2) == bytes(s.pk.g2), (tag, "key bytes")


# route -> [(how the handle came to be, maker)]: every maker returns a prover whose proofs must be the oracle's; it asserts what the route says of
# the key's bytes on the way
def _g16_wire(s, wr, tag):
    return Groth16.from_compressed(s.cs, wr.g1w, wr.g2w)


def _g16_generated(form):
    def make(s, wr, tag):
        pr, pk, _vk = _generate(Groth16, s, form)
        try:
            _same_key(pk, s, tag)
            want = (wr.lag_g1, wr.lag_g2) if form == "lagrange" else (bytes(s.pk.g1), bytes(s.pk.g2))
            assert (bytes(pr.pool_points(1)), bytes(pr.pool_points(2))) == want, (tag, "pools")
        except BaseException:
            pr.close()
            raise
        return pr
    return make


def _g16_cached_lagrange(s, wr, tag):
    derived = Groth16(s.cs, s.pk)
    try:
        derived.derive_lagrange()
        p1, p2 = bytes(derived.pool_points(1, compressed=True)), bytes(derived.pool_points(2, compressed=True))
    finally:
        derived.close()
    assert p1 == wr.lag_g1w and p2 == wr.lag_g2w, (tag, "derived pools in wire form")
    return Groth16.from_compressed(s.cs, p1, p2, lagrange=True)


def _pin_wire(with_h):
    def make(s, wr, tag):
        pr = PIN.ZK.from_compressed(s.cs, wr.q1w, wr.q2w, h_lagrange=wr.hlw if with_h else None)
        if with_h:
            try:
                assert bytes(pr.pool_points(5, compressed=True))[:len(wr.hlw)] == wr.hlw, (tag, "h bases")
            except BaseException:
                pr.close()
                raise
        return pr
    return make


def _pin_generated(form):
    def make(s, wr, tag):
        pr, pk, _vk = _generate(PIN.ZK, s, form)
        try:
            _same_key(pk, s, tag)
        except BaseException:
            pr.close()
            raise
        return pr
    return make


def _pin_lagrange(s, wr, tag):
    pr = PIN.ZK.from_lagrange(s.cs, s.pk, np.frombuffer(wr.hl, dtype=np.uint8))
    try:
        assert bytes(pr.pool_points(5))[:len(wr.hl)] == wr.hl, (tag, "h bases")
    except BaseException:
        pr.close()
        raise
    return pr


MAKERS = {
    "g16_wire": [("wire", _g16_wire)],
    "g16_generated": [(f, _g16_generated(f)) for f in FORMS],
    "g16_cached_lagrange": [("cached", _g16_cached_lagrange)],
    "pin_wire": [("wire", _pin_wire(False)), ("wire + h_lagrange", _pin_wire(True))],
    "pin_generated": [(f, _pin_generated(f)) for f in FORMS],
    "pin_lagrange": [("from_lagrange", _pin_lagrange)],
}
PROVING = list(MAKERS)


def _proto(route, size):
    g16, pin = T.setups(size)
    return (g16, g16_lone, g16_many) if ROUTES[route].protocol == "groth16" else (pin, pin_lone, pin_many)


def run_proving(route, size, tag, device_list=False):
    s, lone, many = _proto(route, size)
    wr = wires(size)
    for how, make in MAKERS[route]:
        if device_list and "h_lagrange" in how:
            continue          # uploaded h bases are for single-device keys: refused on a list (tests/test_gpu_key_wire.py)
        pr = make(s, wr, (tag, how))
        try:
            lone(pr, s, wr, (tag, how))
            many(pr, s, wr, (tag, how))
        finally:
            pr.close()


def run_keygen_on_a_device_list(route, size, tag):
    """zk_*_keygen on a device list: no handle (ZK_ERR_ARG), and without one the key bytes are still keygen's"""
    s, _lone, _many = _proto(route, size)
    proto = ROUTES[route].protocol
    for form in (0, 1):
        assert raw_keygen(proto, s.cs, T.frs(s.toxic), form=form)[0] == -1, (tag, form, "a handle on a device list")
        rc, got, _ = raw_keygen(proto, s.cs, T.frs(s.toxic), form=form, handle=False)
        assert rc == 0 and got[0] == bytes(s.pk.g1) and got[1] == bytes(s.pk.g2), (tag, form, "key bytes")


# ---- the key checks: the n1025 circuit of tests/test_gpu_key_check.py, points and wanted masks once per module
KeySet = namedtuple("KeySet", "cs tau lag")
_keys = []


def key_set():
    """name -> (PKey, VKey, (mask without a verification key, mask with it)) per key form; the masks are the models', and the models' are BITS'"""
    if _keys:
        return _keys[0]
    cs = TK.circuit("n1025")
    tau, lag = {}, {}
    cases = {c[0]: c for c in KC.crafted(cs, TK.TOX)}
    for name in TAU_KEYS:
        _, ex1, ex2, vk = cases[name]
        want = (KM.key_check_mask(cs, ex1, ex2), KM.key_check_mask(cs, ex1, ex2, vk))
        assert want == KC.BITS[name], name
        tau[name] = TK.points(ex1, ex2, vk) + (want,)
    cases = {c[0]: c for c in LC.crafted(cs, TL.TOX)}
    for name in LAG_KEYS:
        _, lx1, lx2, vk = cases[name]
        want = TL.model_masks(cs, lx1, lx2, vk)
        assert want == LC.BITS[name], name
        lag[name] = TL.points(lx1, lx2, vk) + (want,)
    assert {w for _, _, w in tau.values()} | {w for _, _, w in lag.values()} >= {(0, 0), (KM.L,) * 2, (KM.H_BASES,) * 2}
    _keys.append(KeySet(cs, tau, lag))
    return _keys[0]


def _upload(ks, form, name):
    if form == "tau_powers":
        pk, vkey, want = ks.tau[name]
        pr = Groth16(ks.cs, pk)
        return pr, pr.check_key, vkey, want
    pk, vkey, want = ks.lag[name]
    pr = Groth16(ks.cs, pk, lagrange=True)
    return pr, pr.check_lagrange_key, vkey, want


def _checked(check, vkey, want, tag):
    assert (check(seed=SEED).failed, check(vkey, seed=SEED).failed) == want, tag


def _refused(check, vkey, tag):
    """a handle uploaded without the subgroup test: the contract is the refusal, with and without a verification key"""
    for v in (None, vkey):
        with pytest.raises((_lib.ZkError, ValueError)) as e:          # with a verification key the wrapper words a refusal as the wire readers do
            check(v, seed=SEED)
        assert "libzkmi355x error -1:" in str(e.value) and "SUBGROUP_CHECK" in str(e.value), tag


def run_key_check(settings, tag):
    ks = key_set()
    unchecked = str(settings.get("ZK_KEY_SUBGROUP_CHECK", "1")) == "0"
    for form, keys in (("tau_powers", TAU_KEYS), ("lagrange", LAG_KEYS)):
        for name in keys:
            pr, check, vkey, want = _upload(ks, form, name)
            try:
                if unchecked:
                    _refused(check, vkey, (tag, form, name))
                else:
                    _checked(check, vkey, want, (tag, form, name))
            finally:
                pr.close()


# ---- resident MSM bases: the point lists of tests/test_gpu_msm_resident.py (the identity, a duplicate, a P / -P pair), scalars led by 0, 1, r - 1
_resident = []


def resident_cases():
    """(G, n, bases, their wire bytes, [(scalars, the oracle's naive fold)]) -- the full list, a 16-scalar prefix, and the lengths (n, 64, 1) of one
    _many call: n takes the chain, 64 and 1 the short table beside it (short_max is 256 in G1, 64 in G2)"""
    if not _resident:
        for G in (G1, G2):
            for n in RESIDENT_SIZES:
                bases = TR._bases(G, n, 0x0A00 + n)
                cs = [TR._scalars(k, 0x0B00 + n + k) for k in (n, 16, n, 64, 1)]
                _resident.append((G, n, bases, G.to_compressed_bytes_many(bases), [(c, TR._oracle(G, bases, c)) for c in cs]))
    return _resident


def run_resident(tag):
    for G, n, bases, wire, cs in resident_cases():
        for how, up in (("bytes", lambda: G.resident(bases)), ("wire", lambda: G.resident_compressed(wire))):
            with up() as rb:
                assert (rb.n, rb.short_max) == (n, 256 if G is G1 else 64)
                for c, want in cs[:2]:
                    assert bytes(rb.apply_powers(c)) == want, (tag, G.__name__, n, how, len(c) // 32)
                many = [bytes(p) for p in rb.apply_powers_many([c for c, _ in cs[2:]])]
                assert many == [want for _, want in cs[2:]], (tag, G.__name__, n, how, "many")


def run_route(route, size, settings, tag):
    if route == "g16_key_check":
        run_key_check(settings, tag)
    elif route == "resident":
        run_resident(tag)
    else:
        run_proving(route, size, tag)


def prepare(route, size):
    """everything a route computes once, at the library's default options: before the first option is set"""
    _lib.check(_lib.lib().zk_init(0))
    if route == "g16_key_check":
        key_set()
    elif route == "resident":
        resident_cases()
    else:
        wires(size)


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    yield
    _lib.set_device_list([0])          # ZK_ERR_ARG while any handle is alive: every route has closed its own


# ---- every live setting through every route
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("c,settings", [pytest.param(c, settings, id=rid) for rid, c, settings in live_runs()])
def test_a_live_option_on_every_route(c, settings, route):
    prepare(route, c.size)
    settings = route_settings(route, c, settings)
    with T.options(settings):
        run_route(route, c.size, settings, (settings, route))


@pytest.mark.parametrize("route", [r for r in ROUTES if ROUTES[r].multi])
@pytest.mark.parametrize("c,settings", [pytest.param(c, settings, id=rid) for rid, c, settings in live_runs() if c.multi])
def test_a_key_option_on_a_device_list(c, settings, route):
    prepare(route, c.size)
    with T.device_list([0, 0]), T.options(settings):
        if ROUTES[route].multi == "bytes":
            run_keygen_on_a_device_list(route, c.size, (settings, route, "x2"))
        else:
            run_proving(route, c.size, (settings, route, "x2"), device_list=True)


# ---- cached knobs: one fresh process per group runs every route at "small", without ZK_TEST_FORMS (tests/test_gpu_options.py)
def child_main(group):
    _lib.check(_lib.lib().zk_init(0))
    for k, v in CACHED_GROUPS[group].items():
        T.set_option(k, v)                      # before anything else: they are cached at first use
    for route in ROUTES:
        prepare(route, "small")
    for route in ROUTES:
        run_route(route, "small", CACHED_GROUPS[group], (CACHED_GROUPS[group], route))
    print("CACHED-ROUTES-OK %d" % group)


@pytest.mark.parametrize("group", range(len(CACHED_GROUPS)))
def test_cached_options_on_every_route_in_a_fresh_process(group):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_options_routes as R; R.child_main(%d)" % (root, here, group)
    keep = ("ZK_LIBZKMI355X_PATH", "ZK_ORACLE_SO")                  # which build of the library / oracle, not knobs
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZK_") or k in keep}
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert res.returncode == 0 and "CACHED-ROUTES-OK %d" % group in res.stdout, (CACHED_GROUPS[group], res.stdout[-2000:] + res.stderr[-4000:])


# ---- named interactions: the options of ONE handle read at different moments.  Tables are built at upload; a slot's workspaces (batch-affine rounds,
# the sort's levels) when the slot is first used; the key checks' workspaces and their non-table base set per call.
def _flip(fid, direction):
    return ({}, FLIPS[fid]) if direction == "set" else (FLIPS[fid], {})


FLIP_PARAMS = [pytest.param(fid, d, id="%s-%s" % (fid, d)) for fid in FLIPS for d in ("set", "unset")]


@pytest.mark.parametrize("route", PROVING)
@pytest.mark.parametrize("fid,direction", FLIP_PARAMS)
def test_a_handle_made_under_one_setting_proves_under_another(fid, direction, route):
    """two handles made under A: the first meets B untouched, the second has proved once under A -- its slot 0 keeps A's workspaces and prove_many
    allocates slot 1 under B beside them (msm_accumulate_sorted takes the minimum of a batch's rounds)"""
    prepare(route, "small")
    a, b = _flip(fid, direction)
    s, lone, many = _proto(route, "small")
    wr = wires("small")
    how, make = MAKERS[route][-1]
    tag = (route, how, a, b)
    made = []
    try:
        with T.options(a):
            made.append(make(s, wr, tag))
            made.append(make(s, wr, tag))
            lone(made[1], s, wr, (tag, "under A"))
        with T.options(b):
            lone(made[0], s, wr, (tag, "made under A, lone under B"))
            many(made[0], s, wr, (tag, "made under A, many under B"))
            many(made[1], s, wr, (tag, "slot 0 under A, slot 1 under B"))
            lone(made[1], s, wr, (tag, "slot 0 again"))
    finally:
        for pr in made:
            pr.close()


def test_a_point_outside_the_subgroup_never_meets_folded_digits_on_the_wire_routes():
    """Folded digits compute (r - s)(-P), which is s P only for a point of order r (msm.cuh: msm_fold).  With ZK_KEY_SUBGROUP_CHECK=0 a point outside the
    subgroup enters a key or a base list; at the widths that fold, its handle must still give s P: the literal oracle on THAT key (generic point
    arithmetic, no subgroup assumed), the naive fold on THAT list.  The honest keys of every other test cannot tell: their points have order r."""
    from oracle import pyref as P
    from zukelang_amd import r1cs as RC
    _lib.check(_lib.lib().zk_init(0))
    outside = P.g1_to_bytes(TR._point_outside_the_subgroup())
    cs, w = RC.iterated_cubic(6, 9)
    st = P.fr_stream(0x5EED0A00)
    toxic = [next(st) for _ in range(5)]
    r, s = P.R - 12345, P.R - 777                                       # min(x, r - x) is x itself below r / 2: only a scalar above it tells
    it = iter(toxic)
    pk, _ = Groth16.keygen(lambda: next(it), cs)
    g1 = bytes(pk.g1)[:192] + outside + bytes(pk.g1)[288:]             # b1: read by C alone, with the scalar r
    q = O.QAP(cs.n, cs.m, *T._csrs(cs))
    literal = lambda key1: q.groth16_prove(key1, bytes(pk.g2), cs.mid, T.frs(w), P.fr_to_bytes(r), P.fr_to_bytes(s), 1)
    rc, *want = literal(g1)
    rc0, *honest = literal(bytes(pk.g1))
    assert rc == 0 and rc0 == 0 and want[:2] == honest[:2] and want[2] != honest[2], "the proof reads the replaced point"
    g1w, g2w = G1.to_compressed_bytes_many(g1), G2.to_compressed_bytes_many(pk.g2)
    for width in (3, 5, 15, 17):
        with T.options({"ZK_MSM_WINDOW": width, "ZK_KEY_SUBGROUP_CHECK": "0"}):
            pr = Groth16.from_compressed(cs, g1w, g2w)
            try:
                got = pr.prove_rs(w, r, s)
                assert [got.a, got.b, got.c] == want, (width, "lone")
                assert pr.prove_many([(r, s)] * 3, [w] * 3, in_flight=2) == [compress(b"".join(want), G16_WIRE)] * 3, (width, "prove_many")
            finally:
                pr.close()
    # resident bases: the narrow table of the short path is 5 bits wide whatever the options say
    bases = np.array(TR._bases(G1, 40, 31), copy=True)
    bases[96 * 7:96 * 8] = np.frombuffer(outside, dtype=np.uint8)
    cs_ = [np.array(TR._scalars(k, 0x0C00 + k), copy=True) for k in (40, 8, 40, 17, 8)]
    for c in cs_:
        c[32 * 7:32 * 8] = np.frombuffer(P.fr_to_bytes(P.R - 3 - len(c) // 32), dtype=np.uint8)          # above r / 2 on the replaced point
    want = [TR._oracle(G1, bases, c) for c in cs_]
    assert want[1] != TR._oracle(G1, TR._bases(G1, 40, 31), cs_[1]), "the products read the replaced point"
    wire = G1.to_compressed_bytes_many(bases)
    with T.options({"ZK_KEY_SUBGROUP_CHECK": "0"}):
        handles = [G1.resident(bases), G1.resident_compressed(wire)]
    for rb in handles:
        with rb:
            assert [bytes(rb.apply_powers(c)) for c in cs_[:2]] == want[:2]
            assert [bytes(p) for p in rb.apply_powers_many(cs_[2:])] == want[2:]


@pytest.mark.parametrize("fid,direction", FLIP_PARAMS)
def test_a_key_uploaded_under_one_setting_is_checked_under_another(fid, direction):
    prepare("g16_key_check", "small")
    a, b = _flip(fid, direction)
    ks = key_set()
    for form in ("tau_powers", "lagrange"):
        for name in FLIP_KEYS:
            with T.options(a):
                pr, check, vkey, want = _upload(ks, form, name)
            try:
                with T.options(b):
                    _checked(check, vkey, want, (a, b, form, name))
            finally:
                pr.close()
