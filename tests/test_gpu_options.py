"""GPU parity under every public option (tests/option_cases.py): include/zkmi355x.h promises that no knob of zk_set_option changes a result.
Each value is set through zk_set_option before the key is uploaded (a host's real path) and stays set for the whole run: Groth16 (groth16.ml:116-161)
and Pinocchio ZK / NonZK (pinocchio.ml:427-514), tau-power form and derived form, one proof and three pipelined slots, byte for byte against the
trapdoor oracles.  Cached knobs run in child processes; the interactions that broke go by name at the end."""
import os
import subprocess
import sys
from collections import namedtuple
from contextlib import contextmanager

import numpy as np
import pytest

import oracle_lib as O
from oracle import pyref as P
from option_cases import CACHED_GROUPS, CASES, live_runs
from zukelang_amd import _lib, r1cs as RC
from zukelang_amd import pinocchio as PIN
from zukelang_amd.groth16 import Groth16

pytestmark = pytest.mark.gpu

SIZES = {"small": (1 << 12, 1000), "ba": (1 << 14, 1 << 14)}          # (Groth16 constraints, Pinocchio constraints)
DEVICE_LISTS = ([0, 0], [0, 0, 0])
Setup = namedtuple("Setup", "cs w csr toxic pk blind exp")


def frs(xs):
    return b"".join(P.fr_to_bytes(x) for x in xs)


def _csrs(cs):
    return [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]


def set_option(name, value):
    _lib.check(_lib.lib().zk_set_option(name.encode(), None if value is None else str(value).encode()))


@contextmanager
def options(settings):
    try:
        for k, v in settings.items():
            set_option(k, v)
        yield
    finally:
        for k in settings:
            set_option(k, None)


def groth16_setup(n):
    """a key of iterated_cubic(n) and three (r, s) with their trapdoor-oracle proofs"""
    cs, w = RC.iterated_cubic(n, 0x0971 + n)
    st = P.fr_stream(0x5EED0700 + n)
    toxic = [next(st) for _ in range(5)]
    it = iter(toxic)
    pk, _ = Groth16.keygen(lambda: next(it), cs)
    rs = [(next(st), next(st)) for _ in range(3)]
    csr = _csrs(cs)
    exp = [O.groth16_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), frs(toxic), P.fr_to_bytes(r), P.fr_to_bytes(s)) for r, s in rs]
    return Setup(cs, w, csr, toxic, pk, rs, exp)


def pinocchio_setup(n, maker=None):
    """a key of iterated_cubic(n) (or maker()), three blindings (dv, dw, dy) and the NonZK zeros, with their trapdoor-oracle proofs"""
    cs, w = maker() if maker else RC.iterated_cubic(n, 0x0972 + n)
    st = P.fr_stream(0x5EED0800 + cs.n)
    tox = [next(st) for _ in range(8)]
    it = iter(tox)
    pk, _ = PIN.ZK.keygen(lambda: next(it), cs)
    ds = [[next(st) for _ in range(3)] for _ in range(3)] + [[0, 0, 0]]
    csr = _csrs(cs)
    exp = [O.pinocchio_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), frs(tox), *(P.fr_to_bytes(x) for x in d)) for d in ds]
    return Setup(cs, w, csr, tox, pk, ds, exp)


def run_groth16(s, tag):
    pr = Groth16(s.cs, s.pk)
    try:
        for form in ("tau powers", "derived"):
            if form == "derived":
                pr.derive_lagrange()
            got = pr.prove_rs(s.w, *s.blind[0])
            assert (got.a, got.b, got.c) == s.exp[0], (tag, form, "lone")
            pr.set_witness(s.w)
            for slot, (r, r2) in enumerate(s.blind):
                pr.prove_async(None, r, r2, slot)
            got = [pr.prove_wait(slot) for slot in range(len(s.blind))]
            for slot, g in enumerate(got):
                assert (g.a, g.b, g.c) == s.exp[slot], (tag, form, "slot %d" % slot)
    finally:
        pr.close()


def run_pinocchio(s, tag, prover=None):
    """ZK and NonZK (the zeros of NonZK.prove), then three ZK proofs in flight; as uploaded, then with the h pool derived"""
    pr = prover or PIN.ZK(s.cs, s.pk)
    try:
        for form in ("tau powers", "derived"):
            if form == "derived":
                pr.derive_lagrange()
            assert pr.prove_with(s.w, *s.blind[0]).to_bytes() == s.exp[0], (tag, form, "ZK")
            assert PIN.NonZK.prove(pr, None, s.w).to_bytes() == s.exp[3], (tag, form, "NonZK")
            pr.set_witness(s.w)
            for slot, d in enumerate(s.blind[:3]):
                pr.prove_async(*d, slot)
            got = [pr.prove_wait(slot).to_bytes() for slot in range(3)]
            for slot, g in enumerate(got):
                assert g == s.exp[slot], (tag, form, "slot %d" % slot)
    finally:
        pr.close()


_setups = {}


def setups(size):
    """(Groth16, Pinocchio) keys and expected proofs, built once per module and size"""
    if size not in _setups:
        _setups[size] = (groth16_setup(SIZES[size][0]), pinocchio_setup(SIZES[size][1]))
    return _setups[size]


def physical(devs):
    """k distinct cards when the box has them, the one card listed k times otherwise (tests/test_gpu_multidevice.py)"""
    k = len(devs)
    return list(range(k)) if _lib.lib().zk_device_count() >= k else list(devs)


@contextmanager
def device_list(devs):
    _lib.check(_lib.lib().zk_init(0))
    if devs:
        _lib.set_device_list(physical(devs))
    try:
        yield
    finally:
        if devs:
            _lib.set_device_list([0])


def _live_params(multi_only=False):
    return [pytest.param(c, settings, id=rid) for rid, c, settings in live_runs() if c.multi or not multi_only]


@pytest.mark.parametrize("c,settings", _live_params())
def test_a_live_option_leaves_every_proof_as_the_oracle_has_it(c, settings):
    g16, pin = setups(c.size)
    _lib.check(_lib.lib().zk_init(0))
    with options(settings):
        run_groth16(g16, settings)
        run_pinocchio(pin, settings)


@pytest.mark.parametrize("devs", DEVICE_LISTS, ids=["x2", "x3"])
@pytest.mark.parametrize("c,settings", _live_params(multi_only=True))
def test_a_key_option_on_a_device_list(c, settings, devs):
    g16, pin = setups(c.size)
    with device_list(devs), options(settings):
        run_groth16(g16, (settings, devs))
        run_pinocchio(pin, (settings, devs))


def test_resident_key_machinery_through_the_msm_entry_points():
    """ZK_MSM_API_PRECOMP=1 (msm.hip: msm_api): zk_msm_g1 / zk_msm_g2 through window tables, one bucket set and folded digits, over base sets with
    duplicates, negations and the identity, against the oracle's naive fold (curve.ml:94-118)"""
    from zukelang_amd.curve import G1, G2
    assert CASES["ZK_MSM_API_PRECOMP"].values == ("1",)
    st = P.fr_stream(0x5EED0900)
    for G, naive, gen, mul in ((G1, O.g1_msm_naive, O.g1_generator, O.g1_mul), (G2, O.g2_msm_naive, O.g2_generator, O.g2_mul)):
        inf = bytes([0x40]) + bytes(G.POINT_BYTES - 1)
        uniq = [mul(gen(), P.fr_to_bytes(next(st))) for _ in range(3)]
        uniq.append(mul(uniq[0], P.fr_to_bytes(P.R - 1)))                 # a negation of another base
        for n in (1, 7, 300, 2000):
            pts = [inf if i % 11 == 3 else uniq[i % 4] if i % 3 else mul(gen(), P.fr_to_bytes(next(st) % (1 << 64) + i)) for i in range(n)]
            scs = [0 if i % 13 == 5 else 1 if i % 13 == 6 else P.R - 1 if i % 13 == 7 else next(st) for i in range(n)]
            bases, scalars = b"".join(pts), frs(scs)
            rc, ref = naive(bases, scalars)
            assert rc == 0
            for c in (0, 3, 5, 9, 16):
                with options({"ZK_MSM_API_PRECOMP": "1"}):
                    got = bytes(G.apply_powers(scalars, np.frombuffer(bases, dtype=np.uint8), c))
                assert got == ref, (G.__name__, n, c)


# ---- cached knobs: one fresh process per group (tests/option_cases.py: CACHED_GROUPS); the child runs without ZK_TEST_FORMS, so the kernel forms are
# the shipped ones too
def child_main(group):
    _lib.check(_lib.lib().zk_init(0))          # options before the first key: they are cached at first use
    for k, v in CACHED_GROUPS[group].items():
        set_option(k, v)
    g16, pin = setups("small")
    run_groth16(g16, CACHED_GROUPS[group])
    run_pinocchio(pin, CACHED_GROUPS[group])
    print("CACHED-OPTIONS-OK %d" % group)


@pytest.mark.parametrize("group", range(len(CACHED_GROUPS)))
def test_cached_options_in_a_fresh_process(group):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_options as T; T.child_main(%d)" % (root, here, group)
    keep = ("ZK_LIBZKMI355X_PATH", "ZK_ORACLE_SO")                  # which build of the library / oracle, not knobs
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZK_") or k in keep}
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert res.returncode == 0 and "CACHED-OPTIONS-OK %d" % group in res.stdout, (CACHED_GROUPS[group], res.stdout[-2000:] + res.stderr[-4000:])


# ---- named interactions
@pytest.mark.parametrize("devs", [None, [0, 0]], ids=["one", "x2"])
@pytest.mark.parametrize("shared", [None, "0"], ids=["shared-sorts", "own-sorts"])
@pytest.mark.parametrize("rounds", [{"ZK_MSM_BA_ROUNDS": "2"}, {"ZK_MSM_BA_CURVES": "3"}], ids=["rounds2", "curves3"])
def test_batch_affine_rounds_on_a_pinocchio_key(rounds, shared, devs):
    """Generated keys share one sort per scalar vector (vv / vav, yy / yay, ww / waw); msm_accumulate_sorted refuses a shared sort when either workspace
    runs batch-affine rounds.  The prover must fall back to a sort of its own for the pair, at enqueue: the rounds are chosen with the slot's workspaces."""
    _g16, pin = setups("ba")
    with device_list(devs), options(dict(rounds, ZK_PIN_SHARED_SORT=shared)):
        run_pinocchio(pin, (rounds, shared, devs))


def test_batch_affine_rounds_with_a_forced_two_level_sort():
    g16, pin = setups("small")
    with options({"ZK_MSM_BA_ROUNDS": "2", "ZK_MSM_WINDOW": "16", "ZK_SORT_TWO_LEVEL_MIN": "10"}):
        run_groth16(g16, "ba + two levels")
        run_pinocchio(pin, "ba + two levels")
    with options({"ZK_MSM_BA_ROUNDS": "3", "ZK_MSM_WINDOW": "17", "ZK_SORT_TWO_LEVEL_MIN": "10"}):          # folded, 2^16 buckets
        run_groth16(g16, "ba + two levels, 17")
        run_pinocchio(pin, "ba + two levels, 17")


@pytest.mark.parametrize("devs,maker", [([0, 0, 0], lambda: RC.random_r1cs(1, 6, 76, nnz=(1, 2))), ([0, 0, 0, 0], lambda: RC.iterated_cubic(2, 4))],
                         ids=["n1-x3", "n2-x4"])
def test_the_upload_decides_whether_the_derived_h_pool_folds(devs, maker):
    """Folded windows ((r - s)(-P) = sP) hold only for points of order r, so a key uploaded with ZK_KEY_SUBGROUP_CHECK=0 must never get them -- the derived
    h pool included, even when the knob is handed back before zk_pinocchio_pk_derive_lagrange.  The compact h pool (n + 1 points) becomes n + 2 when
    derived, so a device list longer than the old pool has a shard whose old slice was empty (n = 1 on three entries: the first shard then derives
    [Z(s)]).  The key holds a point outside the subgroup at si[n]: v_k, w_k have degree < n, so the compact check does not read it, and [Z(s)] does."""
    from test_gpu_api_errors import _point_outside_the_subgroup
    s = pinocchio_setup(0, maker)
    n = s.cs.n
    nm = int(np.count_nonzero(s.cs.mid))
    at = 5 * nm + n                                                      # si[n] in the flattened G1 key
    g1 = np.array(s.pk.g1, dtype=np.uint8, copy=True)
    g1[96 * at:96 * at + 96] = np.frombuffer(P.g1_to_bytes(_point_outside_the_subgroup()), dtype=np.uint8)
    key = PIN.PKey(g1, s.pk.g2)

    def run(hand_back):
        out = []
        with device_list(devs), options({"ZK_MSM_WINDOW": "5", "ZK_KEY_SUBGROUP_CHECK": "0"}):
            pr = PIN.ZK(s.cs, key)
            try:
                assert pr.pool_size(5) == n + 1, "the compact h pool"
                out.append([pr.prove_with(s.w, *d).to_bytes() for d in s.blind])
                if hand_back:
                    set_option("ZK_KEY_SUBGROUP_CHECK", None)
                pr.derive_lagrange()
                out.append(bytes(pr.pool_points(5)))
                out.append([pr.prove_with(s.w, *d).to_bytes() for d in s.blind])
                pr.set_witness(s.w)
                for slot, d in enumerate(s.blind):
                    pr.prove_async(*d, slot)
                out.append([pr.prove_wait(slot).to_bytes() for slot in range(len(s.blind))])
            finally:
                pr.close()
        return out

    off = run(False)
    assert off[0][3] == s.exp[3], "NonZK does not read si[n]"
    handed_back = run(True)
    assert handed_back[1] == off[1], "derived h pool"
    assert handed_back[2] == off[2], "derived key, one proof at a time"
    assert handed_back[3] == off[3], "derived key, pipelined"
