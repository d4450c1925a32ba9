"""Handles that live together, against the oracles: what every handle of a device SHARES (csrc/zk_common.h Ctx / CtxBufs, the per-device globals) while
keys of different sizes, both protocols, resident bases and a resident verification key are alive at once -- and while the shared tables GROW.

The twiddle heaps of a context (ntt.hip: Fr, floor 2^12; rns_ntt.hip: the residue system's, floor 2^14, ZK_FR_RNS=1) are replaced by larger ones when a
call needs more levels.  Under ZK_GRAPH=1 a slot's proof is captured once with the heap pointers of that moment and replayed; a proof of another key may
be in flight on its own streams.  csrc/ctx_tables.h keeps the old heaps until zk_shutdown (tests/test_ctx_tables.py holds that policy on the CPU); here the
replays run.  A table only ever grows within a process, so each scenario is a fresh child process in which key A (300 constraints, S = 2^10) comes first:
the tables start at their floors.

Key A is RC.iterated_cubic(300, x): the circuit does not depend on x, the witness does, so every check proves a NEW witness with new r, s.  Key B has
8193 constraints (log S = 15), the Pinocchio key 16385 (log S = 16): iterated_cubic makes even counts only, so both are RC.random_r1cs(n, 64, ...) with
one or two entries per row -- few variables, and a key whose size follows n.

What grows when (log2 of the levels held; "Fr" = ntt.hip, "RNS" = rns_ntt.hip):
  child "graphs"        A: Fr 12            1. zk_fr_ntt 2^13: Fr 13     2. zk_fr_poly_mul 5000 x 5000 (2^14): Fr 14     3. key B: Fr 15     4. Pinocchio: Fr 16
  child "graphs-rns"    A: Fr 12, RNS 14    1. Fr 13                     2. nothing (the product runs in the residue system at its floor, 2^14)
                                            3. key B: Fr 15 (two levels), RNS 15                                         4. Pinocchio: Fr 16, RNS 16
  child "streams"       no graphs: three proofs of A in flight while key B is uploaded (Fr 15), zk_fr_ntt runs at 2^13, the Pinocchio key is uploaded
                        (Fr 16) and B's key is checked.  include/zkmi355x.h forbids none of these calls while ANOTHER handle has proofs in flight (its
                        restrictions name the handle's own slots: key_check, derive, set_witness, prove_many), so none is expected to refuse.
After every step every graph of A is replayed: three slots; witness from the host, one proof at a time (slot 0 alone forks onto its three streams: the
non-serial graph); resident witness, three in flight, enqueued 0, 1, 2 and 2, 1, 0 (slot 0 then runs serial: its other graph).

A device-list handle never reaches the graph branch: group_prove_async (csrc/groth16_multi.hip:148-165) calls groth16_scalars_enqueue and
groth16_msms_enqueue itself, prove_enqueue (groth16.hip, the only place that captures) is static and serves single-device handles only, and the shard
entry points refuse a multi-device handle (key_lookup).  So there is no fourth child.

In process, without children: four Groth16 keys (1, 13, 300 and 1025 constraints; the 13 in Lagrange form), a Pinocchio key, resident G1 and G2 bases and
a resident verification key, fifteen proofs in flight at a time over three rounds, one round under ZK_GRAPH=1, a key freed and uploaded again between
rounds.  A handle number is never handed out twice (csrc/handle_table.h): the key comes back under a NEW number and the old one stays unknown.

Child wall times measured on one MI355X are in CHILD_SECONDS (2.4 s, 2.3 s, 1.3 s; the cached-options children of tests/test_gpu_options.py were last
recorded at 13 s); each timeout is three times that plus ten seconds for a cold start.  Every child runs with ZK_TRACE=1 and the parent reads the
library's own account of each growth (CHILD_GROWTH): the scenario shows that it moved the tables it is about."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle_lib as O
from oracle import pyref as P
from zukelang_amd import _lib, r1cs as RC
from zukelang_amd import pinocchio as PIN
from zukelang_amd.curve import FFT_Fr, G1, G2
from zukelang_amd.groth16 import Groth16, Proof

pytestmark = pytest.mark.gpu

ZK_ERR_HANDLE = -7
N_A, N_B, N_PIN = 300, 8193, 16385
CHILD_SECONDS = {"graphs": 2.4, "graphs-rns": 2.3, "streams": 1.3}          # wall time of each child as measured on one MI355X, start-up included
START_UP_SECONDS = 10                                                     # allowance for a cold start (interpreter, code objects, device) on a busy box


def child_timeout(name):
    return 3 * CHILD_SECONDS[name] + START_UP_SECONDS



CHILD_ENV = {"graphs": {"ZK_GRAPH": "1"}, "graphs-rns": {"ZK_GRAPH": "1", "ZK_FR_RNS": "1"}, "streams": {}}
# What each child must have moved, from the library's own account (ZK_TRACE=1, csrc/ctx_tables.h: one line per growth): (from, to) as log2 of the levels
# held, 0 = no table yet.  A scenario that no longer moves a table -- a raised floor, a key that got smaller -- fails here instead of passing idly.
FR, RNS = "Fr twiddle heaps", "residue-system twiddle heap"
CHILD_GROWTH = {
    "graphs": {FR: [(0, 12), (12, 13), (13, 14), (14, 15), (15, 16)], RNS: []},
    "graphs-rns": {FR: [(0, 12), (12, 13), (13, 15), (15, 16)], RNS: [(0, 14), (14, 15), (15, 16)]},
    "streams": {FR: [(0, 12), (12, 15), (15, 16)], RNS: []},
}


def frs(xs):
    return b"".join(P.fr_to_bytes(x) for x in xs)


def _csrs(cs):
    return [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]


class G16:
    """a Groth16 key with its toxic waste: proofs of any witness against the trapdoor oracle"""

    def __init__(self, cs, seed, lagrange=False):
        self.cs, self.csr, self.lagrange = cs, _csrs(cs), lagrange
        self.st = P.fr_stream(seed)
        self.toxic = [next(self.st) for _ in range(5)]
        it = iter(self.toxic)
        self.pk, self.vk = Groth16.keygen(lambda: next(it), cs, lagrange=lagrange)
        self.pr = None

    def upload(self):
        self.pr = Groth16(self.cs, self.pk, lagrange=self.lagrange)
        return self

    def blind(self):
        return next(self.st), next(self.st)

    def expect(self, w, r, s):
        return O.groth16_prove_trapdoor(self.cs.n, self.cs.m, *self.csr, self.cs.mid, frs(w), frs(self.toxic), P.fr_to_bytes(r), P.fr_to_bytes(s))

    def io(self, w):
        return [w[k] for k in range(self.cs.m) if not self.cs.mid[k]]

    def close(self):
        if self.pr is not None:
            self.pr.close()
            self.pr = None


class Pin:
    def __init__(self, cs, w, seed):
        self.cs, self.w, self.csr = cs, w, _csrs(cs)
        self.st = P.fr_stream(seed)
        self.toxic = [next(self.st) for _ in range(8)]
        it = iter(self.toxic)
        self.pk, _ = PIN.ZK.keygen(lambda: next(it), cs)
        self.pr = None

    def upload(self):
        self.pr = PIN.ZK(self.cs, self.pk)
        return self

    def blind(self):
        return [next(self.st) for _ in range(3)]

    def expect(self, d):
        return O.pinocchio_prove_trapdoor(self.cs.n, self.cs.m, *self.csr, self.cs.mid, frs(self.w), frs(self.toxic), *(P.fr_to_bytes(x) for x in d))

    def close(self):
        if self.pr is not None:
            self.pr.close()
            self.pr = None


def same(got, exp):
    return (bytes(got.a), bytes(got.b), bytes(got.c)) == exp


# ---- key A and its graphs
class KeyA(G16):
    def __init__(self):
        cs, _ = RC.iterated_cubic(N_A, 1)
        G16.__init__(self, cs, 0x5EED0C00)
        self.xs = P.fr_stream(0x5EED0C01)
        self.upload()
        self.pr.reserve_slots(3)

    def witness(self):
        cs, w = RC.iterated_cubic(N_A, next(self.xs))
        return w

    def check(self, step):
        """every proof shape on every slot, each with a witness and r, s nobody has proved before"""
        for slot in range(3):                                      # witness from the host, one proof at a time
            w, (r, s) = self.witness(), self.blind()
            self.pr.prove_async(w, r, s, slot)
            assert same(self.pr.prove_wait(slot), self.expect(w, r, s)), (step, "key A, witness from the host", "slot %d" % slot)
        for order in ((0, 1, 2), (2, 1, 0)):                       # resident witness, three in flight
            w = self.witness()
            self.pr.set_witness(w)
            rs = {slot: self.blind() for slot in order}
            for slot in order:
                self.pr.prove_async(None, *rs[slot], slot)
            got = {slot: self.pr.prove_wait(slot) for slot in order}
            for slot in order:
                assert same(got[slot], self.expect(w, *rs[slot])), (step, "key A, resident witness, enqueued %s" % (order,), "slot %d" % slot)


def key_b():
    cs, w = RC.random_r1cs(N_B, 64, 0xB0B, nnz=(1, 2))
    k = G16(cs, 0x5EED0C10)
    k.w = w
    return k


def pinocchio_key():
    cs, w = RC.random_r1cs(N_PIN, 64, 0xB1B, nnz=(1, 2))
    return Pin(cs, w, 0x5EED0C20)


def check_b(b, step):
    r, s = b.blind()
    assert same(b.pr.prove_rs(b.w, r, s), b.expect(b.w, r, s)), (step, "key B")


def check_both_in_flight(a, b, step):
    """proofs of A and of B in flight at once, enqueued alternately: A0 B0 A1 B1 A2 B2"""
    wa = a.witness()
    a.pr.set_witness(wa)
    b.pr.set_witness(b.w)
    ra, rb = [a.blind() for _ in range(3)], [b.blind() for _ in range(3)]
    for slot in range(3):
        a.pr.prove_async(None, *ra[slot], slot)
        b.pr.prove_async(None, *rb[slot], slot)
    for slot in range(3):
        assert same(b.pr.prove_wait(slot), b.expect(b.w, *rb[slot])), (step, "key B beside A", "slot %d" % slot)
        assert same(a.pr.prove_wait(slot), a.expect(wa, *ra[slot])), (step, "key A beside B", "slot %d" % slot)


def step_ntt():
    data = bytes(RC.random_fr_bytes(1 << 13, 0x13))
    assert bytes(FFT_Fr.fft(data, 13)) == O.fr_ntt(data, 13, False), "zk_fr_ntt at 2^13"
    assert bytes(FFT_Fr.ifft(data)) == O.fr_ntt(data, 13, True), "zk_fr_ntt at 2^13, inverse"


def step_poly_mul():
    a, b = bytes(RC.random_fr_bytes(5000, 0x14)), bytes(RC.random_fr_bytes(5000, 0x15))
    assert bytes(FFT_Fr.polynomial_mul(a, b)) == O.poly_mul(a, b), "zk_fr_poly_mul 5000 x 5000"


def child_graphs():
    """ZK_GRAPH=1 (and ZK_FR_RNS=1 in the second child) come with the environment: they are cached at first use"""
    a = KeyA()
    a.check("captured")                    # every graph of A is captured here, with the tables at their floors
    a.check("first replay")
    step_ntt()
    a.check("after zk_fr_ntt at 2^13")
    step_poly_mul()
    a.check("after zk_fr_poly_mul at 2^14")
    b = key_b().upload()
    check_b(b, "key B's first proof")
    a.check("after the upload of key B")
    for turn in range(2):
        check_b(b, "alternating %d" % turn)
        a.check("alternating %d" % turn)
    check_both_in_flight(a, b, "A and B in flight")
    pin = pinocchio_key().upload()
    d = pin.blind()
    assert pin.pr.prove_with(pin.w, *d).to_bytes() == pin.expect(d), "the Pinocchio key's first proof"
    a.check("after the upload of the Pinocchio key")
    check_b(b, "after the upload of the Pinocchio key")
    check_both_in_flight(a, b, "A and B in flight, after the Pinocchio key")
    for k in (pin, b, a):
        k.close()


def child_streams():
    """no graphs: the holders are kernels queued on A's slot streams"""
    a = KeyA()
    a.check("before")
    b, pin = key_b(), pinocchio_key()          # their points come from the device: made before anything is in flight
    w = a.witness()
    a.pr.set_witness(w)
    rs = [a.blind() for _ in range(3)]
    for slot in range(3):
        a.pr.prove_async(None, *rs[slot], slot)
    b.upload()                                 # Fr heaps 2^12 -> 2^15 while the three proofs are in flight
    step_ntt()
    pin.upload()                               # -> 2^16
    verdict = b.pr.check_key(b.vk, seed=bytes(range(32)))
    for slot in range(3):
        assert same(a.pr.prove_wait(slot), a.expect(w, *rs[slot])), ("in flight across two growths", "slot %d" % slot)
    assert verdict.ok, verdict
    check_b(b, "key B")
    d = pin.blind()
    assert pin.pr.prove_with(pin.w, *d).to_bytes() == pin.expect(d), "the Pinocchio key"
    a.check("after")
    for k in (pin, b, a):
        k.close()


CHILDREN = {"graphs": child_graphs, "graphs-rns": child_graphs, "streams": child_streams}


def child_main(name):
    t0 = time.time()
    for k, v in CHILD_ENV[name].items():
        assert os.environ.get(k) == v, "the child's environment carries its options"
    assert "ZK_TEST_FORMS" not in os.environ          # the shipped, cached reading of every knob
    _lib.check(_lib.lib().zk_init(0))
    CHILDREN[name]()
    _lib.check(_lib.lib().zk_shutdown())               # the cleanup hooks: every heap, live and retired
    print("LIVE-TOGETHER-OK %s %.1f s" % (name, time.time() - t0))


@pytest.mark.parametrize("name", list(CHILDREN))
def test_replays_and_proofs_in_flight_survive_the_growth_of_the_shared_tables(name):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_live_together as T; T.child_main(%r)" % (root, here, name)
    keep = ("ZK_LIBZKMI355X_PATH", "ZK_ORACLE_SO")                  # which build of the library / oracle, not knobs
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZK_") or k in keep}
    env.update(CHILD_ENV[name], ZK_TRACE="1")
    t0 = time.time()
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=child_timeout(name), env=env, cwd=root)
    print("child %s: %.1f s" % (name, time.time() - t0))
    assert res.returncode == 0 and "LIVE-TOGETHER-OK %s" % name in res.stdout, (name, res.returncode, res.stdout[-2000:] + res.stderr[-4000:])
    moved = {FR: [], RNS: []}
    for what, a, b, retired in re.findall(r"^\[zk tables\] (.+): 2\^(\d+) -> 2\^(\d+), (\d+) retired$", res.stderr, flags=re.M):
        assert int(retired) == len(moved[what]), (name, what, "every earlier heap is kept, none freed")
        moved[what].append((int(a), int(b)))
    assert moved == CHILD_GROWTH[name], (name, "the tables did not move as the scenario means them to", moved)


# ---- different sizes alive together, in process
def test_keys_of_four_sizes_two_protocols_bases_and_a_verification_key_alive_at_once():
    L = _lib.lib()
    _lib.check(L.zk_init(0))
    keys = {
        1: G16(RC.random_r1cs(1, 6, 76, nnz=(1, 2))[0], 0x5EED0D01),
        13: G16(RC.random_r1cs(13, 20, 77, nnz=(1, 3))[0], 0x5EED0D02, lagrange=True),
        300: G16(RC.iterated_cubic(300, 1)[0], 0x5EED0D03),
        1025: G16(RC.random_r1cs(1025, 64, 78, nnz=(1, 2))[0], 0x5EED0D04),
    }
    wit = {1: RC.random_r1cs(1, 6, 76, nnz=(1, 2))[1], 13: RC.random_r1cs(13, 20, 77, nnz=(1, 3))[1], 1025: RC.random_r1cs(1025, 64, 78, nnz=(1, 2))[1]}
    xs = P.fr_stream(0x5EED0D05)
    pcs, pw = RC.iterated_cubic(300, 0xD06)
    pin = Pin(pcs, pw, 0x5EED0D07)
    pts1 = np.array(G1.of_Fr(RC.random_fr_bytes(50, 0xD08)), dtype=np.uint8).reshape(-1)
    pts2 = np.array(G2.of_Fr(RC.random_fr_bytes(20, 0xD09)), dtype=np.uint8).reshape(-1)
    opened = []
    try:
        for k in keys.values():
            opened.append(k.upload())
            k.pr.reserve_slots(3)
        opened.append(pin.upload())
        pin.pr.reserve_slots(3)
        pin.pr.set_witness(pin.w)
        b1, b2 = G1.resident(pts1), G2.resident(pts2)
        vk = keys[300].vk.resident()
        opened += [b1, b2, vk]
        for rnd in range(3):
            _lib.check(L.zk_set_option(b"ZK_GRAPH", b"1" if rnd == 1 else None))          # read per proof under ZK_TEST_FORMS=1 (tests/conftest.py)
            ws = {n: (RC.iterated_cubic(300, next(xs))[1] if n == 300 else wit[n]) for n in keys}
            for n, k in keys.items():
                k.pr.set_witness(ws[n])
            rs = {(n, slot): keys[n].blind() for slot in range(3) for n in keys}
            ds = {slot: pin.blind() for slot in range(3)}
            for slot in range(3):                                  # round-robin over the handles: fifteen proofs in flight
                for n in keys:
                    keys[n].pr.prove_async(None, *rs[n, slot], slot)
                pin.pr.prove_async(*ds[slot], slot)
            # resident products and verdicts while the proofs are in flight
            sc1, sc2 = bytes(RC.random_fr_bytes(50, 0xD10 + rnd)), bytes(RC.random_fr_bytes(20, 0xD20 + rnd))
            assert bytes(b1.apply_powers(sc1)) == O.g1_msm_naive(bytes(pts1), sc1)[1], ("round %d" % rnd, "resident G1 bases")
            assert bytes(b2.apply_powers(sc2)) == O.g2_msm_naive(bytes(pts2), sc2)[1], ("round %d" % rnd, "resident G2 bases")
            proofs = {}
            for slot in range(3):
                for n in keys:
                    proofs[n, slot] = keys[n].pr.prove_wait(slot)
                    assert same(proofs[n, slot], keys[n].expect(ws[n], *rs[n, slot])), ("round %d" % rnd, "Groth16 key n = %d" % n, "slot %d" % slot)
                assert pin.pr.prove_wait(slot).to_bytes() == pin.expect(ds[slot]), ("round %d" % rnd, "Pinocchio key", "slot %d" % slot)
            good = [proofs[300, slot] for slot in range(3)]
            bad = Proof(good[0].a, good[1].b, good[2].c)          # three honest points that are no proof
            batch, io = good + [bad], keys[300].io(ws[300])
            host = [Groth16.verify(io, keys[300].vk, p) for p in batch]
            assert host == [True, True, True, False], ("round %d" % rnd, "host verifier")
            assert vk.verify_many([io] * 4, batch) == host, ("round %d" % rnd, "resident verification key")
            # one key leaves and comes back: a new handle number, the old one unknown, the others untouched
            n = (13, 1025, 300)[rnd]
            old = keys[n].pr.handle.value
            keys[n].close()
            keys[n].upload()
            keys[n].pr.reserve_slots(3)
            assert keys[n].pr.handle.value != old and L.zk_groth16_reserve_slots(C.c_uint64(old), C.c_uint32(1)) == ZK_ERR_HANDLE, ("round %d" % rnd, n)
    finally:
        L.zk_set_option(b"ZK_GRAPH", None)
        for obj in opened:
            try:
                obj.close()
            except Exception:
                pass
