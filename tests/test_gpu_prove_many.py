"""zk_groth16_prove_many_compressed / zk_pinocchio_prove_many_compressed (include/zkmi355x.h; csrc/prove_many.cuh, k_proofs_to_wire of csrc/msm_points.hip):
a batch of witnesses proved in one call, the proofs out as the wire bytes of the reference's proof record (groth16.ml:110-114, pinocchio.ml:195-208).
What is expected comes from the oracle alone: the trapdoor oracle's proof (tests/oracle_lib.py) through the oracle's compressor; the same bytes are then
also asked of zk_*_prove + zk_g1/g2_compress on the same handle.  The circuits are the README circuit (40 witnesses x = 2 .. 41) and random R1CS with
n = 16 and n = 64; every case is a few dozen proofs of a few constraints."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from oracle import pyref as P
from zukelang_amd import _lib, r1cs as RC
from zukelang_amd import pinocchio as PIN
from zukelang_amd.groth16 import Groth16, PKey

pytestmark = pytest.mark.gpu

R, Pm = P.R, P.P
ZK_OK, ZK_ERR_ARG, ZK_ERR_SCALAR_RANGE, ZK_ERR_REMAINDER = 0, -1, -3, -4
G16_WIRE = ((0, 1), (48, 2), (144, 1))                                                                  # A B C: (offset in the record, group)
PIN_WIRE = ((0, 1), (48, 2), (144, 1), (192, 1), (240, 1), (288, 2), (384, 1), (432, 1))          # vv ww yy h vavv waww yayy bvwy
INF = {1: bytes([0xC0]) + bytes(47), 2: bytes([0xC0]) + bytes(95)}
COUNTS, IN_FLIGHT = (1, 3, 17, 40), (1, 2, 15, 0)


def frs(xs):
    return b"".join(P.fr_to_bytes(x) for x in xs)


def csrs(cs):
    return [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]


def compress(proof, wire):
    """an uncompressed oracle proof -> its wire record, through the oracle's compressor"""
    out, off = [], 0
    for _, g in wire:
        out.append(O.g1_compress(proof[off:off + 96]) if g == 1 else O.g2_compress(proof[off:off + 192]))
        off += 96 * g
    return b"".join(out)


def both_signs_everywhere(proofs, wire):
    """every point position of the record carries the flags 0x80 and 0xA0 somewhere in the list"""
    return all({p[off] & 0xE0 for p in proofs} >= {0x80, 0xA0} for off, _ in wire)


def _p8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def many(fn, handle, sols, rnd, count, in_flight, size):
    """the raw call on buffers full of 0x55 / 77: (rc, the proofs' bytes, the statuses)"""
    out, st = np.full(size * count, 0x55, dtype=np.uint8), np.full(count, 77, dtype=np.int32)
    s = np.frombuffer(bytes(sols), dtype=np.uint8) if sols is not None else None
    r = np.frombuffer(bytes(rnd), dtype=np.uint8)
    rc = getattr(_lib.lib(), fn)(handle, _p8(s) if s is not None else None, _p8(r), count, in_flight, _p8(out), st.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, [bytes(out[size * i:size * i + size]) for i in range(count)], [int(x) for x in st]


G16, PINO = "zk_groth16_prove_many_compressed", "zk_pinocchio_prove_many_compressed"


@pytest.fixture(autouse=True)
def _init_and_leave_nothing_behind():
    _lib.check(_lib.lib().zk_init(0))
    yield
    _lib.set_device_list([0])          # ZK_ERR_ARG while any key handle is alive


class Case:
    """One circuit with its keys for both protocols (trapdoors known to the oracle), witnesses, randomness and the oracle's wire bytes: computed once."""

    def __init__(self, cs, witnesses, seed):
        self.cs, self.wits = cs, witnesses
        st = P.fr_stream(seed)
        self.tox_g = [next(st) for _ in range(5)]
        self.tox_p = [next(st) for _ in range(8)]
        it = iter(self.tox_g)
        self.pk_g, self.vk_g = Groth16.keygen(lambda: next(it), cs, lagrange=True)
        it = iter(self.tox_p)
        self.pk_p, self.vk_p = PIN.ZK.keygen(lambda: next(it), cs)
        n = len(witnesses)
        self.rs = [(next(st), next(st)) for _ in range(n)]
        self.ds = [(next(st), next(st), next(st)) for _ in range(n)]
        L, Rr, Oo = csrs(cs)
        self.plain_g = [b"".join(O.groth16_prove_trapdoor(cs.n, cs.m, L, Rr, Oo, cs.mid, frs(w), frs(self.tox_g), P.fr_to_bytes(r), P.fr_to_bytes(s)))
                        for w, (r, s) in zip(witnesses, self.rs)]
        pin = lambda w, d: O.pinocchio_prove_trapdoor(cs.n, cs.m, L, Rr, Oo, cs.mid, frs(w), frs(self.tox_p), *(P.fr_to_bytes(x) for x in d))
        self.plain_zk = [pin(w, d) for w, d in zip(witnesses, self.ds)]
        self.plain_nz = [pin(w, (0, 0, 0)) for w in witnesses]
        self.exp_g = [compress(p, G16_WIRE) for p in self.plain_g]
        self.exp_zk = [compress(p, PIN_WIRE) for p in self.plain_zk]
        self.exp_nz = [compress(p, PIN_WIRE) for p in self.plain_nz]
        self.ios = [[w[k] for k in range(cs.m) if not cs.mid[k]] for w in witnesses]

    def sols(self, idx):
        return b"".join(frs(self.wits[i]) for i in idx)

    def rnd_g(self, idx):
        return frs([x for i in idx for x in self.rs[i]])

    def rnd_p(self, idx, zero=False):
        return frs([x for i in idx for x in ((0, 0, 0) if zero else self.ds[i])])


@pytest.fixture(scope="module")
def readme():
    wit = [RC.readme_circuit(x) for x in range(2, 42)]
    c = Case(wit[0][0], [w for _, w in wit], 0x5EED9A01)
    # the 40 pairs were chosen so that this holds: it is asserted on the ORACLE's bytes, before any of them is compared with the GPU's
    assert both_signs_everywhere(c.exp_g, G16_WIRE) and both_signs_everywhere(c.exp_zk, PIN_WIRE) and both_signs_everywhere(c.exp_nz, PIN_WIRE)
    return c


@pytest.fixture(scope="module", params=[16, 64])
def random_case(request):
    n = request.param
    cs, w = RC.random_r1cs(n, n + 9, 0xA11CE + n)
    return Case(cs, [w] * 5, 0x5EED9B00 + n)


def run_all_shapes(fn, handle, size, c, exp, rnd_of):
    for count in COUNTS:
        for infl in IN_FLIGHT:
            idx = list(range(count))
            rc, got, st = many(fn, handle, c.sols(idx), rnd_of(idx), count, infl, size)
            assert rc == 0 and st == [0] * count, (count, infl, st)
            assert got == exp[:count], (count, infl)


# ------------------------------------------------------------------------------------------------------------------ 1: every proof equals the expected bytes
@pytest.mark.parametrize("form", ["tau_powers", "derived"])
def test_groth16_batches_equal_the_oracles_wire_bytes(readme, form):
    c = readme
    p = Groth16(c.cs, c.pk_g)
    if form == "derived":
        p.derive_lagrange()
    run_all_shapes(G16, p.handle, 192, c, c.exp_g, c.rnd_g)
    # ... and zk_groth16_prove + zk_g1/g2_compress on the same handle, witness and randomness
    assert [p.prove_rs(w, r, s).to_compressed() for w, (r, s) in zip(c.wits, c.rs)] == c.exp_g
    # the Python surface: the pairs handed over, and drawn from a generator in proof order (r then s)
    assert p.prove_many(c.rs[:7], c.wits[:7], in_flight=3) == c.exp_g[:7]
    flat = iter([x for pair in c.rs[:7] for x in pair])
    assert p.prove_many(lambda: next(flat), c.wits[:7]) == c.exp_g[:7]
    # sols = NULL: the resident witness for every proof
    p.set_witness(c.wits[4])
    L, Rr, Oo = csrs(c.cs)
    want = [compress(b"".join(O.groth16_prove_trapdoor(c.cs.n, c.cs.m, L, Rr, Oo, c.cs.mid, frs(c.wits[4]), frs(c.tox_g), P.fr_to_bytes(r), P.fr_to_bytes(s))), G16_WIRE)
            for r, s in c.rs[:6]]
    rc, got, st = many(G16, p.handle, None, c.rnd_g(range(6)), 6, 4, 192)
    assert (rc, st) == (0, [0] * 6) and got == want and want[4] == c.exp_g[4]
    assert p.prove_many(c.rs[:6], 6, in_flight=2) == want
    # ZK_GRAPH=1: every slot replays its raw graph, the row copy stays outside it (capture, then replays with slots reused more than twice)
    old = os.environ.get("ZK_GRAPH")
    os.environ["ZK_GRAPH"] = "1"
    try:
        for sols, exp in ((c.sols(range(9)), c.exp_g[:9]), (None, want)):
            rc, got, st = many(G16, p.handle, sols, c.rnd_g(range(len(exp))), len(exp), 2, 192)
            assert (rc, st) == (0, [0] * len(exp)) and got == exp, sols is None
    finally:
        if old is None:
            os.environ.pop("ZK_GRAPH", None)
        else:
            os.environ["ZK_GRAPH"] = old
    p.close()


@pytest.mark.parametrize("zk", [True, False])
def test_pinocchio_batches_equal_the_oracles_wire_bytes(readme, zk):
    c = readme
    p = (PIN.ZK if zk else PIN.NonZK)(c.cs, c.pk_p)
    exp = c.exp_zk if zk else c.exp_nz
    run_all_shapes(PINO, p.handle, 480, c, exp, lambda idx: c.rnd_p(idx, zero=not zk))
    ds = c.ds if zk else [(0, 0, 0)] * len(c.wits)
    assert [p.prove_with(w, *d).to_compressed() for w, d in zip(c.wits[:8], ds)] == exp[:8]
    if zk:
        flat = iter([x for t in c.ds[:5] for x in t])
        assert p.prove_many(lambda: next(flat), c.wits[:5], in_flight=2) == exp[:5]
    else:
        assert p.prove_many(None, c.wits[:5], in_flight=2) == exp[:5]
    # sols = NULL: the resident witness; and the derived h bases give the same bytes
    p.set_witness(c.wits[3])
    p.derive_lagrange()
    rc, got, st = many(PINO, p.handle, None, c.rnd_p([3, 3], zero=not zk), 2, 0, 480)
    assert (rc, st) == (0, [0, 0]) and got == [exp[3], exp[3]]
    rc, got, st = many(PINO, p.handle, c.sols(range(9)), c.rnd_p(range(9), zero=not zk), 9, 4, 480)
    assert (rc, st) == (0, [0] * 9) and got == exp[:9]
    p.close()


def test_random_r1cs_in_every_key_form(random_case):
    """n = 16 and n = 64: keys as uploaded, uploaded in Lagrange form, derived, generated on the device and uploaded compressed -- the same bytes"""
    c = random_case
    idx = list(range(5))
    from zukelang_amd.curve import G1, G2
    it = iter(c.tox_g)
    generated = Groth16.generate(lambda: next(it), c.cs, form="lagrange")[0]
    provers = [Groth16(c.cs, c.pk_g), Groth16(c.cs, c.pk_g, lagrange=True), Groth16(c.cs, c.pk_g), generated,
               Groth16.from_compressed(c.cs, G1.to_compressed_bytes_many(bytes(c.pk_g.g1)), G2.to_compressed_bytes_many(bytes(c.pk_g.g2)))]
    provers[2].derive_lagrange()
    for k, p in enumerate(provers):
        rc, got, st = many(G16, p.handle, c.sols(idx), c.rnd_g(idx), 5, 2, 192)
        assert (rc, st) == (0, [0] * 5) and got == c.exp_g, k
        p.close()
    for cls, exp, zero in ((PIN.ZK, c.exp_zk, False), (PIN.NonZK, c.exp_nz, True)):
        p = cls(c.cs, c.pk_p)
        for stage in ("as uploaded", "derived"):
            if stage == "derived":
                p.derive_lagrange()
            rc, got, st = many(PINO, p.handle, c.sols(idx), c.rnd_p(idx, zero=zero), 5, 2, 480)
            assert (rc, st) == (0, [0] * 5) and got == exp, stage
        p.close()


# ------------------------------------------------------------------------------------------------------------------ 2: mixed batches
def spoiled(w):
    """a witness that breaks the last gate"""
    return list(w[:-1]) + [(w[-1] + 1) % R]


def mixed(c, count, infl):
    """(sols, the indices of the unsatisfied witnesses, the index of a witness value >= r): index 0, in_flight (the first reuse of slot 0), the middle, the last"""
    bad = sorted({0, infl, count // 2, count - 1})
    rng_at = count // 2 + 1
    assert rng_at not in bad
    sols = [frs(spoiled(c.wits[i])) if i in bad else frs(c.wits[i]) for i in range(count)]
    sols[rng_at] = sols[rng_at][:32] + (R + 1).to_bytes(32, "little") + sols[rng_at][64:]
    return sols, bad, rng_at


def test_groth16_mixed_batch(readme):
    c = readme
    count, infl, big_r = 12, 3, 9
    p = Groth16(c.cs, c.pk_g)
    sols, bad, rng_at = mixed(c, count, infl)
    rnd = [frs(c.rs[i]) for i in range(count)]
    rnd[big_r] = (R + 5).to_bytes(32, "little") + rnd[big_r][32:]                    # r >= the modulus
    # what the single call says about each of them, on the same handle
    single = []
    for i in range(count):
        out = np.zeros(384, dtype=np.uint8)
        s_, r_ = np.frombuffer(sols[i], dtype=np.uint8), np.frombuffer(rnd[i], dtype=np.uint8)
        rc = _lib.lib().zk_groth16_prove(p.handle, _p8(s_), _p8(r_), _p8(r_[32:]), _p8(out))
        single.append((rc, bytes(out)))
    assert [single[i][0] for i in sorted(bad + [rng_at])] == [ZK_ERR_REMAINDER if i in bad else ZK_ERR_SCALAR_RANGE for i in sorted(bad + [rng_at])]
    rc, got, st = many(G16, p.handle, b"".join(sols), b"".join(rnd), count, infl, 192)
    assert rc == 0
    assert st == [s[0] for s in single]
    for i in range(count):
        if i in bad or i == rng_at:
            assert st[i] == (ZK_ERR_REMAINDER if i in bad else ZK_ERR_SCALAR_RANGE) and got[i] == bytes(192), i
        elif i == big_r:          # the status and the bytes of the single call, whatever it makes of such an r
            assert got[i] == (compress(single[i][1], G16_WIRE) if single[i][0] == 0 else bytes(192)), i
        else:
            assert st[i] == 0 and got[i] == c.exp_g[i], i
    # the Python surface: statuses on request, the reference's exception otherwise
    pr, codes = p.prove_many(c.rs[:4], [spoiled(c.wits[0])] + c.wits[1:4], in_flight=2, return_status=True)
    assert codes == [ZK_ERR_REMAINDER, 0, 0, 0] and pr == [bytes(192)] + c.exp_g[1:4]
    with pytest.raises(AssertionError, match="Polynomial.is_zero rem"):
        p.prove_many(c.rs[:4], c.wits[:3] + [spoiled(c.wits[3])])
    p.close()


def test_pinocchio_mixed_batch(readme):
    c = readme
    count, infl = 11, 2
    p = PIN.ZK(c.cs, c.pk_p)
    sols, bad, rng_at = mixed(c, count, infl)
    rc, got, st = many(PINO, p.handle, b"".join(sols), c.rnd_p(range(count)), count, infl, 480)
    assert rc == 0
    for i in range(count):
        want = ZK_ERR_REMAINDER if i in bad else ZK_ERR_SCALAR_RANGE if i == rng_at else 0
        assert st[i] == want and got[i] == (bytes(480) if want else c.exp_zk[i]), i
    with pytest.raises(AssertionError, match="Polynomial.is_zero rem"):
        p.prove_many(c.ds[:2], [c.wits[0], spoiled(c.wits[1])])
    p.close()


# ------------------------------------------------------------------------------------------------------------------ 3: busy slot; the handle afterwards
def test_a_busy_slot_refuses_the_batch_and_keeps_its_proof(readme):
    c = readme
    p = Groth16(c.cs, c.pk_g)
    before = p.prove_rs(c.wits[0], *c.rs[0])
    pools = [bytes(p.pool_points(g)) for g in (1, 2)]
    for slot in (0, 5):
        p.prove_async(c.wits[1], *c.rs[1], slot)
        rc, got, st = many(G16, p.handle, c.sols(range(3)), c.rnd_g(range(3)), 3, 2, 192)
        assert rc == ZK_ERR_ARG and st == [77] * 3 and got == [bytes([0x55]) * 192] * 3          # refused, nothing written
        pr = p.prove_wait(slot)
        assert pr.a + pr.b + pr.c == c.plain_g[1]
    rc, got, st = many(G16, p.handle, c.sols(range(20)), c.rnd_g(range(20)), 20, 15, 192)
    assert (rc, st) == (0, [0] * 20) and got == c.exp_g[:20]
    # every slot is idle again, and the single calls give what they gave before
    for slot in range(15):
        assert _lib.lib().zk_groth16_prove_wait(p.handle, C.c_uint32(slot), _p8(np.zeros(384, dtype=np.uint8))) == ZK_ERR_ARG
    after = p.prove_rs(c.wits[0], *c.rs[0])
    assert (after.a, after.b, after.c) == (before.a, before.b, before.c) and after.a + after.b + after.c == c.plain_g[0]
    assert [bytes(p.pool_points(g)) for g in (1, 2)] == pools
    # the shard of a point-sharded prover produces partial sums only
    p.shard(0, 2)
    assert many(G16, p.handle, c.sols(range(2)), c.rnd_g(range(2)), 2, 1, 192)[0] == ZK_ERR_ARG
    p.close()
    q = PIN.ZK(c.cs, c.pk_p)
    q.set_witness(c.wits[2])
    q.prove_async(*c.ds[2], 1)
    assert many(PINO, q.handle, c.sols(range(3)), c.rnd_p(range(3)), 3, 2, 480)[0] == ZK_ERR_ARG
    assert q.prove_wait(1).to_bytes() == c.plain_zk[2]
    rc, got, st = many(PINO, q.handle, c.sols(range(3)), c.rnd_p(range(3)), 3, 2, 480)
    assert (rc, st) == (0, [0] * 3) and got == c.exp_zk[:3]
    assert q.prove_with(c.wits[2], *c.ds[2]).to_bytes() == c.plain_zk[2]
    # null sols with no resident witness on a fresh handle
    fresh = Groth16(c.cs, c.pk_g)
    assert many(G16, fresh.handle, None, c.rnd_g(range(2)), 2, 1, 192)[0] == ZK_ERR_ARG
    fresh.close()
    q.close()


# ------------------------------------------------------------------------------------------------------------------ 4: an all-identity key
def test_an_all_identity_key_gives_the_identity_on_every_point(readme):
    c = readme
    zero = PKey(np.zeros(len(c.pk_g.g1), dtype=np.uint8), np.zeros(len(c.pk_g.g2), dtype=np.uint8))          # zero bytes: the uncompressed upload's identity
    p = Groth16(c.cs, zero)
    rc, got, st = many(G16, p.handle, c.sols(range(5)), c.rnd_g(range(5)), 5, 2, 192)
    assert (rc, st) == (0, [0] * 5)
    assert got == [INF[1] + INF[2] + INF[1]] * 5
    p.close()


# ------------------------------------------------------------------------------------------------------------------ 5: round trip to the verifier
def test_the_bytes_go_straight_into_the_compressed_verifiers(readme):
    c = readme
    p = Groth16(c.cs, c.pk_g)
    wits = [spoiled(c.wits[i]) if i == 2 else c.wits[i] for i in range(6)]
    proofs, codes = p.prove_many(c.rs[:6], wits, in_flight=4, return_status=True)
    assert codes == [0, 0, ZK_ERR_REMAINDER, 0, 0, 0]
    with c.vk_g.resident() as vk:
        ok, st = vk.verify_many(c.ios[:6], proofs, return_status=True, compressed=True)
    assert ok == [True, True, False, True, True, True] and st == [0, 0, ZK_ERR_ARG, 0, 0, 0]          # the zeroed row carries no compression flag
    p.close()
    for cls, ds in ((PIN.ZK, c.ds), (PIN.NonZK, None)):
        q = cls(c.cs, c.pk_p)
        proofs, codes = q.prove_many(ds[:6] if ds else None, wits, in_flight=3, return_status=True)
        assert codes == [0, 0, ZK_ERR_REMAINDER, 0, 0, 0]
        with c.vk_p.resident() as vk:
            ok, st = vk.verify_many(c.ios[:6], proofs, return_status=True, compressed=True)
        assert ok == [True, True, False, True, True, True] and st == [0, 0, ZK_ERR_ARG, 0, 0, 0]
        q.close()


# ------------------------------------------------------------------------------------------------------------------ 6: a device list
def test_a_device_list_gives_the_single_device_bytes(readme):
    from test_gpu_multidevice import physical
    c = readme
    _lib.set_device_list(physical([0, 0]))
    try:
        p = Groth16(c.cs, c.pk_g)
        sols = c.sols(range(4)) + frs(spoiled(c.wits[4]))
        rc, got, st = many(G16, p.handle, sols, c.rnd_g(range(5)), 5, 3, 192)
        assert (rc, st) == (0, [0, 0, 0, 0, ZK_ERR_REMAINDER]) and got == c.exp_g[:4] + [bytes(192)]
        rc, got, st = many(G16, p.handle, c.sols(range(5)), c.rnd_g(range(5)), 5, 0, 192)
        assert (rc, st) == (0, [0] * 5) and got == c.exp_g[:5]
        pr = p.prove_rs(c.wits[0], *c.rs[0])
        assert pr.a + pr.b + pr.c == c.plain_g[0]
        p.close()
        q = PIN.ZK(c.cs, c.pk_p)
        rc, got, st = many(PINO, q.handle, c.sols(range(5)), c.rnd_p(range(5)), 5, 0, 480)
        assert (rc, st) == (0, [0] * 5) and got == c.exp_zk[:5]
        q.close()
    finally:
        _lib.set_device_list([0])


# ------------------------------------------------------------------------------------------------------------------ 7: the hook, against the oracle's compressor
def hook(group, pts, zs):
    """pts: (x, y) of integers (G2: ((x0, x1), (y0, y1))) or None for the identity"""
    be = lambda v: int(v).to_bytes(48, "big")
    if group == 0:
        aff = b"".join(bytes(96) if q is None else be(q[0]) + be(q[1]) for q in pts)
    else:
        aff = b"".join(bytes(192) if q is None else be(q[0][1]) + be(q[0][0]) + be(q[1][1]) + be(q[1][0]) for q in pts)
    n, size = len(pts), 48 * (group + 1)
    a, z, out = np.frombuffer(aff, dtype=np.uint8), np.frombuffer(frs(zs), dtype=np.uint8), np.full(size * n, 0x55, dtype=np.uint8)
    rc = _lib.lib().zk_selftest_proof_wire(group, _p8(a), _p8(z), n, _p8(out))
    return rc, [bytes(out[size * i:size * i + size]) for i in range(n)]


def oracle_wire(group, q):
    if group == 0:
        return P.g1_compress(None if q is None else (P.Fp1(q[0]), P.Fp1(q[1])))
    return P.g2_compress(None if q is None else (P.Fp2(*q[0]), P.Fp2(*q[1])))


HALF = (Pm - 1) // 2


def hook_points(group):
    """a few dozen coordinate pairs no proof reaches (neither curve nor subgroup is asked for), the identity between them"""
    st = P.fr_stream(0x5EED9C00 + group)
    fp = lambda: (next(st) * next(st)) % Pm or 1
    if group == 0:
        x = fp()
        pts = [(x, 5), (x, Pm - 5), None, (fp(), HALF), (fp(), HALF + 1), (fp(), 1), (fp(), Pm - 1), None, None, (1, HALF), (Pm - 1, HALF + 1)]
        pts += [(fp(), fp()) for _ in range(24)]
    else:
        x = (fp(), fp())
        y = (fp(), fp())
        pts = [(x, y), (x, (Pm - y[0], Pm - y[1])), None,
               ((fp(), fp()), (HALF, 0)), ((fp(), fp()), (HALF + 1, 0)), ((fp(), fp()), (1, 0)), ((fp(), fp()), (Pm - 1, 0)),          # c1 = 0: c0 decides
               ((fp(), fp()), (fp(), HALF)), ((fp(), fp()), (fp(), HALF + 1)), None, None,                                       # c1 at the border
               ((fp(), 0), (0, HALF)), ((0, fp()), (0, HALF + 1)), ((fp(), fp()), (HALF + 1, HALF)), ((fp(), fp()), (HALF, HALF + 1))]
        pts += [((fp(), fp()), (fp(), fp())) for _ in range(20)]
    zs = [1, R - 1, 1, R - 1, 1, R - 1] + [next(st) or 1 for _ in range(len(pts) - 6)]
    return pts, zs


@pytest.mark.parametrize("group", [0, 1])
def test_the_conversion_kernel_against_the_oracles_compressor(group):
    pts, zs = hook_points(group)
    want = [oracle_wire(group, q) for q in pts]
    assert {w[0] & 0xE0 for w in want} == {0x80, 0xA0, 0xC0}
    rc, got = hook(group, pts, zs)
    assert rc == 0 and got == want
    # z = 1 and z = r - 1 on every point; one lane, a wave and one lane, a block and one lane
    for z in (1, R - 1):
        rc, got = hook(group, pts, [z] * len(pts))
        assert rc == 0 and got == want, z
    for n in (1, 65, 129):
        idx = [(7 * i + 3) % len(pts) for i in range(n)]
        rc, got = hook(group, [pts[i] for i in idx], [zs[i] for i in idx])
        assert rc == 0 and got == [want[i] for i in idx], n
    # what the hook itself refuses: z = 0, z >= r, a coordinate >= p
    assert hook(group, pts[:2], [0, 1])[0] == ZK_ERR_ARG
    assert hook(group, pts[:2], [1, R])[0] == ZK_ERR_ARG
    big = (Pm, 1) if group == 0 else ((1, Pm), (1, 1))
    assert hook(group, [pts[0], big], [1, 1])[0] == ZK_ERR_ARG
