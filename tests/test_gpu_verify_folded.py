"""zk_groth16_verify_folded (csrc/verify_resident.hip, csrc/pairing_dev.hip): one folded pairing equation for a whole batch under a resident key.
Both sides of the equation and the two sums that enter it (zk_selftest_groth16_fold) are held, byte for byte, to a path that shares nothing with the
device's: pyref's big-integer group law for the points and the HOST pairing (zk_pairing_product) for the GT values.  The statuses are held to
zk_groth16_verify_resident on the same inputs.  rho comes from pyref.fr_stream cut to 128 bits: every run is the same."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyref as P
from zukelang_amd import _lib
from zukelang_amd import r1cs as RC
from zukelang_amd.groth16 import Groth16
import oracle_lib as O
import test_gpu_verify_many as VM
import test_gpu_verify_resident as VR
from test_gpu_verify_resident import spoiled_batch          # noqa: F401  (the resident tests' fixture)

pytestmark = pytest.mark.gpu

R = P.R
ZK_OK, ZK_ERR_ARG, ZK_ERR_SCALAR_RANGE, ZK_ERR_HANDLE = 0, -1, -3, -7
VK_SLAB = 8192          # csrc/verify_resident.hip
u8, frs = VM.u8, VM.frs
g1b, g2b = P.g1_to_bytes, P.g2_to_bytes
A, B, Cc = (lambda p: p[:96]), (lambda p: p[96:288]), (lambda p: p[288:])


def rhos(seed, n):
    st = P.fr_stream(seed)
    return [(next(st) & ((1 << 128) - 1)) or 1 for _ in range(n)]


rho_bytes = lambda rho: b"".join(r.to_bytes(16, "little") for r in rho)


def folded(h, ios, proofs, rho, with_status=True):
    n = len(proofs)
    ok = C.c_int(9)
    st = (C.c_int32 * n)(*([9] * n))
    rc = _lib.lib().zk_groth16_verify_folded(h, u8(b"".join(ios)), u8(b"".join(proofs)), u8(rho_bytes(rho)), n, C.byref(ok), st if with_status else None)
    return rc, ok.value, list(st)


def selftest(h, ios, proofs, rho):
    n = len(proofs)
    bufs = [(C.c_uint8 * k)() for k in (576, 576, 96, 96)]
    st = (C.c_int32 * n)(*([9] * n))
    rc = _lib.lib().zk_selftest_groth16_fold(h, u8(b"".join(ios)), u8(b"".join(proofs)), u8(rho_bytes(rho)), n, *[C.cast(b, _lib._P8) for b in bufs], st)
    assert rc == 0
    return [bytes(b) for b in bufs] + [list(st)]


def expected(key, alpha, beta, ios, proofs, rho):
    """lhs, rhs, sum_c, sum_io of the folded equation from pyref's points and the host's pairing; ios as lists of integers, every proof taken as live"""
    ab, lt, gm, d = key
    n_io = len(lt) // 96
    sum_c = None
    for r, p in zip(rho, proofs):
        sum_c = P.pt_add(sum_c, P.pt_mul(P.g1_from_bytes(Cc(p)), r))
    t = [sum(r * io[k] for r, io in zip(rho, ios)) % R for k in range(n_io)]
    sum_io = P.msm([P.g1_from_bytes(lt[96 * k:96 * k + 96]) for k in range(n_io)], t)
    g1s = [g1b(P.pt_mul(P.g1_from_bytes(A(p)), r)) for r, p in zip(rho, proofs)] + [g1b(P.pt_neg(sum_io)), g1b(P.pt_neg(sum_c))]
    g2s = [B(p) for p in proofs] + [gm, d]
    lhs = VM.host_pairing(b"".join(g1s), b"".join(g2s))
    rhs = VM.host_pairing(g1b(P.pt_mul(P.g1_from_bytes(alpha), sum(rho))), beta)
    return lhs, rhs, g1b(sum_c), g1b(sum_io)


@pytest.fixture(scope="module")
def readme():
    """The README circuit (2 public values): the oracle's key with alpha and beta, 12 good oracle proofs, and the key's handle"""
    seed = 0x5EED00F0
    wit = [RC.readme_circuit(x) for x in range(3, 15)]
    cs = wit[0][0]
    key, ios, proofs = VM.g16_oracle(cs, [w for _, w in wit], seed)
    st = P.fr_stream(seed)
    toxic = [next(st) for _ in range(5)]
    pk1, pk2, _, _ = O.QAP(cs.n, cs.m, *VM.csrs(cs)).groth16_setup(frs(toxic), cs.mid)
    rc, h = VR.g16_upload(key)
    assert rc == 0
    yield key, pk1[:96], pk2[:192], ios, proofs, h
    assert VR.free(h) == 0


# ------------------------------------------------------------------------------------------------------------------ 1. bytes against an independent path
@pytest.mark.parametrize("count", [1, 2, 3, 8, 9, 65])          # 9: more pairs than the eight groups of a Miller wave; 65: a second block of the scaling and sum kernels, a ragged tree
def test_both_sides_and_both_sums_match_pyref_and_the_host_pairing(readme, count):
    key, alpha, beta, ios, proofs, h = readme
    idx = [i % 3 for i in range(count)] if count > 12 else list(range(count))
    io_i, pr = [ios[i] for i in idx], [proofs[i] for i in idx]
    io_b = [frs(x) for x in io_i]
    rho = rhos(0x5EED0100 + count, count)
    lhs, rhs, sum_c, sum_io, st = selftest(h, io_b, pr, rho)
    want = expected(key, alpha, beta, io_i, pr, rho)
    assert (sum_c, sum_io) == want[2:]
    assert lhs == want[0]
    assert rhs == want[1]
    assert lhs == rhs and st == [0] * count
    assert folded(h, io_b, pr, rho) == (0, 1, [0] * count)
    rc, ok, st = folded(h, io_b, pr, rho, with_status=False)
    assert (rc, ok) == (0, 1) and st == [9] * count                    # status == NULL: nothing written


# ------------------------------------------------------------------------------------------------------------------ 2. rho is used, and must be secret
def test_equal_coefficients_let_a_crafted_pair_through_and_different_ones_do_not(readme):
    key, alpha, beta, ios, proofs, h = readme
    D = P.pt_mul(P.G1, 0xD15EA5E)
    shift = lambda p, q: A(p) + B(p) + g1b(P.pt_add(P.g1_from_bytes(Cc(p)), q))
    pr = [shift(proofs[1], D), shift(proofs[2], P.pt_neg(D))]
    io_b = [frs(ios[1]), frs(ios[2])]
    assert VR.g16_res(h, io_b, pr) == (0, [0, 0], [0, 0])                # each proof alone is bad
    for _ in range(2):                                                   # and both answers are the same every time
        assert folded(h, io_b, pr, [7, 7]) == (0, 1, [0, 0])             # e(-[7] D, d) e([7] D, d) = 1: a CHOSEN rho lets the pair through
        assert folded(h, io_b, pr, [7, 8]) == (0, 0, [0, 0])


# ------------------------------------------------------------------------------------------------------------------ 3. the group law's corners in k_fold_sum
def test_equal_and_opposite_summands_and_an_identity_a(readme):
    key, alpha, beta, ios, proofs, h = readme
    io_b = [frs(ios[4])] * 2
    rho = rhos(0x5EED0103, 1) * 2
    lhs, rhs, sum_c, sum_io, st = selftest(h, io_b, [proofs[4]] * 2, rho)
    assert sum_c == g1b(P.pt_mul(P.g1_from_bytes(Cc(proofs[4])), 2 * rho[0])) and lhs == rhs
    assert folded(h, io_b, [proofs[4]] * 2, rho) == (0, 1, [0, 0])
    neg = A(proofs[4]) + B(proofs[4]) + g1b(P.pt_neg(P.g1_from_bytes(Cc(proofs[4]))))
    lhs, rhs, sum_c, sum_io, st = selftest(h, io_b, [proofs[4], neg], rho)
    assert sum_c == g1b(None) and st == [0, 0] and lhs != rhs
    assert folded(h, io_b, [proofs[4], neg], rho) == (0, 0, [0, 0])
    pr = [g1b(None) + proofs[4][96:], proofs[5]]                          # A = the identity, next to a good proof
    io2 = [frs(ios[4]), frs(ios[5])]
    rc, ok, st = VR.g16_res(h, io2, pr)
    assert rc == 0
    assert folded(h, io2, pr, rhos(0x5EED0104, 2)) == (0, int(all(ok)), st)


# ------------------------------------------------------------------------------------------------------------------ 4. rejections
def test_statuses_are_the_resident_calls_and_one_bad_proof_fails_the_batch(spoiled_batch, readme):
    key, io_b, proofs, host = spoiled_batch
    rc, h = VR.g16_upload(key)
    assert rc == 0
    rho = rhos(0x5EED0105, 12)
    rc, ok, st = VR.g16_res(h, io_b, proofs)
    assert rc == 0 and st == [x[0] for x in host] and any(st)
    assert folded(h, io_b, proofs, rho) == (0, 0, st)
    good = [i for i in range(12) if ok[i]]
    assert len(good) == 5
    assert folded(h, [io_b[i] for i in good], [proofs[i] for i in good], rho[:5]) == (0, 1, [0] * 5)
    # a rejected proof next to good ones: its status, and nothing of it in the fold -- the others still satisfy their part, the batch is refused all the same
    some = good[:2] + [1] + good[2:]
    rc, ok1, st1 = folded(h, [io_b[i] for i in some], [proofs[i] for i in some], rho[:6])
    assert (rc, ok1) == (0, 0) and st1 == [0, 0, host[1][0], 0, 0, 0]
    lhs, rhs, _, _, _ = selftest(h, [io_b[i] for i in some], [proofs[i] for i in some], rho[:6])
    assert lhs == rhs
    assert VR.free(h) == 0
    # every status 0, one proof wrong: C moved to another point of the subgroup / a public input moved below r
    key, alpha, beta, ios, pr, h = readme
    io_r = [frs(x) for x in ios[:5]]
    moved = pr[3][:288] + g1b(P.pt_add(P.g1_from_bytes(Cc(pr[3])), P.G1))
    assert folded(h, io_r, pr[:3] + [moved] + pr[4:5], rho[:5]) == (0, 0, [0] * 5)
    io_w = io_r[:2] + [frs([ios[2][0], (ios[2][1] + 1) % R])] + io_r[3:]
    assert folded(h, io_w, pr[:5], rho[:5]) == (0, 0, [0] * 5)
    assert folded(h, io_r, pr[:5], rho[:5]) == (0, 1, [0] * 5)


# ------------------------------------------------------------------------------------------------------------------ 5. public inputs
@pytest.mark.parametrize("n_io", [0, 1])
def test_no_or_one_public_input(n_io):
    a, b, c, dd, t, g, w = 11, 13, 17, 19, 23, 29, 31 if n_io else 0      # the keys of the resident tests: ab = e(G1, G2)^(a b - w t g - c dd)
    g1 = lambda k: g1b(P.pt_mul(P.G1, k % R))
    g2 = lambda k: g2b(P.pt_mul(P.G2, k % R))
    alpha, beta = g1(a * b - w * t * g - c * dd), g2(1)
    key = (VM.host_pairing(alpha, beta), g1(t) * n_io, g2(g), g2(dd))
    proofs = [g1(a) + g2(b) + g1(c), g1(a) + g2(b) + g1(c + 1), g1(2 * a) + g2(b * pow(2, -1, R)) + g1(c)]
    ios = [frs([w] * n_io)] * 3
    rc, h = VR.g16_upload(key)
    assert rc == 0
    rho = rhos(0x5EED0106 + n_io, 3)
    assert folded(h, ios, proofs, rho) == (0, 0, [0, 0, 0])
    good, r2 = [proofs[0], proofs[2]], [rho[0], rho[2]]
    assert folded(h, ios[:2], good, r2) == (0, 1, [0, 0])
    lhs, rhs, sum_c, sum_io, st = selftest(h, ios[:2], good, r2)
    assert (lhs, rhs, sum_c, sum_io) == expected(key, alpha, beta, [[w] * n_io] * 2, good, r2) and lhs == rhs
    if n_io:
        big = [ios[0], R.to_bytes(32, "little")]
        assert folded(h, big, good, r2) == (0, 0, [0, ZK_ERR_SCALAR_RANGE])
    else:
        assert sum_io == g1b(None)
    assert VR.free(h) == 0


def test_seventy_four_public_inputs():
    cs, w = RC.random_r1cs(48, 256, 4)
    seed = 0x5EED0074
    key, ios, proofs = VM.g16_oracle(cs, [w, w, w], seed)
    assert len(ios[0]) == 74
    st = P.fr_stream(seed)
    toxic = [next(st) for _ in range(5)]
    pk1, pk2, _, _ = O.QAP(cs.n, cs.m, *VM.csrs(cs)).groth16_setup(frs(toxic), cs.mid)
    io_b = [frs(x) for x in ios]
    rc, h = VR.g16_upload(key)
    assert rc == 0
    rho = rhos(0x5EED0108, 3)
    assert folded(h, io_b, proofs, rho) == (0, 1, [0] * 3)
    lhs, rhs, sum_c, sum_io, _ = selftest(h, io_b, proofs, rho)
    assert (lhs, rhs, sum_c, sum_io) == expected(key, pk1[:96], pk2[:192], ios, proofs, rho) and lhs == rhs
    wrong = [io_b[0], io_b[1][:32 * 40] + P.fr_to_bytes((ios[1][40] + 1) % R) + io_b[1][32 * 41:], io_b[2]]
    assert folded(h, wrong, proofs, rho) == (0, 0, [0] * 3)
    big = [io_b[0], io_b[1], io_b[2][:32 * 73] + (R + 5).to_bytes(32, "little")]
    assert folded(h, big, proofs, rho) == (0, 0, [0, 0, ZK_ERR_SCALAR_RANGE])
    assert VR.free(h) == 0


# ------------------------------------------------------------------------------------------------------------------ 6. slabs
def test_more_proofs_than_a_slab_fold_across_slabs(readme):
    key, alpha, beta, ios, proofs, h = readme
    n = VK_SLAB + 3
    io_b = [frs(x) for x in ios[:5]]
    io_all, pr = [io_b[i % 5] for i in range(n)], [proofs[i % 5] for i in range(n)]
    rho = rhos(0x5EED0109, n)
    assert folded(h, io_all, pr, rho, with_status=False)[:2] == (0, 1)
    lhs, rhs, sum_c, _, st = selftest(h, io_all, pr, rho)
    assert lhs == rhs and st == [0] * n
    by = [sum(rho[i] for i in range(j, n, 5)) % R for j in range(5)]          # five multiples instead of 8195
    assert sum_c == g1b(P.msm([P.g1_from_bytes(Cc(proofs[j])) for j in range(5)], by))
    bad = list(pr)
    i = VK_SLAB + 1
    bad[i] = pr[i][:288] + g1b(P.pt_add(P.g1_from_bytes(Cc(pr[i])), P.G1))
    rc, ok, st = folded(h, io_all, bad, rho)
    assert (rc, ok) == (0, 0) and st == [0] * n
    # the same handle at 2 and at 65 again: the workspaces have grown, nothing of the long call is left in them
    for m in (2, 65):
        assert folded(h, io_all[:m], pr[:m], rho[:m]) == (0, 1, [0] * m), m
        assert folded(h, io_all[i - 1:i + 1] + io_all[2:m], bad[i - 1:i + 1] + pr[2:m], rho[:m])[:2] == (0, 0), m


# ------------------------------------------------------------------------------------------------------------------ 7. arguments with a live handle, and Python
def test_argument_and_handle_errors_with_a_live_handle(readme):
    key, alpha, beta, ios, proofs, h = readme
    lib = _lib.lib()
    io, pr, rho = frs(ios[0]), proofs[0], rho_bytes([5])
    ok = C.c_int(9)
    assert lib.zk_groth16_verify_folded(h, None, None, None, 0, C.byref(ok), None) == 0 and ok.value == 1          # count = 0
    ok.value = 9
    assert lib.zk_groth16_verify_folded(h, None, u8(pr), u8(rho), 1, C.byref(ok), None) == ZK_ERR_ARG              # n_io = 2 and no inputs
    assert lib.zk_groth16_verify_folded(h, u8(io), u8(pr), u8(bytes(16)), 1, C.byref(ok), None) == ZK_ERR_ARG      # rho = 0
    assert lib.zk_groth16_verify_folded(h + 1, u8(io), u8(pr), u8(rho), 1, C.byref(ok), None) == ZK_ERR_HANDLE     # unknown, with a device present
    assert ok.value == 9
    g1, g2 = g1b(P.G1), g2b(P.G2)
    rc, hp = VR.pin_upload(g1 * 5, g2 * 7, 1)
    assert rc == 0
    assert lib.zk_groth16_verify_folded(hp, u8(io), u8(pr), u8(rho), 1, C.byref(ok), None) == ZK_ERR_HANDLE        # the other protocol's
    assert VR.free(hp) == 0
    assert lib.zk_groth16_verify_folded(hp, u8(io), u8(pr), u8(rho), 1, C.byref(ok), None) == ZK_ERR_HANDLE        # freed


def test_python_verify_all_and_fold_first(spoiled_batch):
    _lib.check(_lib.lib().zk_init(0))
    st = RC.fr_stream(0x5EED0079)
    rng = lambda: next(st)
    cs, _ = RC.iterated_cubic(16, 5)
    prover, _, vk = Groth16.generate(rng, cs)
    wits = [RC.iterated_cubic(16, x)[1] for x in (5, 6, 7)]
    proofs = [prover.prove_rs(w, next(st), next(st)) for w in wits]
    prover.close()
    ios = [[w[k] for k in range(cs.m) if not cs.mid[k]] for w in wits]
    changed = [type(p)(VM._another_point(p.a, 1), p.b, p.c) if i == 0 else p for i, p in enumerate(proofs)]
    with vk.resident() as rv:
        assert rv.verify_all(ios, proofs) is True                                       # rho drawn from `secrets`
        assert rv.verify_all(ios, changed) is False
        assert rv.verify_all(ios, proofs, rho=[3, 4, 5], return_status=True) == (True, [0, 0, 0])
        assert rv.verify_all([], []) is True
        with pytest.raises(ValueError):
            rv.verify_all(ios, proofs, rho=[3, 0, 5])
        assert rv.verify_many(ios, proofs, fold_first=True) == rv.verify_many(ios, proofs) == [True] * 3
        assert rv.verify_many(ios, changed, fold_first=True, return_status=True) == rv.verify_many(ios, changed, return_status=True) == ([False, True, True], [0] * 3)
    # the spoiled batch of the resident tests through the same two doors
    from zukelang_amd.groth16 import Proof, VKey
    key, io_b, pb, host = spoiled_batch
    ab, lt, gm, d = key
    prs = [Proof(A(p), B(p), Cc(p)) for p in pb]
    with VKey(b"", np.frombuffer(lt, dtype=np.uint8), b"", gm, d, ab).resident() as rv:
        want = rv.verify_many(io_b, prs, return_status=True)
        assert want == ([bool(x[1]) for x in host], [x[0] for x in host])
        assert rv.verify_many(io_b, prs, fold_first=True, return_status=True) == want
        assert rv.verify_all(io_b, prs, return_status=True) == (False, want[1])
