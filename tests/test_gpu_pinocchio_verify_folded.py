"""zk_pinocchio_verify_folded (csrc/verify_resident.hip): one folded pairing equation for a whole batch under a resident Pinocchio key.  The ten sums
that enter the key's pairs and the value of the left-hand side (zk_selftest_pinocchio_fold) are held, byte for byte, to a path that shares nothing with
the device's: tests/pinocchio_fold_model.py on pyref's big-integer group law for the points and the HOST pairing (zk_pairing_product) for the GT value.
The statuses are held to zk_pinocchio_verify_resident on the same inputs.  The coefficients come from pyref.fr_stream cut to 128 bits: every run is
the same.  From 65 proofs on the batches cycle three good proofs and five rows, and every big-integer multiple is memoised: 15 sets, not 65."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyref as P
from zukelang_amd import _lib
from zukelang_amd import pinocchio as PIN
from zukelang_amd import r1cs as RC
import oracle_lib as O
import pinocchio_fold_model as M
import pinocchio_handbuilt as H
import test_gpu_verify_many as VM
import test_gpu_verify_resident as VR
from test_gpu_verify_many import pinocchio_batch          # noqa: F401  (the batched verifier's fixture)

pytestmark = pytest.mark.gpu

R = P.R
ZK_OK, ZK_ERR_ARG, ZK_ERR_SCALAR_RANGE, ZK_ERR_HANDLE = 0, -1, -3, -7
VK_SLAB = 8192          # csrc/verify_resident.hip
u8, frs = VM.u8, VM.frs
g1b, g2b = P.g1_to_bytes, P.g2_to_bytes
GT_ONE = bytes(47) + b"\x01" + bytes(528)
D = P.pt_mul(P.G1, 0xD15EA5E)


def rows(seed, n):
    st = P.fr_stream(seed)
    return [[(next(st) & ((1 << 128) - 1)) or 1 for _ in range(5)] for _ in range(n)]


rho_bytes = lambda rho: b"".join(r.to_bytes(16, "little") for row in rho for r in row)
io_ints = lambda b: [int.from_bytes(b[k:k + 32], "little") for k in range(0, len(b), 32)]
_memo = {}


def mul(pt, k):
    """pyref's multiple, computed once per (point, scalar)"""
    if pt is None or not k:
        return None
    key = (g1b(pt) if isinstance(pt[0], P.Fp1) else g2b(pt), k)
    if key not in _memo:
        _memo[key] = P.pt_mul_jac(pt, k)
    return _memo[key]


def folded(h, ios, proofs, rho, with_status=True):
    n = len(proofs)
    ok = C.c_int(9)
    st = (C.c_int32 * n)(*([9] * n))
    rc = _lib.lib().zk_pinocchio_verify_folded(h, u8(b"".join(ios)), u8(b"".join(proofs)), u8(rho_bytes(rho)), n, C.byref(ok), st if with_status else None)
    return rc, ok.value, list(st)


def selftest(h, ios, proofs, rho):
    """(lhs_gt, sums_g1, sums_g2, statuses) of the hook"""
    n = len(proofs)
    bufs = [(C.c_uint8 * k)() for k in (576, 7 * 96, 3 * 192)]
    st = (C.c_int32 * n)(*([9] * n))
    rc = _lib.lib().zk_selftest_pinocchio_fold(h, u8(b"".join(ios)), u8(b"".join(proofs)), u8(rho_bytes(rho)), n, *[C.cast(b, _lib._P8) for b in bufs], st)
    assert rc == 0
    return [bytes(b) for b in bufs] + [list(st)]


def expected(vk1, vk2, ios, proofs, rho, with_lhs=True):
    """(lhs_gt, sums_g1, sums_g2) of the model: the sums as the hook's bytes, the left-hand side by the host's pairing over the model's count + 9 pairs"""
    s1, s2, pairs = M.fold(vk1, vk2, [io_ints(io) for io in ios], proofs, rho, mul=mul)
    lhs = VM.host_pairing(*M.pairs_bytes(pairs)) if with_lhs else None
    return (lhs,) + M.sums_bytes(s1, s2)


def oracle_pin(cs, witnesses, seed):
    """The oracle's Pinocchio key for `cs` and one ZK oracle proof per witness: (vk_g1, vk_g2, public inputs as bytes, proofs)"""
    csr = VM.csrs(cs)
    st = P.fr_stream(seed)
    toxic = frs([next(st) for _ in range(8)])
    ex = O.pinocchio_keygen_exponents(None, cs.n, cs.m, *csr, cs.mid, toxic, False)
    vk1, vk2 = O.points_of_exponents_g1(ex[2]), O.points_of_exponents_g2(ex[3])
    ios, proofs = [], []
    for w in witnesses:
        dv, dw, dy = (P.fr_to_bytes(next(st)) for _ in range(3))
        proofs.append(O.pinocchio_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), toxic, dv, dw, dy))
        ios.append(frs([w[k] for k in range(cs.m) if not cs.mid[k]]))
    return vk1, vk2, ios, proofs


@pytest.fixture(scope="module")
def pin(pinocchio_batch):
    """The batched verifier's fixture (iterated_cubic(6, x): proofs 0-3 good, 4 h tripled, 5 ww of another proof, 6 a public input changed, 7 yy off the
    curve, 8 good with vio + vv = O) and its key's handle"""
    vk1, vk2, ios, proofs, host = pinocchio_batch
    assert [x[1] for x in host] == [1, 1, 1, 1, 0, 0, 0, 0, 1]
    rc, h = VR.pin_upload(vk1, vk2, len(ios[0]) // 32)
    assert rc == 0
    yield vk1, vk2, ios, proofs, host, h
    assert VR.free(h) == 0


# ------------------------------------------------------------------------------------------------------------------ 1. bytes against an independent path
@pytest.mark.parametrize("count", [1, 2, 3, 8, 9, 65])          # 9: more pairs than the eight groups of a Miller wave; 65: a second block of the scaling and sum kernels, a ragged tree
def test_the_ten_sums_and_the_left_side_match_pyref_and_the_host_pairing(pin, count):
    vk1, vk2, ios, proofs, host, h = pin
    io, pr = [ios[i % 3] for i in range(count)], [proofs[i % 3] for i in range(count)]
    rho = rows(0x5EED0300 + count, count) if count < 65 else [rows(0x5EED0300, 5)[i % 5] for i in range(count)]
    lhs, s1, s2, st = selftest(h, io, pr, rho)
    want = expected(vk1, vk2, io, pr, rho)
    assert (s1, s2) == want[1:]
    assert lhs == want[0] == GT_ONE and st == [0] * count
    assert folded(h, io, pr, rho) == (0, 1, [0] * count)
    rc, ok, st = folded(h, io, pr, rho, with_status=False)
    assert (rc, ok) == (0, 1) and st == [9] * count                    # status == NULL: nothing written


# ------------------------------------------------------------------------------------------------------------------ 2. rho is used, and must be secret
def test_chosen_coefficients_let_crafted_proofs_through_across_two_proofs_and_inside_one(pin):
    vk1, vk2, ios, proofs, host, h = pin
    # across proofs: vavv moved by +D and -D
    pr = [M.moved(proofs[1], vavv=D), M.moved(proofs[2], vavv=P.pt_neg(D))]
    assert VR.pin_res(h, ios[1:3], pr) == (0, [0, 0], [0, 0])            # each proof alone is bad
    rho = rows(0x5EED0310, 2)
    same = [rho[0], [rho[0][0]] + rho[1][1:]]                            # rho_00 = rho_10, the other eight differ
    for _ in range(2):                                                   # and both answers are the same every time
        assert folded(h, ios[1:3], pr, same) == (0, 1, [0, 0])
        assert folded(h, ios[1:3], pr, rho) == (0, 0, [0, 0])
    # inside one proof: vavv moved by +D, yayy by -D, both meet one2
    one = [M.moved(proofs[3], vavv=D, yayy=P.pt_neg(D))]
    assert VR.pin_res(h, ios[3:4], one) == (0, [0], [0])
    row = rows(0x5EED0311, 1)[0]
    assert folded(h, ios[3:4], one, [[row[0], row[1], row[0], row[3], row[4]]]) == (0, 1, [0])          # rho_i0 = rho_i2
    assert folded(h, ios[3:4], one, [row]) == (0, 0, [0])
    assert folded(h, ios[2:4], [proofs[2]] + one, [rows(0x5EED0312, 1)[0], row]) == (0, 0, [0, 0])      # ... and next to a good proof


# ------------------------------------------------------------------------------------------------------------------ 3. the group law's corners
def test_equal_and_opposite_summands_in_both_groups_and_an_identity_pair(pin):
    vk1, vk2, ios, proofs, host, h = pin
    row = rows(0x5EED0320, 1)[0]
    # a proof repeated with the same row: equal summands in all nine tracked sums -> each the doubled multiple
    lhs, s1, s2, st = selftest(h, [ios[0]] * 2, [proofs[0]] * 2, [row] * 2)
    assert (s1, s2) == expected(vk1, vk2, [ios[0]], [proofs[0]], [[2 * r for r in row]], with_lhs=False)[1:]
    assert lhs == GT_ONE and st == [0, 0]
    assert folded(h, [ios[0]] * 2, [proofs[0]] * 2, [row] * 2) == (0, 1, [0, 0])
    # a proof and its negation in ww and waww under the same rho_1 (and rho_3): opposite summands in G2
    pts = M.proof_points(proofs[0])
    pts["ww"], pts["waww"] = P.pt_neg(pts["ww"]), P.pt_neg(pts["waww"])
    neg = M.proof_bytes(pts)
    lhs, s1, s2, st = selftest(h, [ios[0]] * 2, [proofs[0], neg], [row] * 2)
    assert s2 == g2b(None) * 3 and st == [0, 0] and lhs != GT_ONE
    assert (s1, s2) == expected(vk1, vk2, [ios[0]] * 2, [proofs[0], neg], [row] * 2, with_lhs=False)[1:]
    rc, ok, st = VR.pin_res(h, [ios[0]] * 2, [proofs[0], neg])
    assert (rc, ok, st) == (0, [1, 0], [0, 0])
    assert folded(h, [ios[0]] * 2, [proofs[0], neg], [row] * 2) == (0, 0, [0, 0])
    # the proof whose vio + vv is the identity: its Miller pair contributes 1
    rc, ok, st = VR.pin_res(h, ios[8:9], proofs[8:9])
    assert rc == 0
    assert folded(h, ios[8:9], proofs[8:9], [row]) == (0, int(all(ok)), st)
    mix_io, mix = [ios[0], ios[8], ios[1]], [proofs[0], proofs[8], proofs[1]]
    rho = rows(0x5EED0321, 3)
    rc, ok, st = VR.pin_res(h, mix_io, mix)
    assert rc == 0 and all(ok)
    assert folded(h, mix_io, mix, rho) == (0, int(all(ok)), st)
    lhs, s1, s2, st = selftest(h, mix_io, mix, rho)
    assert (lhs, s1, s2) == expected(vk1, vk2, mix_io, mix, rho)


def test_a_proof_whose_vv_plus_yy_is_the_identity(pin):
    """[rho_3](vv + yy) is one multiple of a sum formed on the device: with yy = -vv the sum is the identity before it is scaled"""
    vk1, vk2, ios, proofs, host, h = pin
    pts = M.proof_points(proofs[0])
    pts["yy"] = P.pt_neg(pts["vv"])
    flat = M.proof_bytes(pts)
    assert VR.pin_res(h, ios[:1], [flat]) == (0, [0], [0])               # every point is good, the proof is not
    rho = rows(0x5EED0322, 2)
    lhs, s1, s2, st = selftest(h, ios[:1], [flat], rho[:1])
    assert (lhs, s1, s2) == expected(vk1, vk2, ios[:1], [flat], rho[:1]) and st == [0] and lhs != GT_ONE
    assert s1[4 * 96:5 * 96] == g1b(None)                                # S_bgm2
    assert folded(h, ios[:1], [flat], rho[:1]) == (0, 0, [0])
    lhs, s1, s2, st = selftest(h, [ios[1], ios[0]], [proofs[1], flat], rho)          # next to a good proof: S_bgm2 is the good proof's alone
    assert (lhs, s1, s2) == expected(vk1, vk2, [ios[1], ios[0]], [proofs[1], flat], rho) and st == [0, 0]
    assert s1[4 * 96:5 * 96] == g1b(P.pt_mul_jac(P.pt_add(M.proof_points(proofs[1])["vv"], M.proof_points(proofs[1])["yy"]), rho[0][3]))
    assert folded(h, [ios[1], ios[0]], [proofs[1], flat], rho) == (0, 0, [0, 0])


# ------------------------------------------------------------------------------------------------------------------ 4. rejections
def test_statuses_are_the_resident_calls_and_one_bad_proof_fails_the_batch(pin):
    vk1, vk2, ios, proofs, host, h = pin
    io_all, pr_all = list(ios), list(proofs)
    for q in range(8):                                                   # every proof point spoiled alone, the kinds in turn
        pr_all.append(VR._spoil(proofs[0], q, q % 3)); io_all.append(ios[0])
    n = len(pr_all)
    rho = rows(0x5EED0330, n)
    rc, ok, st = VR.pin_res(h, io_all, pr_all)
    assert rc == 0 and st[:9] == [x[0] for x in host] and all(st[9:]) and ok[9:] == [0] * 8
    assert folded(h, io_all, pr_all, rho) == (0, 0, st)
    good = [0, 1, 2, 3, 8]
    assert folded(h, [ios[i] for i in good], [proofs[i] for i in good], rho[:5]) == (0, 1, [0] * 5)
    # a rejected proof between good ones: its status, and nothing of it in the fold -- the others still satisfy their part, the batch is refused all the same
    some_io, some = [ios[0], ios[0], ios[1]], [proofs[0], pr_all[9 + 1], proofs[1]]
    assert folded(h, some_io, some, rho[:3]) == (0, 0, [0, st[9 + 1], 0])
    lhs, s1, s2, st3 = selftest(h, some_io, some, rho[:3])
    assert lhs == GT_ONE and st3 == [0, st[9 + 1], 0]
    assert (s1, s2) == expected(vk1, vk2, [ios[0], ios[1]], [proofs[0], proofs[1]], [rho[0], rho[2]], with_lhs=False)[1:]
    # every status 0, one proof wrong: h tripled / ww of another proof / a public input changed below r
    for bad in (4, 5, 6):
        assert folded(h, [ios[0], ios[bad], ios[1]], [proofs[0], proofs[bad], proofs[1]], rho[:3]) == (0, 0, [0, 0, 0]), bad
    # a public input >= r
    big = ios[1][:32] + (R + 1).to_bytes(32, "little") + ios[1][64:]
    assert folded(h, [ios[0], big], proofs[:2], rho[:2]) == (0, 0, [0, ZK_ERR_SCALAR_RANGE])


# ------------------------------------------------------------------------------------------------------------------ 5. public inputs
def test_a_key_without_public_inputs():
    vk1 = H.g1(1) + H.g1(H.AW) + H.g1(H.BGM)
    vk2 = H.g2(1) + H.g2(H.AV) + H.g2(H.AY) + H.g2(1) + H.g2(H.BGM2) + H.g2(1)
    good = H.proof(0, io=[])
    assert VM.pin_host(vk1, vk2, b"", good) == (0, 1)
    rc, h = VR.pin_upload(vk1, vk2, 0)
    assert rc == 0
    rho = rows(0x5EED0340, 2)
    lhs, s1, s2, st = selftest(h, [b"", b""], [good, good], rho)               # io_scalars is null
    assert (lhs, s1, s2) == expected(vk1, vk2, [b"", b""], [good, good], rho) and lhs == GT_ONE
    assert s1[6 * 96:] == g1b(None)                                              # S_yio
    assert folded(h, [b"", b""], [good, good], rho) == (0, 1, [0, 0])
    wrong = M.moved(good, h=P.G1)
    assert folded(h, [b"", b""], [good, wrong], rho) == (0, 0, [0, 0])
    assert VR.free(h) == 0


def test_one_public_input():
    cs, _ = RC.iterated_cubic(2, 9)
    mid = np.array([0, 1, 1, 1], dtype=np.uint8)                                 # ONE alone is public
    cs = RC.R1CS(cs.n, cs.m, cs.L, cs.R, cs.O, mid)
    vk1, vk2, ios, proofs = oracle_pin(cs, [RC.iterated_cubic(2, x)[1] for x in (9, 10)], 0x5EED0341)
    assert len(ios[0]) == 32 and VM.pin_host(vk1, vk2, ios[0], proofs[0]) == (0, 1)
    rc, h = VR.pin_upload(vk1, vk2, 1)
    assert rc == 0
    rho = rows(0x5EED0342, 2)
    lhs, s1, s2, st = selftest(h, ios, proofs, rho)
    assert (lhs, s1, s2) == expected(vk1, vk2, ios, proofs, rho) and lhs == GT_ONE
    assert folded(h, ios, proofs, rho) == (0, 1, [0, 0])
    assert folded(h, [ios[0], frs([2])], proofs, rho) == (0, 0, [0, 0])
    assert folded(h, [ios[0], R.to_bytes(32, "little")], proofs, rho) == (0, 0, [0, ZK_ERR_SCALAR_RANGE])
    assert VR.free(h) == 0


def test_seventy_four_public_inputs():
    cs, w = RC.random_r1cs(48, 256, 4)
    vk1, vk2, ios, proofs = oracle_pin(cs, [w, w, w], 0x5EED0374)
    assert len(ios[0]) == 32 * 74
    rc, h = VR.pin_upload(vk1, vk2, 74)
    assert rc == 0
    rho = rows(0x5EED0375, 3)
    assert folded(h, ios, proofs, rho) == (0, 1, [0] * 3)
    lhs, s1, s2, st = selftest(h, ios, proofs, rho)
    assert (lhs, s1, s2) == expected(vk1, vk2, ios, proofs, rho) and lhs == GT_ONE
    x = io_ints(ios[1])
    wrong = [ios[0], ios[1][:32 * 40] + P.fr_to_bytes((x[40] + 1) % R) + ios[1][32 * 41:], ios[2]]
    assert folded(h, wrong, proofs, rho) == (0, 0, [0] * 3)
    big = [ios[0], ios[1], ios[2][:32 * 73] + (R + 5).to_bytes(32, "little")]
    assert folded(h, big, proofs, rho) == (0, 0, [0, 0, ZK_ERR_SCALAR_RANGE])
    assert VR.free(h) == 0


# ------------------------------------------------------------------------------------------------------------------ 6. slabs
def test_more_proofs_than_a_slab_fold_across_slabs(pin):
    vk1, vk2, ios, proofs, host, h = pin
    n = VK_SLAB + 3
    five = rows(0x5EED0350, 5)
    io_all, pr, rho = [ios[i % 3] for i in range(n)], [proofs[i % 3] for i in range(n)], [five[i % 5] for i in range(n)]
    assert folded(h, io_all, pr, rho, with_status=False)[:2] == (0, 1)
    lhs, s1, s2, st = selftest(h, io_all, pr, rho)
    assert lhs == GT_ONE and st == [0] * n
    # every sum is linear in its coefficients: the fifteen (proof, row) combinations, each with its row times the number of times it occurs
    times = {}
    for i in range(n):
        times[(i % 3, i % 5)] = times.get((i % 3, i % 5), 0) + 1
    combos = sorted(times)
    want = expected(vk1, vk2, [ios[j] for j, _ in combos], [proofs[j] for j, _ in combos], [[times[c] * r % R for r in five[c[1]]] for c in combos], with_lhs=False)
    assert (s1, s2) == want[1:]
    bad = list(pr)
    i = VK_SLAB + 1
    bad[i] = M.moved(pr[i], h=P.G1)
    rc, ok, st = folded(h, io_all, bad, rho)
    assert (rc, ok) == (0, 0) and st == [0] * n
    # the same handle at 2 and at 65 again: the workspaces have grown, nothing of the long call is left in them
    for m in (2, 65):
        assert folded(h, io_all[:m], pr[:m], rho[:m]) == (0, 1, [0] * m), m
        assert folded(h, io_all[i - 1:i + 1] + io_all[2:m], bad[i - 1:i + 1] + pr[2:m], rho[:m])[:2] == (0, 0), m


# ------------------------------------------------------------------------------------------------------------------ 7. arguments with a live handle, and Python
def test_argument_and_handle_errors_with_a_live_handle(pin):
    vk1, vk2, ios, proofs, host, h = pin
    lib = _lib.lib()
    io, pr, rho = ios[0], proofs[0], rho_bytes([[5, 6, 7, 8, 9]])
    ok = C.c_int(9)
    assert lib.zk_pinocchio_verify_folded(h, None, None, None, 0, C.byref(ok), None) == 0 and ok.value == 1          # count = 0
    ok.value = 9
    assert lib.zk_pinocchio_verify_folded(h, None, u8(pr), u8(rho), 1, C.byref(ok), None) == ZK_ERR_ARG              # n_io = 2 and no inputs
    assert lib.zk_pinocchio_verify_folded(h, u8(io), u8(pr), u8(rho[:64] + bytes(16)), 1, C.byref(ok), None) == ZK_ERR_ARG          # rho_4 = 0
    assert lib.zk_pinocchio_verify_folded(h + 1, u8(io), u8(pr), u8(rho), 1, C.byref(ok), None) == ZK_ERR_HANDLE     # unknown, with a device present
    assert ok.value == 9
    # the resident call before and after a folded call on the same handle: the same bytes
    before = VR.pin_res(h, ios, proofs)
    assert before == (0, [x[1] for x in host], [x[0] for x in host])
    assert folded(h, ios, proofs, rows(0x5EED0360, 9))[:2] == (0, 0)
    assert VR.pin_res(h, ios, proofs) == before
    g1, g2 = g1b(P.G1), g2b(P.G2)
    rc, hg = VR.g16_upload((bytes(576), g1 * 2, g2, g2))
    assert rc == 0
    assert lib.zk_pinocchio_verify_folded(hg, u8(io), u8(pr), u8(rho), 1, C.byref(ok), None) == ZK_ERR_HANDLE        # the other protocol's
    assert lib.zk_groth16_verify_folded(h, u8(io), u8(pr), u8(rho), 1, C.byref(ok), None) == ZK_ERR_HANDLE           # ... and the other way round
    assert VR.free(hg) == 0
    assert lib.zk_pinocchio_verify_folded(hg, u8(io), u8(pr), u8(rho), 1, C.byref(ok), None) == ZK_ERR_HANDLE        # freed
    assert ok.value == 9


def test_python_verify_all_and_fold_first(pin):
    vk1, vk2, ios, proofs, host, h = pin
    vk = PIN.VKey(np.frombuffer(vk1, dtype=np.uint8), np.frombuffer(vk2, dtype=np.uint8))
    good = [0, 1, 2, 3, 8]
    gio, gpr = [ios[i] for i in good], [proofs[i] for i in good]
    with vk.resident() as rv:
        assert isinstance(rv, PIN.PinocchioResidentVKey)
        assert rv.verify_all(gio, gpr) is True                                              # rows drawn from `secrets`
        assert rv.verify_all(ios, proofs) is False
        assert rv.verify_all(gio, gpr, rho=rows(0x5EED0370, 5), return_status=True) == (True, [0] * 5)
        assert rv.verify_all(ios, proofs, rho=rows(0x5EED0371, 9), return_status=True) == (False, [x[0] for x in host])
        assert rv.verify_all([], []) is True
        with pytest.raises(ValueError):
            rv.verify_all(gio, gpr, rho=[[1, 2, 3, 4, 5]] * 4 + [[1, 2, 3, 0, 5]])
        assert rv.verify_many(gio, gpr, fold_first=True) == rv.verify_many(gio, gpr) == [True] * 5
        want = rv.verify_many(ios, proofs, return_status=True)
        assert want == ([bool(x[1]) for x in host], [x[0] for x in host])
        assert rv.verify_many(ios, proofs, fold_first=True, return_status=True) == want     # a failed fold falls through to the per-proof call
    with pytest.raises(ValueError):
        rv.verify_all(gio, gpr)                                                             # closed
