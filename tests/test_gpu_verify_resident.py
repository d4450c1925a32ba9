"""Resident verification keys (csrc/verify_resident.hip): zk_groth16_verify_resident / zk_pinocchio_verify_resident against the batched verifiers
(zk_*_verify_many) and the single-proof host verifiers on the same keys and inputs -- `ok` and `status` byte for byte -- on batches that hold good
proofs and proofs spoiled one point or one input at a time, on one handle called with growing and shrinking counts, on keys with 0, 1 and 74
public inputs, on defective keys (the upload fails with the host's code) and on handles that are freed or of the other protocol."""
import ctypes as C
import json
import os

import pytest

from oracle import pyref as P
from zukelang_amd import _lib
from zukelang_amd import pinocchio as PIN
from zukelang_amd import r1cs as RC
from zukelang_amd.groth16 import Groth16
import oracle_lib as O
import test_gpu_verify_many as VM
from test_gpu_verify_many import pinocchio_batch          # noqa: F401  (the existing batch fixture)

pytestmark = pytest.mark.gpu

R = P.R
ZK_OK, ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE, ZK_ERR_SCALAR_RANGE, ZK_ERR_HANDLE = 0, -1, -2, -3, -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORSION = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_points.json")))["points"]
u8, frs = VM.u8, VM.frs


def torsion(group, what):
    return bytes.fromhex(next(r["hex"] for r in TORSION if r["group"] == group and r["what"] == what))


def g16_upload(key):
    ab, lt, gm, d = key
    h = C.c_uint64(0)
    rc = _lib.lib().zk_groth16_vk_upload(u8(ab), u8(lt), len(lt) // 96, u8(gm), u8(d), C.byref(h))
    return rc, h.value


def pin_upload(vk1, vk2, n_io):
    h = C.c_uint64(0)
    rc = _lib.lib().zk_pinocchio_vk_upload(u8(vk1), u8(vk2), n_io, C.byref(h))
    return rc, h.value


def resident(call, h, ios, proofs, with_status=True):
    n = len(proofs)
    ok = (C.c_uint8 * n)(*([9] * n))
    st = (C.c_int32 * n)(*([9] * n))
    rc = getattr(_lib.lib(), call)(h, u8(b"".join(ios)), u8(b"".join(proofs)), n, C.cast(ok, _lib._P8), st if with_status else None)
    return rc, list(ok), list(st)


g16_res = lambda h, ios, proofs, **kw: resident("zk_groth16_verify_resident", h, ios, proofs, **kw)
pin_res = lambda h, ios, proofs, **kw: resident("zk_pinocchio_verify_resident", h, ios, proofs, **kw)
free = lambda h: _lib.lib().zk_vk_free(C.c_uint64(h))


# ------------------------------------------------------------------------------------------------------------------ Groth16
@pytest.fixture(scope="module")
def spoiled_batch():
    """The README circuit: 12 oracle proofs (x = 3 .. 14), five intact, seven spoiled one at a time, and what the host says about each."""
    wit = [RC.readme_circuit(x) for x in range(3, 15)]
    cs = wit[0][0]
    key, ios, proofs = VM.g16_oracle(cs, [w for _, w in wit], 0x5EED0012)
    A, B, Cc = (lambda p: p[:96]), (lambda p: p[96:288]), (lambda p: p[288:])
    off = bytearray(proofs[1]); off[95] ^= 1
    proofs[1] = bytes(off)                                                                                   # A off the curve
    proofs[3] = A(proofs[3]) + bytes([proofs[3][96] | 0x80]) + proofs[3][97:]                                # B: bad encoding
    proofs[4] = A(proofs[4]) + B(proofs[4]) + torsion(0, "torsion 11")                                       # C on the curve, of order 11^k
    proofs[6] = A(proofs[6]) + B(proofs[6]) + VM._g1_outside_subgroup()                                      # C a random point of the curve
    io_b = [frs(x) for x in ios]
    io_b[7] = io_b[7][:-32] + (R + 2).to_bytes(32, "little")                                                 # a public input >= r
    io_b[9] = frs(ios[9][:-1] + [(ios[9][-1] + 1) % R])                                                      # a wrong public input
    proofs[10] = proofs[0]                                                                                   # a valid proof of another witness
    host = [VM.g16_host(key, io_b[i], proofs[i]) for i in range(12)]
    return key, io_b, proofs, host


def test_groth16_resident_matches_many_and_twelve_host_calls(spoiled_batch):
    key, ios, proofs, host = spoiled_batch
    assert [h[1] for h in host] == [1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1]
    assert [h[0] for h in host] == [0, ZK_ERR_NOT_ON_CURVE, 0, ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE, 0, ZK_ERR_NOT_ON_CURVE, ZK_ERR_SCALAR_RANGE, 0, 0, 0, 0]
    rc, h = g16_upload(key)
    assert rc == 0 and h != 0
    proto, n_io = C.c_int(-1), C.c_uint64(99)
    assert _lib.lib().zk_vk_info(h, C.byref(proto), C.byref(n_io)) == 0 and (proto.value, n_io.value) == (0, len(key[1]) // 96)
    assert _lib.lib().zk_vk_info(h, None, None) == 0
    many = VM.g16_many(key, ios, proofs)
    got = g16_res(h, ios, proofs)
    assert got == many and got == (0, [x[1] for x in host], [x[0] for x in host])
    rc, ok, st = g16_res(h, ios, proofs, with_status=False)
    assert rc == 0 and ok == [x[1] for x in host] and st == [9] * 12                                          # status == NULL: nothing written
    # the same handle: 3 proofs, then 65 (one past eight waves of eight Miller groups; the workspaces grow), then 2 (nothing stale)
    for n in (3, 65, 2):
        idx = [(5 * i + 1) % 12 for i in range(n)]
        i2, p2 = [ios[i] for i in idx], [proofs[i] for i in idx]
        assert g16_res(h, i2, p2) == (0, [host[i][1] for i in idx], [host[i][0] for i in idx]), n
        if n == 65:
            assert VM.g16_many(key, i2, p2) == g16_res(h, i2, p2)
    # count = 0 touches nothing
    ok = (C.c_uint8 * 2)(7, 7)
    assert _lib.lib().zk_groth16_verify_resident(h, None, None, 0, C.cast(ok, _lib._P8), None) == 0 and list(ok) == [7, 7]
    assert _lib.lib().zk_groth16_verify_resident(h, u8(ios[0]), None, 1, C.cast(ok, _lib._P8), None) == ZK_ERR_ARG
    assert _lib.lib().zk_groth16_verify_resident(h, u8(ios[0]), u8(proofs[0]), 1, None, None) == ZK_ERR_ARG
    assert _lib.lib().zk_groth16_verify_resident(h, None, u8(proofs[0]), 1, C.cast(ok, _lib._P8), None) == ZK_ERR_ARG
    assert _lib.lib().zk_groth16_verify_resident(h, u8(ios[0]), u8(proofs[0]), (1 << 24) + 1, C.cast(ok, _lib._P8), None) == ZK_ERR_ARG
    # a freed handle
    assert free(h) == 0
    assert g16_res(h, ios, proofs)[0] == ZK_ERR_HANDLE and free(h) == ZK_ERR_HANDLE and _lib.lib().zk_vk_info(h, None, None) == ZK_ERR_HANDLE


def test_groth16_bad_key_fails_the_upload_with_the_hosts_code(spoiled_batch):
    key, ios, proofs, host = spoiled_batch
    ab, lt, gm, d = key
    bad = bytearray(gm); bad[191] ^= 1
    bad_d = bytes([d[0] | 0x80]) + d[1:]
    cases = ((ab, lt, bytes(bad), d), (ab, lt, gm, bad_d), (ab, VM._g1_outside_subgroup() + lt[96:], gm, d), (ab, lt, torsion(1, "torsion 13"), d),
             (ab, lt[:96] + torsion(0, "torsion 3"), gm, d), (ab, torsion(0, "torsion 3 + subgroup") + lt[96:], bytes(bad), bad_d))
    for k2 in cases:
        want = VM.g16_host(k2, ios[0], proofs[0])[0]
        assert want in (ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE)
        assert g16_upload(k2) == (want, 0)                                                                     # the host's code, and no handle
        assert VM.g16_many(k2, ios[:2], proofs[:2])[0] == want
    # a malformed ab is kept and compared on bytes: no proof passes, no call fails
    rc, h = g16_upload((bytes(576), lt, gm, d))
    assert rc == 0
    assert g16_res(h, ios, proofs) == (0, [0] * 12, [x[0] for x in host])
    assert free(h) == 0


def test_a_live_handle_pins_the_device_list():
    g1, g2 = P.g1_to_bytes(P.G1), P.g2_to_bytes(P.G2)
    rc, h = g16_upload((bytes(576), g1, g2, g2))
    assert rc == 0
    before = _lib.device_list()
    other = before + before[:1]
    assert _lib.lib().zk_set_device_list((C.c_int32 * len(other))(*other), len(other)) == ZK_ERR_ARG          # a key handle is alive: the list may not change
    assert _lib.device_list() == before
    assert free(h) == 0


@pytest.mark.parametrize("n_io", [0, 1])
def test_groth16_resident_with_no_or_one_public_input(n_io):
    a, b, c, dd, t, g, w = 11, 13, 17, 19, 23, 29, 31 if n_io else 0
    g1 = lambda k: P.g1_to_bytes(P.pt_mul(P.G1, k % R))
    g2 = lambda k: P.g2_to_bytes(P.pt_mul(P.G2, k % R))
    ab = VM.host_pairing(g1(a * b - w * t * g - c * dd), g2(1))
    key = (ab, g1(t) * n_io, g2(g), g2(dd))
    proofs = [g1(a) + g2(b) + g1(c), g1(a) + g2(b) + g1(c + 1), g1(2 * a) + g2(b * pow(2, -1, R)) + g1(c)]
    ios = [frs([w] * n_io)] * 3
    rc, h = g16_upload(key)
    assert rc == 0
    n = C.c_uint64(99)
    assert _lib.lib().zk_vk_info(h, None, C.byref(n)) == 0 and n.value == n_io
    assert g16_res(h, ios, proofs) == (0, [1, 0, 1], [0, 0, 0]) == VM.g16_many(key, ios, proofs)
    if n_io:
        big = [ios[0], (R).to_bytes(32, "little"), ios[2]]
        assert g16_res(h, big, proofs) == (0, [1, 0, 1], [0, ZK_ERR_SCALAR_RANGE, 0]) == VM.g16_many(key, big, proofs)
    assert free(h) == 0


def test_groth16_resident_with_seventy_four_public_inputs():
    cs, w = RC.random_r1cs(48, 256, 4)
    assert int((cs.mid == 0).sum()) >= 70
    key, ios, proofs = VM.g16_oracle(cs, [w, w, w], 0x5EED0074)
    io_b = [frs(x) for x in ios]
    io_b[1] = io_b[1][:32 * 40] + P.fr_to_bytes((ios[1][40] + 1) % R) + io_b[1][32 * 41:]
    io_b[2] = io_b[2][:32 * 73] + (R + 5).to_bytes(32, "little") + io_b[2][32 * 74:]
    rc, h = g16_upload(key)
    assert rc == 0
    assert g16_res(h, io_b, proofs) == (0, [1, 0, 0], [0, 0, ZK_ERR_SCALAR_RANGE]) == VM.g16_many(key, io_b, proofs)
    assert free(h) == 0


# ------------------------------------------------------------------------------------------------------------------ Pinocchio
PIN_POINTS = (("vv", 0, 0), ("ww", 96, 1), ("yy", 288, 0), ("h", 384, 0), ("vavv", 480, 0), ("waww", 576, 1), ("yayy", 768, 0), ("bvwy", 864, 0))


def _spoil(proof, q, kind):
    """point q of the proof (the host's order) made bad: 0 off the curve, 1 bad encoding, 2 on the curve outside the subgroup (a fixture torsion point)"""
    _, off, group = PIN_POINTS[q]
    size = 192 if group else 96
    pt = bytearray(proof[off:off + size])
    if kind == 0:
        pt[-1] ^= 1
    elif kind == 1:
        pt[0] |= 0x80
    else:
        pt = torsion(group, "torsion 23" if group else "torsion 3")
    return proof[:off] + bytes(pt) + proof[off + size:]


def test_pinocchio_resident_matches_many_and_the_host_calls(pinocchio_batch):
    vk1, vk2, ios, proofs, host = pinocchio_batch
    n_io = len(ios[0]) // 32
    ios, proofs = list(ios), list(proofs)
    # NonZK proofs (delta_v = delta_w = delta_y = 0) next to the ZK ones of the fixture
    cs, _ = RC.iterated_cubic(6, 9)
    csr = VM.csrs(cs)
    st = P.fr_stream(0x5EED0003)
    toxic = frs([next(st) for _ in range(8)])
    zero = P.fr_to_bytes(0)
    for x in (30, 31):
        _, w = RC.iterated_cubic(6, x)
        proofs.append(O.pinocchio_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), toxic, zero, zero, zero))
        ios.append(frs([w[k] for k in range(cs.m) if not cs.mid[k]]))
    # every proof point spoiled alone, the kinds in turn; then two at once: the earlier one in the host's order decides
    for q in range(8):
        proofs.append(_spoil(proofs[0], q, q % 3)); ios.append(ios[0])
        proofs.append(_spoil(proofs[9], q, (q + 2) % 3)); ios.append(ios[9])          # a NonZK proof
    for q in range(7):
        proofs.append(_spoil(_spoil(proofs[1], q, 2), q + 1, 1)); ios.append(ios[1])
    proofs.append(_spoil(proofs[2], 7, 2)); ios.append(ios[2][:32] + (R + 1).to_bytes(32, "little") + ios[2][64:])      # a bad point beats a bad scalar
    proofs.append(proofs[2]); ios.append(ios[2][:32] + (R + 1).to_bytes(32, "little") + ios[2][64:])
    want = [VM.pin_host(vk1, vk2, io, pr) for io, pr in zip(ios, proofs)]
    assert [x[1] for x in want[9:11]] == [1, 1] and not any(x[1] for x in want[11:])
    assert {x[0] for x in want[11:]} == {ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE, ZK_ERR_SCALAR_RANGE}
    rc, h = pin_upload(vk1, vk2, n_io)
    assert rc == 0
    proto = C.c_int(-1)
    assert _lib.lib().zk_vk_info(h, C.byref(proto), None) == 0 and proto.value == 1
    many = VM.pin_many(vk1, vk2, ios, proofs)
    got = pin_res(h, ios, proofs)
    assert got == many and got == (0, [x[1] for x in want], [x[0] for x in want])
    for n in (3, 65, 2):
        idx = [(7 * i + 2) % len(proofs) for i in range(n)]
        assert pin_res(h, [ios[i] for i in idx], [proofs[i] for i in idx]) == (0, [want[i][1] for i in idx], [want[i][0] for i in idx]), n
    # the other protocol's call refuses the handle, both ways
    assert g16_res(h, ios[:1], proofs[:1])[0] == ZK_ERR_HANDLE
    g1, g2 = P.g1_to_bytes(P.G1), P.g2_to_bytes(P.G2)
    rc, hg = g16_upload((bytes(576), g1, g2, g2))
    assert rc == 0 and pin_res(hg, ios[:1], proofs[:1])[0] == ZK_ERR_HANDLE
    assert free(hg) == 0 and free(h) == 0
    assert pin_res(h, ios[:1], proofs[:1])[0] == ZK_ERR_HANDLE


def test_pinocchio_bad_key_fails_the_upload_with_the_hosts_code(pinocchio_batch):
    vk1, vk2, ios, proofs, host = pinocchio_batch
    n_io = len(ios[0]) // 32
    bad_yt = bytearray(vk2); bad_yt[192 * 6 - 1] ^= 1
    bad_ww = bytes(vk2[:192 * 6]) + bytes([vk2[192 * 6] | 0x80]) + vk2[192 * 6 + 1:]
    bad_vv = vk1[:96 * (3 + n_io - 1)] + VM._g1_outside_subgroup() + vk1[96 * (3 + n_io):]
    tors_av = vk2[:192] + torsion(1, "torsion 13 + subgroup") + vk2[384:]
    tors_aw = vk1[:96] + torsion(0, "torsion 11") + vk1[192:]
    for k1, k2 in ((vk1, bytes(bad_yt)), (vk1, bad_ww), (bad_vv, vk2), (bad_vv, bad_ww), (vk1, tors_av), (tors_aw, vk2), (tors_aw, bad_ww)):
        want = VM.pin_host(k1, k2, ios[0], proofs[0])[0]
        assert want in (ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE)
        assert pin_upload(k1, k2, n_io) == (want, 0)


# ------------------------------------------------------------------------------------------------------------------ through the Python surface
def test_python_resident_keys_on_gpu_made_proofs():
    _lib.check(_lib.lib().zk_init(0))
    st = RC.fr_stream(0x5EED0078)
    rng = lambda: next(st)
    cs, _ = RC.iterated_cubic(16, 5)
    prover, _, vk = Groth16.generate(rng, cs)
    wits = [RC.iterated_cubic(16, x)[1] for x in (5, 6, 7)]
    proofs = [prover.prove_rs(w, next(st), next(st)) for w in wits]
    prover.close()
    ios = [[w[k] for k in range(cs.m) if not cs.mid[k]] for w in wits]
    changed = [type(p)(VM._another_point(p.a, 1), p.b, p.c) if i == 0 else p for i, p in enumerate(proofs)]
    with vk.resident() as rv:
        assert rv.verify_many(ios, proofs) == Groth16.verify_many(ios, vk, proofs) == [True] * 3
        assert rv.verify_many(ios, changed, return_status=True) == Groth16.verify_many(ios, vk, changed, return_status=True) == ([False, True, True], [0] * 3)
        assert rv.verify_many([], []) == []
        with pytest.raises(ValueError):
            rv.verify_many(ios[:2], proofs)
    with pytest.raises(ValueError):
        rv.verify_many(ios, proofs)                                  # closed
    for cls in (PIN.ZK, PIN.NonZK):
        pr, _, pvk = cls.generate(rng, cs)
        pp = [pr.prove(rng, w) for w in wits]
        pr.close()
        ch = [PIN.Proof(**dict(p.__dict__, **{f: VM._another_point(getattr(p, f), 2 if f in ("ww", "waww") else 1)})) for p, f in zip(pp, ("h", "ww", "bvwy"))]
        rv = pvk.resident()
        assert rv.verify_many(ios, pp) == cls.verify_many(ios, pvk, pp) == [True] * 3
        assert rv.verify_many(ios, ch, return_status=True) == cls.verify_many(ios, pvk, ch, return_status=True) == ([False] * 3, [0] * 3)
        rv.close()
        rv.close()                                                    # idempotent
