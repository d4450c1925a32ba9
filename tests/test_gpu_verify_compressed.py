"""zk_*_verify_resident_compressed / zk_*_verify_folded_compressed (csrc/verify_resident.hip): proofs in the reference's wire form, decompressed on the
device in the call that verifies them.  The batches are built as tests/test_gpu_verify_resident.py builds its own -- README circuit, oracle proofs --
then compressed with pyref.g1/g2_compress and spoiled one proof at a time.  What is expected comes from the reference side alone: a proof's status is
the verdict of pyref's decoders on its points in the verifier's order, then the range of its public inputs; its `ok` is what the single-proof host
verifier says about the proof pyref decompressed."""
import ctypes as C
import json
import os

import pytest

from oracle import pyref as P
from zukelang_amd import _lib
from zukelang_amd import pinocchio as PIN
from zukelang_amd import r1cs as RC
from zukelang_amd.groth16 import Groth16
import test_gpu_verify_many as VM
from test_gpu_verify_many import pinocchio_batch          # noqa: F401  (the existing batch fixture)

pytestmark = pytest.mark.gpu

R, Pm = P.R, P.P
ZK_OK, ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE, ZK_ERR_SCALAR_RANGE = 0, -1, -2, -3
CODE = {P.OK: 0, P.BAD_ENCODING: ZK_ERR_ARG, P.NOT_ON_CURVE: ZK_ERR_NOT_ON_CURVE, P.NOT_IN_SUBGROUP: ZK_ERR_NOT_ON_CURVE}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORSION = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_points.json")))["points"]
u8, frs = VM.u8, VM.frs
# a proof's points in the order a verifier meets them: (offset in the wire form, group)
G16_WIRE = ((0, 1), (48, 2), (144, 1))
PIN_WIRE = ((0, 1), (48, 2), (144, 1), (192, 1), (240, 1), (288, 2), (384, 1), (432, 1))          # vv ww yy h vavv waww yayy bvwy
INF1 = bytes([0xC0]) + bytes(47)


def torsion_compressed(group, what):
    raw = bytes.fromhex(next(r["hex"] for r in TORSION if r["group"] == group and r["what"] == what))
    return P.g2_compress(P.g2_from_bytes(raw)) if group else P.g1_compress(P.g1_from_bytes(raw))


def compress(proof, wire):
    """an uncompressed proof of valid points -> its wire form"""
    out, off = [], 0
    for _, g in wire:
        size = 96 * g
        pt = proof[off:off + size]
        out.append(P.g1_compress(P.g1_from_bytes(pt)) if g == 1 else P.g2_compress(P.g2_from_bytes(pt)))
        off += size
    return b"".join(out)


def put(proof, wire, q, point):
    off, g = wire[q]
    assert len(point) == 48 * g
    return proof[:off] + point + proof[off + 48 * g:]


def get(proof, wire, q):
    off, g = wire[q]
    return proof[off:off + 48 * g]


flip = lambda pt, mask: bytes([pt[0] ^ mask]) + pt[1:]
X_IS_P = bytes([0x80 | (Pm >> 376)]) + Pm.to_bytes(48, "big")[1:]


def g1_off_curve():
    x = 0
    while True:
        x += 1
        s = bytes([0x80]) + x.to_bytes(47, "big")
        if P.g1_decompress(s)[0] == P.NOT_ON_CURVE:
            return s


def reference(wire, host, io, proof):
    """(status, ok, the decompressed proof or None) from pyref's decoders and the single-proof host verifier"""
    pts = []
    for off, g in wire:
        v, pt = (P.g1_decompress if g == 1 else P.g2_decompress)(proof[off:off + 48 * g])
        if v != P.OK:
            return CODE[v], 0, None
        pts.append(P.g1_to_bytes(pt) if g == 1 else P.g2_to_bytes(pt))
    plain = b"".join(pts)
    if any(int.from_bytes(io[32 * k:32 * k + 32], "little") >= R for k in range(len(io) // 32)):
        return ZK_ERR_SCALAR_RANGE, 0, plain
    rc, ok = host(io, plain)
    assert rc == 0
    return 0, ok, plain


def call(name, h, ios, proofs, with_status=True):
    n = len(proofs)
    ok = (C.c_uint8 * n)(*([9] * n))
    st = (C.c_int32 * n)(*([9] * n))
    rc = getattr(_lib.lib(), name)(h, u8(b"".join(ios)), u8(b"".join(proofs)), n, C.cast(ok, _lib._P8), st if with_status else None)
    return rc, list(ok), list(st)


def folded(name, h, ios, proofs, rho):
    n = len(proofs)
    all_ok = C.c_int(9)
    st = (C.c_int32 * n)(*([9] * n))
    rc = getattr(_lib.lib(), name)(h, u8(b"".join(ios)), u8(b"".join(proofs)), u8(rho), n, C.byref(all_ok), st)
    return rc, all_ok.value, list(st)


free = lambda h: _lib.lib().zk_vk_free(C.c_uint64(h))


def upload(fn, *args):
    h = C.c_uint64(0)
    assert getattr(_lib.lib(), fn)(*args, C.byref(h)) == 0 and h.value
    return h.value


def run_the_handle(res, res_c, h, ios, proofs, want):
    """what both protocols ask of one handle: the whole batch, the uncompressed twin on what decompresses, status = NULL, 3 / 65 / 2 proofs, and 8193"""
    st, ok = [w[0] for w in want], [w[1] for w in want]
    assert call(res_c, h, ios, proofs) == (0, ok, st)
    plain = [i for i, w in enumerate(want) if w[2] is not None]
    assert len(plain) >= 8
    assert call(res, h, [ios[i] for i in plain], [want[i][2] for i in plain]) == (0, [ok[i] for i in plain], [st[i] for i in plain])
    assert call(res_c, h, ios, proofs, with_status=False) == (0, ok, [9] * len(proofs))                       # status == NULL: nothing written
    n = len(proofs)
    for count in (3, 65, 2):                                                                                # the workspaces grow, then nothing is stale
        idx = [(5 * i + 1) % n for i in range(count)]
        assert call(res_c, h, [ios[i] for i in idx], [proofs[i] for i in idx]) == (0, [ok[i] for i in idx], [st[i] for i in idx]), count
    idx = [i % n for i in range(8193)]                                                                      # a slab of 8192, then a slab of one
    assert call(res_c, h, [ios[i] for i in idx], [proofs[i] for i in idx]) == (0, [ok[i] for i in idx], [st[i] for i in idx])
    o2 = (C.c_uint8 * 2)(7, 7)
    assert getattr(_lib.lib(), res_c)(h, None, None, 0, C.cast(o2, _lib._P8), None) == 0 and list(o2) == [7, 7]        # count = 0 touches nothing
    assert getattr(_lib.lib(), res_c)(h, u8(ios[0]), None, 1, C.cast(o2, _lib._P8), None) == ZK_ERR_ARG
    assert getattr(_lib.lib(), res_c)(h, None, u8(proofs[0]), 1, C.cast(o2, _lib._P8), None) == ZK_ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ Groth16
@pytest.fixture(scope="module")
def g16_batch():
    """The README circuit: 18 oracle proofs (x = 3 .. 20) in wire form, six intact and twelve spoiled one at a time, with the reference's view of each."""
    wit = [RC.readme_circuit(x) for x in range(3, 21)]
    cs = wit[0][0]
    key, ios, plain = VM.g16_oracle(cs, [w for _, w in wit], 0x5EED0C12)
    W = G16_WIRE
    pr = [compress(p, W) for p in plain]
    io_b = [frs(x) for x in ios]
    A, B, Cc = 0, 1, 2
    pr[1] = put(pr[1], W, A, flip(get(pr[1], W, A), 0x80))                                  # A: the compression bit cleared
    pr[3] = put(pr[3], W, A, X_IS_P)                                                        # A: x = p
    pr[4] = put(pr[4], W, B, bytes([0xC0]) + bytes(94) + b"\x01")                           # B: the infinity bit and a non-zero byte
    pr[6] = put(pr[6], W, A, g1_off_curve())                                                # A: an abscissa on no point of the curve
    pr[7] = put(pr[7], W, Cc, torsion_compressed(0, "torsion 11"))                          # C: on the curve, of order 11^k
    pr[8] = put(pr[8], W, B, torsion_compressed(1, "torsion 13"))                           # B: on the twist, of order 13^k
    pr[9] = put(pr[9], W, Cc, flip(get(pr[9], W, Cc), 0x20))                                # -C: a point of the group, a wrong proof
    pr[10] = put(put(pr[10], W, A, flip(get(pr[10], W, A), 0x20)), W, B, flip(get(pr[10], W, B), 0x20))       # e(-A, -B) = e(A, B)
    pr[11] = put(pr[11], W, A, INF1)                                                        # A the identity
    pr[12] = put(put(pr[12], W, A, g1_off_curve()), W, B, flip(get(pr[12], W, B), 0x80))    # A off the curve AND B badly encoded
    io_b[13] = io_b[13][:-32] + (R + 2).to_bytes(32, "little")                              # a public input >= r
    io_b[14] = io_b[14][:-32] + R.to_bytes(32, "little")                                    # ... together with a bad point
    pr[14] = put(pr[14], W, Cc, flip(get(pr[14], W, Cc), 0x80))
    io_b[15] = frs(ios[15][:-1] + [(ios[15][-1] + 1) % R])                                  # a wrong public input
    host = lambda io, proof: VM.g16_host(key, io, proof)
    want = [reference(W, host, io_b[i], pr[i]) for i in range(18)]
    return key, io_b, pr, want


def test_groth16_compressed_matches_the_reference_side(g16_batch):
    key, ios, proofs, want = g16_batch
    A, N, S = ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE, ZK_ERR_SCALAR_RANGE
    assert [w[0] for w in want] == [0, A, 0, A, A, 0, N, N, N, 0, 0, 0, N, S, A, 0, 0, 0]
    assert [w[1] for w in want] == [1, 0, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1]
    ab, lt, gm, d = key
    h = upload("zk_groth16_vk_upload", u8(ab), u8(lt), len(lt) // 96, u8(gm), u8(d))
    run_the_handle("zk_groth16_verify_resident", "zk_groth16_verify_resident_compressed", h, ios, proofs, want)
    assert free(h) == 0
    assert call("zk_groth16_verify_resident_compressed", h, ios, proofs)[0] == -7                            # a freed handle


def test_groth16_folded_compressed(g16_batch):
    key, ios, proofs, want = g16_batch
    ab, lt, gm, d = key
    h = upload("zk_groth16_vk_upload", u8(ab), u8(lt), len(lt) // 96, u8(gm), u8(d))
    good = [i for i, w in enumerate(want) if w[1] == 1]
    rho_of = lambda n: b"".join((0x9E3779B97F4A7C15F39CC0605CEDC835 * (i + 1) % (1 << 128) or 1).to_bytes(16, "little") for i in range(n))
    fc, fu = "zk_groth16_verify_folded_compressed", "zk_groth16_verify_folded"
    # three batches the uncompressed twin can take as well: all good | a wrong proof of valid points | a public input >= r
    for extra, all_ok in (([], 1), ([9], 0), ([13], 0)):
        idx = good[:3] + extra + good[3:]
        rho = rho_of(len(idx))
        got = folded(fc, h, [ios[i] for i in idx], [proofs[i] for i in idx], rho)
        assert got == (0, all_ok, [want[i][0] for i in idx]), extra
        assert got == folded(fu, h, [ios[i] for i in idx], [want[i][2] for i in idx], rho), extra
    # a point that does not decode: the statuses of the per-proof call
    idx = good[:2] + [12, 4] + good[2:]
    got = folded(fc, h, [ios[i] for i in idx], [proofs[i] for i in idx], rho_of(len(idx)))
    assert got == (0, 0, [want[i][0] for i in idx])
    assert got[2] == call("zk_groth16_verify_resident_compressed", h, [ios[i] for i in idx], [proofs[i] for i in idx])[2]
    # 8193 good proofs: the fold crosses a slab
    idx = [good[i % len(good)] for i in range(8193)]
    assert folded(fc, h, [ios[i] for i in idx], [proofs[i] for i in idx], rho_of(8193)) == (0, 1, [0] * 8193)
    assert free(h) == 0


# ------------------------------------------------------------------------------------------------------------------ Pinocchio
@pytest.fixture(scope="module")
def pin_batch(pinocchio_batch):
    """The fixture of tests/test_gpu_verify_many.py in wire form -- its five honest proofs, its two wrong proofs of valid points and its changed public
    input -- and copies of the honest ones spoiled in wire form, the last point (bvwy) and the second G2 point (waww) among them."""
    vk1, vk2, io_u, plain, _ = pinocchio_batch
    W = PIN_WIRE
    VV, WW, YY, H, VAVV, WAWW, YAYY, BVWY = range(8)
    keep = [0, 1, 2, 3, 8, 4, 5, 6]                                                          # 7 holds a point off the curve: no wire form
    pr = [compress(plain[i], W) for i in keep]
    io_b = [io_u[i] for i in keep]
    honest = lambda k: (pr[k % 5], io_b[k % 5])
    def add(k, fn, io_fn=None):
        p, io = honest(k)
        pr.append(fn(p))
        io_b.append(io_fn(io) if io_fn else io)
    add(0, lambda p: put(p, W, BVWY, flip(get(p, W, BVWY), 0x80)))                            # 8: bvwy, the compression bit cleared
    add(1, lambda p: put(p, W, WAWW, torsion_compressed(1, "torsion 23")))                    # 9: waww outside the subgroup
    add(2, lambda p: put(put(p, W, VV, g1_off_curve()), W, WW, flip(get(p, W, WW), 0x80)))    # 10: vv off the curve AND ww badly encoded
    add(3, lambda p: put(p, W, H, X_IS_P))                                                    # 11: h: x = p
    add(4, lambda p: p, lambda io: (R + 1).to_bytes(32, "little") + io[32:])                  # 12: a public input >= r
    add(0, lambda p: put(p, W, YAYY, torsion_compressed(0, "torsion 3")), lambda io: R.to_bytes(32, "little") + io[32:])          # 13: ... and a bad point
    add(1, lambda p: put(p, W, H, flip(get(p, W, H), 0x20)))                                  # 14: -h
    add(2, lambda p: put(p, W, VAVV, INF1))                                                   # 15: vavv the identity
    add(3, lambda p: put(p, W, WAWW, bytes([0xE0]) + bytes(95)))                              # 16: waww: the identity with a sign bit
    host = lambda io, proof: VM.pin_host(vk1, vk2, io, proof)
    want = [reference(W, host, io_b[i], pr[i]) for i in range(len(pr))]
    return vk1, vk2, io_b, pr, want


def test_pinocchio_compressed_matches_the_reference_side(pin_batch):
    vk1, vk2, ios, proofs, want = pin_batch
    A, N, S = ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE, ZK_ERR_SCALAR_RANGE
    assert [w[0] for w in want] == [0, 0, 0, 0, 0, 0, 0, 0, A, N, N, A, S, N, 0, 0, A]
    assert [w[1] for w in want] == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    h = upload("zk_pinocchio_vk_upload", u8(vk1), u8(vk2), len(ios[0]) // 32)
    run_the_handle("zk_pinocchio_verify_resident", "zk_pinocchio_verify_resident_compressed", h, ios, proofs, want)
    # the Groth16 call refuses a Pinocchio handle
    assert call("zk_groth16_verify_resident_compressed", h, ios[:1], [bytes(192)])[0] == -7
    assert free(h) == 0


def test_pinocchio_folded_compressed(pin_batch):
    vk1, vk2, ios, proofs, want = pin_batch
    h = upload("zk_pinocchio_vk_upload", u8(vk1), u8(vk2), len(ios[0]) // 32)
    good = [i for i, w in enumerate(want) if w[1] == 1]
    rho_of = lambda n: b"".join((0x9E3779B97F4A7C15F39CC0605CEDC835 * (i + 1) % (1 << 128) or 1).to_bytes(16, "little") for i in range(5 * n))
    fc, fu = "zk_pinocchio_verify_folded_compressed", "zk_pinocchio_verify_folded"
    for extra, all_ok in (([], 1), ([14], 0), ([12], 0)):
        idx = good[:3] + extra + good[3:]
        rho = rho_of(len(idx))
        got = folded(fc, h, [ios[i] for i in idx], [proofs[i] for i in idx], rho)
        assert got == (0, all_ok, [want[i][0] for i in idx]), extra
        assert got == folded(fu, h, [ios[i] for i in idx], [want[i][2] for i in idx], rho), extra
    idx = good[:2] + [8, 9] + good[2:]
    got = folded(fc, h, [ios[i] for i in idx], [proofs[i] for i in idx], rho_of(len(idx)))
    assert got == (0, 0, [want[i][0] for i in idx])
    assert got[2] == call("zk_pinocchio_verify_resident_compressed", h, [ios[i] for i in idx], [proofs[i] for i in idx])[2]
    idx = [good[i % len(good)] for i in range(8193)]
    assert folded(fc, h, [ios[i] for i in idx], [proofs[i] for i in idx], rho_of(8193)) == (0, 1, [0] * 8193)
    assert free(h) == 0


# ------------------------------------------------------------------------------------------------------------------ through the Python surface
def test_python_compressed_equals_uncompressed_on_gpu_made_proofs():
    _lib.check(_lib.lib().zk_init(0))
    st = RC.fr_stream(0x5EED0C77)
    rng = lambda: next(st)
    cs, _ = RC.iterated_cubic(16, 5)
    wits = [RC.iterated_cubic(16, x)[1] for x in (5, 6, 7)]
    ios = [[w[k] for k in range(cs.m) if not cs.mid[k]] for w in wits]
    prover, _, vk = Groth16.generate(rng, cs)
    proofs = [prover.prove_rs(w, next(st), next(st)) for w in wits]
    prover.close()
    proofs[1] = type(proofs[1])(proofs[1].a, proofs[1].b, VM._another_point(proofs[1].c, 1))
    with vk.resident() as rv:
        plain = rv.verify_many(ios, proofs, return_status=True)
        assert plain == ([True, False, True], [0] * 3)
        assert rv.verify_many(ios, proofs, return_status=True, compressed=True) == plain
        assert rv.verify_many(ios, [p.to_compressed() for p in proofs], return_status=True, compressed=True) == plain
        assert rv.verify_many(ios, proofs, fold_first=True, compressed=True) == plain[0]
        assert rv.verify_all(ios, proofs, compressed=True) is False
        assert rv.verify_all(ios[::2], proofs[::2], compressed=True) is True
    for cls in (PIN.ZK, PIN.NonZK):
        pr, _, pvk = cls.generate(rng, cs)
        pp = [pr.prove(rng, w) for w in wits]
        pr.close()
        pp[2] = PIN.Proof(**dict(pp[2].__dict__, bvwy=VM._another_point(pp[2].bvwy, 1)))
        with pvk.resident() as rv:
            plain = rv.verify_many(ios, pp, return_status=True)
            assert plain == ([True, True, False], [0] * 3)
            assert rv.verify_many(ios, pp, return_status=True, compressed=True) == plain
            assert rv.verify_many(ios, [p.to_compressed() for p in pp], return_status=True, compressed=True) == plain
            assert rv.verify_all(ios, pp, compressed=True) is False
            assert rv.verify_all(ios[:2], pp[:2], compressed=True) is True
