"""zk_groth16_verify_many / zk_pinocchio_verify_many (csrc/verify_resident.hip: a resident key that lives for one call) against the single-proof host
verifiers: keys and proofs made by the ORACLE, good and defective entries in one batch, and for every entry the `ok` and the status code that
zk_groth16_verify / zk_pinocchio_verify return for it alone.  Then the Python surface on proofs the GPU prover made in the same test."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from oracle import pyref as P
from zukelang_amd import _lib
from zukelang_amd import pinocchio as PIN
from zukelang_amd import r1cs as RC
from zukelang_amd.curve import G1, G2
from zukelang_amd.groth16 import Groth16

pytestmark = pytest.mark.gpu

R = P.R
ZK_OK, ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE, ZK_ERR_SCALAR_RANGE = 0, -1, -2, -3
frs = lambda xs: b"".join(P.fr_to_bytes(x) for x in xs)
csrs = lambda cs: [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
u8 = lambda b: C.cast(C.c_char_p(bytes(b)), _lib._P8) if len(b) else None


def _g1_outside_subgroup():
    x = 0
    while True:
        x += 1
        y2 = (x ** 3 + 4) % P.P
        y = pow(y2, (P.P + 1) // 4, P.P)
        if y * y % P.P == y2 and P.pt_mul((P.Fp1(x), P.Fp1(y)), R) is not None:
            return P.g1_to_bytes((P.Fp1(x), P.Fp1(y)))


def host_pairing(g1, g2):
    out = C.create_string_buffer(576)
    _lib.check(_lib.lib().zk_pairing_product(g1, g2, C.c_size_t(len(g1) // 96), out))
    return out.raw


# ------------------------------------------------------------------------------------------------------------------ Groth16
def g16_host(key, io, proof):
    """(status, ok) of zk_groth16_verify for one proof: the reference of every batch below."""
    ab, lt, gm, d = key
    ok = C.c_int(-1)
    rc = _lib.lib().zk_groth16_verify(ab, u8(lt), u8(io), C.c_size_t(len(lt) // 96), gm, d, proof, C.byref(ok))
    return rc, (ok.value if rc == 0 else 0)


def g16_many(key, ios, proofs, with_status=True):
    ab, lt, gm, d = key
    n = len(proofs)
    ok = (C.c_uint8 * n)(*([9] * n))
    st = (C.c_int32 * n)(*([9] * n))
    rc = _lib.lib().zk_groth16_verify_many(u8(ab), u8(lt), len(lt) // 96, u8(gm), u8(d), u8(b"".join(ios)), u8(b"".join(proofs)), n,
                                           C.cast(ok, _lib._P8), st if with_status else None)
    return rc, list(ok), list(st)


def g16_oracle(cs, witnesses, seed):
    """The oracle's key for `cs` and one oracle proof per witness, each with its own r and s."""
    st = P.fr_stream(seed)
    toxic = [next(st) for _ in range(5)]
    csr = csrs(cs)
    pk1, pk2, vk1, vk2 = O.QAP(cs.n, cs.m, *csr).groth16_setup(frs(toxic), cs.mid)
    key = (host_pairing(pk1[:96], pk2[:192]), vk1[96:], vk2[192:384], vk2[384:])          # ab = e(alpha, beta) | ltgm_io | gm | d
    proofs, ios = [], []
    for w in witnesses:
        r, s = next(st), next(st)
        proofs.append(b"".join(O.groth16_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), frs(toxic), P.fr_to_bytes(r), P.fr_to_bytes(s))))
        ios.append([w[k] for k in range(cs.m) if not cs.mid[k]])
    return key, ios, proofs


@pytest.fixture(scope="module")
def readme_batch():
    """The README circuit: 12 oracle proofs (witnesses x = 3 .. 14), 6 left intact and 6 defective, and what the host says about each."""
    wit = [RC.readme_circuit(x) for x in range(3, 15)]
    cs = wit[0][0]
    key, ios, proofs = g16_oracle(cs, [w for _, w in wit], 0x5EED0002)
    A, B, Cc = (lambda p: p[:96]), (lambda p: p[96:288]), (lambda p: p[288:])
    proofs[6] = A(proofs[6]) + B(proofs[6]) + P.g1_to_bytes(P.pt_mul(P.g1_from_bytes(Cc(proofs[6])), 2))          # another C
    proofs[7] = A(proofs[0]) + B(proofs[7]) + Cc(proofs[0])                                                        # A and C of another proof
    ios[8] = ios[8][:-1] + [(ios[8][-1] + 1) % R]                                                                  # a public input plus one
    off = bytearray(proofs[9]); off[287] ^= 1                                                                      # B off the curve
    proofs[9] = bytes(off)
    proofs[10] = _g1_outside_subgroup() + proofs[10][96:]                                                          # A outside the subgroup
    io_b = [frs(x) for x in ios]
    io_b[11] = io_b[11][:-32] + R.to_bytes(32, "little")                                                           # a public input equal to r
    host = [g16_host(key, io_b[i], proofs[i]) for i in range(12)]
    return key, io_b, proofs, host


def test_groth16_batch_matches_twelve_host_calls(readme_batch):
    key, ios, proofs, host = readme_batch
    assert [h[1] for h in host] == [1] * 6 + [0] * 6                                                               # the host sees what the batch was built to be
    assert [h[0] for h in host] == [0] * 9 + [ZK_ERR_NOT_ON_CURVE, ZK_ERR_NOT_ON_CURVE, ZK_ERR_SCALAR_RANGE]
    rc, ok, st = g16_many(key, ios, proofs)
    assert rc == 0 and ok == [h[1] for h in host] and st == [h[0] for h in host]
    rc, ok, st = g16_many(key, ios, proofs, with_status=False)
    assert rc == 0 and ok == [h[1] for h in host] and st == [9] * 12                                               # status == NULL: nothing written
    # one proof, and the batch in another order (a defective proof first)
    assert g16_many(key, ios[:1], proofs[:1]) == (0, [1], [0])
    rc, ok, st = g16_many(key, ios[::-1], proofs[::-1])
    assert rc == 0 and ok == [h[1] for h in host][::-1] and st == [h[0] for h in host][::-1]


def test_groth16_bad_key_fails_the_call_with_the_hosts_code(readme_batch):
    key, ios, proofs, host = readme_batch
    ab, lt, gm, d = key
    bad = bytearray(gm); bad[191] ^= 1
    for k2 in ((ab, lt, bytes(bad), d), (ab, lt, gm, bytes([gm[0] | 0x80]) + gm[1:]), (ab, _g1_outside_subgroup() + lt[96:], gm, d)):
        want = g16_host(k2, ios[0], proofs[0])[0]
        assert want in (ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE)
        assert g16_many(k2, ios, proofs)[0] == want
    # a malformed ab is compared on bytes, as on the host: no proof passes, no call fails
    k3 = (bytes(576), lt, gm, d)
    assert g16_host(k3, ios[0], proofs[0]) == (0, 0)
    rc, ok, st = g16_many(k3, ios, proofs)
    assert rc == 0 and ok == [0] * 12 and st == [h[0] for h in host]


@pytest.mark.parametrize("n_io", [0, 1])
def test_groth16_with_no_or_one_public_input(n_io):
    """e(A, B) = ab e(w T, gm) e(C, d) built from chosen exponents (no circuit has so few public values): A = [a] G1, B = [b] G2, C = [c] G1,
    d = [dd] G2, T = [t] G1, gm = [g] G2, ab = e(G1, G2)^(a b - w t g - c dd)."""
    a, b, c, dd, t, g, w = 11, 13, 17, 19, 23, 29, 31 if n_io else 0
    g1 = lambda k: P.g1_to_bytes(P.pt_mul(P.G1, k % R))
    g2 = lambda k: P.g2_to_bytes(P.pt_mul(P.G2, k % R))
    ab = host_pairing(g1(a * b - w * t * g - c * dd), g2(1))
    key = (ab, g1(t) * n_io, g2(g), g2(dd))
    io = frs([w] * n_io)
    proofs = [g1(a) + g2(b) + g1(c), g1(a) + g2(b) + g1(c + 1), g1(2 * a) + g2(b * pow(2, -1, R)) + g1(c)]
    ios = [io] * 3
    host = [g16_host(key, i, p) for i, p in zip(ios, proofs)]
    assert host == [(0, 1), (0, 0), (0, 1)]
    rc, ok, st = g16_many(key, ios, proofs)
    assert rc == 0 and ok == [1, 0, 1] and st == [0, 0, 0]


def test_groth16_with_seventy_four_public_inputs():
    """A random R1CS whose statement has 74 public values: one short product of 74 scalars per proof over the key's narrow table, a changed scalar in
    the middle of one and a scalar >= r at the end of another."""
    cs, w = RC.random_r1cs(48, 256, 4)
    assert int((cs.mid == 0).sum()) >= 70
    key, ios, proofs = g16_oracle(cs, [w, w, w], 0x5EED0074)
    io_b = [frs(x) for x in ios]
    io_b[1] = io_b[1][:32 * 40] + P.fr_to_bytes((ios[1][40] + 1) % R) + io_b[1][32 * 41:]
    io_b[2] = io_b[2][:32 * 73] + (R + 5).to_bytes(32, "little") + io_b[2][32 * 74:]
    host = [g16_host(key, io_b[i], proofs[i]) for i in range(3)]
    assert host == [(0, 1), (0, 0), (ZK_ERR_SCALAR_RANGE, 0)]
    rc, ok, st = g16_many(key, io_b, proofs)
    assert rc == 0 and ok == [1, 0, 0] and st == [0, 0, ZK_ERR_SCALAR_RANGE]


@pytest.mark.parametrize("n_io", [8192, 8193])
def test_groth16_with_as_many_public_inputs_as_one_narrow_table_holds_and_one_more(n_io):
    """The batched call takes any number of public inputs; a resident key refuses more than 8192 (tests/test_verify_resident_surface.py).  Built like
    the test above: ltgm_io[k] = [t] G1 below index 8192 and [t2] G1 from there on, w_k = k + 1, ab = e(G1, G2)^(a b - g sum_k w_k t_k - c dd): a sum
    that reads a wrong point or a wrong scalar is another sum.  ONE host call per size: the host's sum over 8193 points takes seconds."""
    a, b, c, dd, t, t2, g = 11, 13, 17, 19, 23, 37, 29
    g1 = lambda k: P.g1_to_bytes(P.pt_mul(P.G1, k % R))
    g2 = lambda k: P.g2_to_bytes(P.pt_mul(P.G2, k % R))
    w = [k + 1 for k in range(n_io)]
    dot = sum(wk * (t if k < 8192 else t2) for k, wk in enumerate(w))
    ab = host_pairing(g1(a * b - g * dot - c * dd), g2(1))
    key = (ab, g1(t) * min(n_io, 8192) + g1(t2) * (n_io - min(n_io, 8192)), g2(g), g2(dd))
    io = frs(w)
    good = g1(a) + g2(b) + g1(c)
    proofs = [good, g1(2 * a) + g2(b * pow(2, -1, R)) + g1(c), g1(a) + g2(b) + g1(c + 1), good]
    ios = [io, io, io, io[:-32] + R.to_bytes(32, "little")]
    assert g16_host(key, ios[0], proofs[0]) == (0, 1)
    rc, ok, st = g16_many(key, ios, proofs)
    assert rc == 0 and ok == [1, 1, 0, 0] and st == [0, 0, 0, ZK_ERR_SCALAR_RANGE]


# ------------------------------------------------------------------------------------------------------------------ Pinocchio
def pin_host(vk1, vk2, io, proof):
    ok = C.c_int(-1)
    rc = _lib.lib().zk_pinocchio_verify(vk1, vk2, u8(io), C.c_size_t(len(io) // 32), proof, C.byref(ok))
    return rc, (ok.value if rc == 0 else 0)


def pin_many(vk1, vk2, ios, proofs, with_status=True):
    n = len(proofs)
    ok = (C.c_uint8 * n)(*([9] * n))
    st = (C.c_int32 * n)(*([9] * n))
    rc = _lib.lib().zk_pinocchio_verify_many(u8(vk1), u8(vk2), len(ios[0]) // 32, u8(b"".join(ios)), u8(b"".join(proofs)), n, C.cast(ok, _lib._P8),
                                             st if with_status else None)
    return rc, list(ok), list(st)


@pytest.fixture(scope="module")
def pinocchio_batch():
    """iterated_cubic(6, x): the oracle's key and 9 oracle proofs -- 4 intact, 4 defective, and one honest proof whose delta_v is chosen with the
    trapdoor so that vio + vv is the identity (the sum the verifier forms before the divisibility check, pinocchio.ml:418-420)."""
    cs, _ = RC.iterated_cubic(6, 9)
    csr = csrs(cs)
    st = P.fr_stream(0x5EED0003)
    tox = [next(st) for _ in range(8)]
    toxic = frs(tox)
    ex = O.pinocchio_keygen_exponents(None, cs.n, cs.m, *csr, cs.mid, toxic, False)
    vk1, vk2 = O.points_of_exponents_g1(ex[2]), O.points_of_exponents_g2(ex[3])
    ios, proofs = [], []
    for x in range(9, 17):
        _, w = RC.iterated_cubic(6, x)
        dv, dw, dy = (P.fr_to_bytes(next(st)) for _ in range(3))
        proofs.append(O.pinocchio_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), toxic, dv, dw, dy))
        ios.append([w[k] for k in range(cs.m) if not cs.mid[k]])
    pt3 = lambda b: P.g1_to_bytes(P.pt_mul(P.g1_from_bytes(b), 3))
    proofs[4] = proofs[4][:384] + pt3(proofs[4][384:480]) + proofs[4][480:]                       # another h
    proofs[5] = proofs[5][:96] + proofs[0][96:288] + proofs[5][288:]                              # ww of another proof
    ios[6] = [(ios[6][0] + 1) % R] + ios[6][1:]                                                   # a public input changed
    off = bytearray(proofs[7]); off[383] ^= 1                                                     # yy off the curve
    proofs[7] = bytes(off)
    # vio + vv = O: the exponent of vio + vv is sum_k c_k rv v_k(s) + dv rv t(s); the oracle's exponent lists hold every term
    _, w = RC.iterated_cubic(6, 21)
    n_mid, n_io = int(cs.mid.sum()), cs.m - int(cs.mid.sum())
    e1 = [int.from_bytes(ex[0][32 * i:32 * i + 32], "little") for i in range(len(ex[0]) // 32)]
    v1 = [int.from_bytes(ex[2][32 * i:32 * i + 32], "little") for i in range(len(ex[2]) // 32)]
    mids = [k for k in range(cs.m) if cs.mid[k]]
    pub = [k for k in range(cs.m) if not cs.mid[k]]
    vt = e1[5 * n_mid + (cs.n + 1) + 2 * cs.m]                                                    # pk_g1 = vv | yy | vav | yay | bvwy | si | v_all | w_all | vt | ...
    total = (sum(w[k] * e1[i] for i, k in enumerate(mids)) + sum(w[k] * v1[3 + i] for i, k in enumerate(pub))) % R
    dv = (-total * pow(vt, -1, R)) % R
    proofs.append(O.pinocchio_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), toxic, P.fr_to_bytes(dv), P.fr_to_bytes(next(st)), P.fr_to_bytes(next(st))))
    ios.append([w[k] for k in pub])
    vio = P.msm([P.g1_from_bytes(vk1[96 * (3 + i):96 * (4 + i)]) for i in range(n_io)], ios[-1])
    assert P.pt_add(vio, P.g1_from_bytes(proofs[-1][:96])) is None                                # the sum IS the identity
    io_b = [frs(x) for x in ios]
    host = [pin_host(vk1, vk2, io_b[i], proofs[i]) for i in range(9)]
    return vk1, vk2, io_b, proofs, host


def test_pinocchio_batch_matches_the_host_calls(pinocchio_batch):
    vk1, vk2, ios, proofs, host = pinocchio_batch
    assert [h[1] for h in host] == [1, 1, 1, 1, 0, 0, 0, 0, 1]
    assert [h[0] for h in host] == [0] * 7 + [ZK_ERR_NOT_ON_CURVE, 0]
    rc, ok, st = pin_many(vk1, vk2, ios, proofs)
    assert rc == 0 and ok == [h[1] for h in host] and st == [h[0] for h in host]
    rc, ok, st = pin_many(vk1, vk2, ios, proofs, with_status=False)
    assert rc == 0 and ok == [h[1] for h in host] and st == [9] * 9
    # the statuses of a proof's points in the host's order: waww (G2) with a compression flag after a vavv outside the subgroup
    p = proofs[0]
    two = p[:480] + _g1_outside_subgroup() + bytes([p[576] | 0x80]) + p[577:]
    flag_first = p[:96] + bytes([p[96] | 0x80]) + p[97:384] + _g1_outside_subgroup() + p[480:]
    big = ios[0][:32] + (R + 1).to_bytes(32, "little")
    cases = [(ios[0], two), (ios[0], flag_first), (big, p), (big, two)]
    want = [pin_host(vk1, vk2, io, pr) for io, pr in cases]
    assert [w[0] for w in want] == [ZK_ERR_NOT_ON_CURVE, ZK_ERR_ARG, ZK_ERR_SCALAR_RANGE, ZK_ERR_NOT_ON_CURVE]
    rc, ok, st = pin_many(vk1, vk2, [c[0] for c in cases], [c[1] for c in cases])
    assert rc == 0 and ok == [0] * 4 and st == [w[0] for w in want]


def test_pinocchio_bad_key_fails_the_call_with_the_hosts_code(pinocchio_batch):
    vk1, vk2, ios, proofs, host = pinocchio_batch
    n_io = len(ios[0]) // 32
    bad_yt = bytearray(vk2); bad_yt[192 * 6 - 1] ^= 1                              # yt off the twist
    bad_ww = bytes(vk2[:192 * 6]) + bytes([vk2[192 * 6] | 0x80]) + vk2[192 * 6 + 1:]          # ww_io[0] with a compression flag ...
    bad_vv = vk1[:96 * (3 + n_io - 1)] + _g1_outside_subgroup() + vk1[96 * (3 + n_io):]       # ... against vv_io[n_io - 1] outside the subgroup: ww_io[0] is decoded first
    for k1, k2 in ((vk1, bytes(bad_yt)), (vk1, bad_ww), (bad_vv, vk2), (bad_vv, bad_ww)):
        want = pin_host(k1, k2, ios[0], proofs[0])[0]
        assert want in (ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE)
        assert pin_many(k1, k2, ios, proofs)[0] == want
    assert pin_host(bad_vv, bad_ww, ios[0], proofs[0])[0] == (ZK_ERR_ARG if n_io > 1 else ZK_ERR_NOT_ON_CURVE)


@pytest.mark.parametrize("n_io", [2, 8193])
def test_pinocchio_hand_built_with_two_and_with_8193_public_inputs(n_io):
    """tests/pinocchio_handbuilt.py: the sums over the public inputs in G1 AND in G2 over more points than one narrow table holds.  At two public inputs
    the host verifier is asked as well (tests/test_pairing_host.py holds the construction to it without a GPU); at 8193 the expected verdicts are the
    construction's: a host call would take three sums over 8193 points."""
    import pinocchio_handbuilt as H
    vk1, vk2 = H.key(n_io)
    w = H.public_inputs(n_io)
    good = H.proof(n_io)
    ios = [frs(w), frs(w[:-1] + [w[-1] + 1]), frs(w)]
    proofs = [good, good, H.ww_off_the_curve(good)]
    if n_io == 2:
        assert [pin_host(vk1, vk2, i, p) for i, p in zip(ios, proofs)] == [(0, 1), (0, 0), (ZK_ERR_NOT_ON_CURVE, 0)]
    rc, ok, st = pin_many(vk1, vk2, ios, proofs)
    assert rc == 0 and ok == [1, 0, 0] and st == [0, 0, ZK_ERR_NOT_ON_CURVE]


# ------------------------------------------------------------------------------------------------------------------ through the Python surface
def _another_point(b, group):
    """The encoding of another valid point of the same group: 2 P."""
    return P.g1_to_bytes(P.pt_mul(P.g1_from_bytes(bytes(b)), 2)) if group == 1 else P.g2_to_bytes(P.pt_mul(P.g2_from_bytes(bytes(b)), 2))


def test_python_verify_many_on_gpu_made_proofs():
    _lib.check(_lib.lib().zk_init(0))
    st = RC.fr_stream(0x5EED0077)
    rng = lambda: next(st)
    # Groth16
    cs, _ = RC.iterated_cubic(16, 5)
    prover, _, vk = Groth16.generate(rng, cs)
    wits = [RC.iterated_cubic(16, x)[1] for x in (5, 6, 7)]
    proofs = [prover.prove_rs(w, next(st), next(st)) for w in wits]
    prover.close()
    ios = [[w[k] for k in range(cs.m) if not cs.mid[k]] for w in wits]
    assert Groth16.verify_many(ios, vk, proofs) == [True] * 3
    assert Groth16.verify_many(ios, vk, proofs, return_status=True) == ([True] * 3, [0] * 3)
    assert [Groth16.verify(io, vk, p) for io, p in zip(ios, proofs)] == [True] * 3
    changed = [type(p)(_another_point(p.a, 1), p.b, p.c) if i == 0 else type(p)(p.a, _another_point(p.b, 2), p.c) if i == 1 else type(p)(p.a, p.b, _another_point(p.c, 1))
               for i, p in enumerate(proofs)]
    assert Groth16.verify_many(ios, vk, changed, return_status=True) == ([False] * 3, [0] * 3)
    # Pinocchio, both variants
    for cls in (PIN.ZK, PIN.NonZK):
        pr, _, pvk = cls.generate(rng, cs)
        pp = [pr.prove(rng, w) for w in wits]
        pr.close()
        assert cls.verify_many(ios, pvk, pp) == [True] * 3
        assert [cls.verify(io, pvk, p) for io, p in zip(ios, pp)] == [True] * 3
        ch = [PIN.Proof(**dict(p.__dict__, **{f: _another_point(getattr(p, f), 2 if f in ("ww", "waww") else 1)})) for p, f in zip(pp, ("h", "ww", "bvwy"))]
        assert cls.verify_many(ios, pvk, ch, return_status=True) == ([False] * 3, [0] * 3)
