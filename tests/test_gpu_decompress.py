"""GPU parity of zk_g1/g2_decompress_batch (of_compressed_bytes_exn over a list, src/lib/zk/curve.ml:199-212) with the one-point host functions
zk_g1/g2_decompress -- which tests/test_wire.py and tests/test_pairing_host.py hold to the oracle -- on valid points of every shape (both signs,
the identity, multiples of the generator and hashed-looking points), on every kind of invalid encoding, and through zukelang_amd/wire.py on a key large
enough to take the batched path; and, like the host functions in tests/test_decoders.py, with the decoder oracle of oracle/pyref.py over the encoding
matrix of tests/encoding_cases.py.  (A y with a zero imaginary part belongs to no subgroup point that can be constructed here: that branch of the
sign rule, and both branches of the Fp2 square root, are held to the oracle by zk_selftest_sqrt in tests/test_gpu_field.py.)"""
import ctypes as C

import numpy as np
import pytest

import encoding_cases as E
import oracle_lib as O
from oracle import pyref as P
from zukelang_amd import _lib, r1cs as RC, wire
from zukelang_amd.curve import G1, G2

pytestmark = pytest.mark.gpu


def host_one(grp, comp):
    out = C.create_string_buffer(grp.POINT_BYTES)
    rc = getattr(_lib.lib(), "zk_g1_decompress" if grp is G1 else "zk_g2_decompress")(bytes(comp), out)
    return rc, out.raw


def batch(grp, comps):
    n = len(comps)
    out = np.zeros(n * grp.POINT_BYTES, dtype=np.uint8)
    buf = np.frombuffer(b"".join(comps), dtype=np.uint8)
    rc = getattr(_lib.lib(), "zk_g1_decompress_batch" if grp is G1 else "zk_g2_decompress_batch")(buf.ctypes.data_as(C.c_void_p), C.c_size_t(n), out.ctypes.data_as(C.c_void_p))
    return rc, bytes(out)


@pytest.mark.parametrize("grp,gen,mul", [(G1, O.g1_generator, O.g1_mul), (G2, O.g2_generator, O.g2_mul)])
def test_batch_decompression_equals_the_host_function(grp, gen, mul):
    _lib.check(_lib.lib().zk_init(0))
    st = P.fr_stream(0x5EEDDEC0 + grp.POINT_BYTES)
    ks = [1, 2, 3, P.R - 1, P.R - 2] + [next(st) for _ in range(600)]
    pts = grp.of_Fr(RC.fr_bytes(ks))                                  # s_i G on the fixed-base kernel: both signs of y occur
    B, Cb = grp.POINT_BYTES, grp.COMPRESSED_BYTES
    comps = [grp.to_compressed_bytes(pts[B * i:B * (i + 1)]) for i in range(len(ks))]
    inf = bytes([0xC0]) + bytes(Cb - 1)
    comps = comps[:300] + [inf] + comps[300:] + [inf]
    rc, out = batch(grp, comps)
    assert rc == 0
    for i, c in enumerate(comps):
        rc1, ref = host_one(grp, c)
        assert rc1 == 0 and out[B * i:B * (i + 1)] == ref, i
    want = bytes(pts[:B * 300]) + bytes([0x40]) + bytes(B - 1) + bytes(pts[B * 300:]) + bytes([0x40]) + bytes(B - 1)
    assert out == want                                                 # ... and both are the points that were compressed
    assert grp.of_compressed_bytes_many(b"".join(comps)) == want
    assert grp.of_compressed_bytes_many(b"") == b""


def _bad_cases(grp):
    Cb = grp.COMPRESSED_BYTES
    good = grp.to_compressed_bytes(grp.of_Fr(RC.fr_bytes([5])))
    no_flag = bytes([good[0] & 0x7F]) + good[1:]                       # compression bit missing
    big = bytes([0x80 | 0x1F]) + bytes([0xFF]) * (Cb - 1)              # coordinate >= p
    # an abscissa whose x^3 + b is not a square: search small x
    x = 0
    while True:
        x += 1
        cand = bytes([0x80]) + x.to_bytes(Cb - 1, "big")
        rc, _ = host_one(grp, cand)
        if rc != 0:
            off_curve = cand
            break
    # on the curve, outside the prime-order subgroup: the first small x with a square right-hand side that the host rejects for the subgroup
    x = 0
    outside = None
    while outside is None and x < 4000:
        x += 1
        cand = bytes([0x80]) + x.to_bytes(Cb - 1, "big")
        rc, _ = host_one(grp, cand)
        if rc != 0 and b"subgroup" in _lib.lib().zk_last_error():
            outside = cand
    return good, {"no_flag": no_flag, "coordinate >= p": big, "off the curve": off_curve, "outside the subgroup": outside}


@pytest.mark.parametrize("grp", [G1, G2])
def test_batch_decompression_rejects_what_the_host_function_rejects(grp):
    _lib.check(_lib.lib().zk_init(0))
    _lib.lib().zk_last_error.restype = C.c_char_p
    good, bad = _bad_cases(grp)
    assert bad["outside the subgroup"] is not None
    for what, c in bad.items():
        rc1, _ = host_one(grp, c)
        assert rc1 != 0, what
        for pos in (0, 7, 299):                                       # one bad point anywhere in a list fails the list with the host's code
            comps = [good] * 300
            comps[pos] = c
            rc, _ = batch(grp, comps)
            assert rc == rc1, (what, pos, rc, rc1)
    rc, _ = batch(grp, [good] * 300)
    assert rc == 0


def test_a_key_in_the_reference_json_is_read_through_the_batched_path():
    """wire.groth16_pkey_of_json / pinocchio_pkey_of_json on keys of a few thousand points (above wire.BATCH_MIN): the points come back exactly."""
    from zukelang_amd.groth16 import Groth16
    from zukelang_amd import pinocchio as PIN
    cs, w = RC.iterated_cubic(600, 0xBEEF)
    st = P.fr_stream(0x5EEDDEC1)
    pk, _ = Groth16.keygen(lambda: next(st), cs)
    mids = [k for k in range(cs.m) if cs.mid[k]]
    mid_vars = [("v%d" % k, k) for k in mids]
    data = wire.groth16_pkey_to_json(pk, cs.n, mid_vars)
    back, mv = wire.groth16_pkey_of_json(data)
    assert bytes(back.g1) == bytes(pk.g1) and bytes(back.g2) == bytes(pk.g2) and mv == mid_vars
    assert len(pk.g1) // 96 > wire.BATCH_MIN and len(pk.g2) // 192 > wire.BATCH_MIN
    ppk, _ = PIN.ZK.keygen(lambda: next(st), cs)
    all_vars = [("v%d" % k, k) for k in range(cs.m)]
    pdata = wire.pinocchio_pkey_to_json(ppk, cs.n, mid_vars, all_vars)
    pback, n, mv, av = wire.pinocchio_pkey_of_json(pdata)
    assert bytes(pback.g1) == bytes(ppk.g1) and bytes(pback.g2) == bytes(ppk.g2) and n == cs.n and mv == mid_vars and av == all_vars


WANT = {P.OK: 0, P.BAD_ENCODING: -1, P.NOT_ON_CURVE: -2, P.NOT_IN_SUBGROUP: -2}


@pytest.mark.parametrize("grp,group", [(G1, 1), (G2, 2)])
def test_batch_decompression_agrees_with_the_oracle_on_the_encoding_matrix(grp, group):
    """The compressed half of the matrix through zk_g1/g2_decompress_batch: the strings the oracle accepts as ONE list (its points, byte for byte), every
    string it refuses at positions 0, 130 and 299 of a list of 300 valid points (three workgroups of 128 lanes) with the oracle's verdict as the status."""
    _lib.check(_lib.lib().zk_init(0))
    rows = E.matrix(group, True)
    ok = [(c, pt) for c, v, pt in rows if v == P.OK]
    bad = [(c, v) for c, v, _ in rows if v != P.OK]
    assert len(ok) > 128 and {v for _, v in bad} == {P.BAD_ENCODING, P.NOT_ON_CURVE, P.NOT_IN_SUBGROUP}
    rc, out = batch(grp, [c.data for c, _ in ok])
    assert rc == 0 and out == b"".join(pt for _, pt in ok)
    filler = [c.data for c, _ in ok][1:] * 3                              # valid points, not all alike
    wrong = []
    for c, v in bad:
        for pos in (0, 130, 299):
            comps = filler[:300]
            comps[pos] = c.data
            rc, _ = batch(grp, comps)
            if rc != WANT[v]:
                wrong.append((c.label, c.data.hex(), pos, v, rc))
    assert not wrong, "%d lists with a status other than the oracle's verdict: %r" % (len(wrong), wrong[:6])


@pytest.mark.parametrize("grp,group", [(G1, 1), (G2, 2)])
def test_a_list_fails_with_the_status_of_its_first_bad_element(grp, group):
    """zukelang_amd/wire.py promises the same checks and the same error below and above BATCH_MIN; below it the elements are decoded one by one, in list
    order.  Two bad elements of different kinds in one list, in both orders, at (5, 290) (different workgroups) and (140, 141) (neighbouring lanes): the
    batch's status and its message's kind are the one-point function's on the EARLIER element."""
    _lib.check(_lib.lib().zk_init(0))
    _lib.lib().zk_last_error.restype = C.c_char_p
    rows = E.matrix(group, True)
    filler = [c.data for c, v, _ in rows if v == P.OK][1:] * 3
    pick = {}
    for c, v, _ in rows:
        if v != P.OK and c.kind in ("flags", "curve"):
            pick.setdefault(v, c.data)
    assert set(pick) == {P.BAD_ENCODING, P.NOT_ON_CURVE, P.NOT_IN_SUBGROUP}
    kind_of = lambda: "subgroup" if b"subgroup" in _lib.lib().zk_last_error() else ("curve" if b"not on the curve" in _lib.lib().zk_last_error() else "encoding")
    tried = 0
    for va, a in pick.items():
        for vb, b in pick.items():
            if va == vb:
                continue
            for pa, pb in ((5, 290), (140, 141)):
                comps = filler[:300]
                comps[pa], comps[pb] = a, b
                rc1, _ = host_one(grp, a)
                k1 = kind_of()
                rc, _ = batch(grp, comps)
                assert (rc, kind_of()) == (rc1, k1) and rc == WANT[va], (va, vb, pa, pb, rc, rc1)
                tried += 1
    assert tried == 12


def test_a_large_key_record_with_a_bad_point_string_raises_the_same_error_as_a_small_one():
    """The readers on a key of more than wire.BATCH_MIN points per group (lists decoded on the GPU): wrong lengths and malformed identities in the first,
    a middle and the last point field raise ValueError of the same class as in the small golden records of tests/test_decoders.py."""
    from zukelang_amd.groth16 import Groth16
    cs, w = RC.iterated_cubic(300, 0xBEE5)
    st = P.fr_stream(0x5EEDDEC2)
    pk, _ = Groth16.keygen(lambda: next(st), cs)
    assert len(pk.g1) // 96 > wire.BATCH_MIN and len(pk.g2) // 192 > wire.BATCH_MIN
    mid_vars = [("v%d" % k, k) for k in range(cs.m) if cs.mid[k]]
    record = wire.groth16_pkey_to_json(pk, cs.n, mid_vars)
    assert E.check_reader_refuses_bad_point_strings(wire, wire.groth16_pkey_of_json, record) == 6 * len(E.bad_point_strings(1))
