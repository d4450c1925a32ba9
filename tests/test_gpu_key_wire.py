"""Proving keys and MSM bases from their compressed wire bytes (include/zkmi355x.h, "keys and base lists in WIRE form"): a handle made by
zk_groth16_pk_upload_compressed / zk_pinocchio_pk_upload_compressed / zk_bases_upload_compressed cannot be told apart from the one the uncompressed
upload makes from the same points -- pool bytes, proof bytes (which equal the oracle's), derivation, resident products, on one device and on a device
list -- and a list with a bad point is refused with pyref's verdict on its FIRST bad point (oracle/pyref.py g1/g2_decompress over
tests/encoding_cases.py and tests/golden/torsion_points.json).  zk_*_pool_points_compressed is the host compression of zk_*_pool_points, and with the
uploads it closes the key-cache round trip (derive once, store compressed, reload)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import encoding_cases as E
import oracle_lib as O
from oracle import pyref as P
from zukelang_amd import _lib, r1cs as RC
from zukelang_amd import pinocchio as PIN
from zukelang_amd.curve import G1, G2
from zukelang_amd.groth16 import Groth16

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CODE = {P.OK: 0, P.BAD_ENCODING: -1, P.NOT_ON_CURVE: -2, P.NOT_IN_SUBGROUP: -2}          # ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE (twice)

CIRCUITS = {
    "readme": lambda: RC.readme_circuit(3),
    "n5": lambda: RC.random_r1cs(5, 12, 3, nnz=(1, 3)),                      # no power of two, pools of a few points, one variable in no row
    "n301": lambda: RC.random_r1cs(301, 331, 5, nnz=(1, 4), unused=0),       # every pool of both protocols and both forms: > 2 x 128 points, no multiple of 128
    "unused": lambda: RC.random_r1cs(24, 40, 77),                            # m // 8 variables occur in no row: identity key points
}


def frs(xs):
    return b"".join(P.fr_to_bytes(x) for x in xs)


def csrs(cs):
    return [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]


def w1(b):
    return G1.to_compressed_bytes_many(bytes(b))


def w2(b):
    return G2.to_compressed_bytes_many(bytes(b))


def set_option(name, value):
    _lib.check(_lib.lib().zk_set_option(name.encode(), None if value is None else str(value).encode()))


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def put(wire, size, idx, data):
    out = bytearray(wire)
    out[size * idx:size * (idx + 1)] = data
    return bytes(out)


@pytest.fixture(autouse=True)
def _init_and_leave_nothing_behind():
    _lib.check(_lib.lib().zk_init(0))
    yield
    _lib.set_device_list([0])          # ZK_ERR_ARG while any key handle is alive: live_key_handles() is back at 0 after every test


_G16 = {}


def g16_key(name):
    """(circuit, witness, toxic, key with both forms): once per process"""
    if name not in _G16:
        cs, w = CIRCUITS[name]()
        st = P.fr_stream(0xC0A1 + len(name))
        tox = [next(st) for _ in range(5)]
        it = iter(tox)
        pk, _ = Groth16.keygen(lambda: next(it), cs, lagrange=True)
        _G16[name] = (cs, w, tox, pk)
    return _G16[name]


_PIN = {}


def pin_key(name):
    if name not in _PIN:
        cs, w = CIRCUITS[name]()
        st = P.fr_stream(0xC0A2 + len(name))
        tox = [next(st) for _ in range(8)]
        it = iter(tox)
        pk, _ = PIN.ZK.keygen(lambda: next(it), cs)
        _PIN[name] = (cs, w, tox, pk)
    return _PIN[name]


def g16_pools(p):
    return [bytes(p.pool_points(g)) for g in (1, 2)]


def pin_pools(p):
    return [bytes(p.pool_points(i)) for i in range(8)]


def abc(proof):
    return (proof.a, proof.b, proof.c)


# ------------------------------------------------------------------------------------------------------------------ Groth16
@pytest.mark.parametrize("name", ["readme", "n5", "n301", "unused"])
def test_groth16_handle_from_wire_bytes_is_the_uncompressed_handle(name):
    cs, w, tox, pk = g16_key(name)
    if name == "unused":          # the key holds identity points: they travel as C0 00 .. 00
        assert IDENT48 in [w1(pk.g1)[48 * i:48 * i + 48] for i in range(len(pk.g1) // 96)]
    rs = [(11, 13), (P.R - 1, 0)]
    exp = [O.groth16_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, frs(w), frs(tox), P.fr_to_bytes(r), P.fr_to_bytes(s)) for r, s in rs]
    if cs.n <= 24:          # the literal restatement of groth16.ml:116-161 on the key's own points
        q = O.QAP(cs.n, cs.m, *csrs(cs))
        rc, *lit = q.groth16_prove(bytes(pk.g1), bytes(pk.g2), cs.mid, frs(w), P.fr_to_bytes(rs[0][0]), P.fr_to_bytes(rs[0][1]), True)
        assert rc == 0 and tuple(lit) == exp[0]
    ref, got = Groth16(cs, pk), Groth16.from_compressed(cs, w1(pk.g1), w2(pk.g2))
    assert g16_pools(got) == g16_pools(ref) == [bytes(pk.g1), bytes(pk.g2)]
    for (r, s), e in zip(rs, exp):
        assert abc(got.prove_rs(w, r, s)) == abc(ref.prove_rs(w, r, s)) == e
    # the Lagrange form handed in
    refl, gotl = Groth16(cs, pk, lagrange=True), Groth16.from_compressed(cs, w1(pk.lag_g1), w2(pk.lag_g2), lagrange=True)
    assert g16_pools(gotl) == g16_pools(refl) == [bytes(pk.lag_g1), bytes(pk.lag_g2)]
    assert abc(gotl.prove_rs(w, *rs[0])) == exp[0]
    # ... and derived on the device from a compressed-uploaded key: the pools and proofs of the uncompressed key after ITS derivation
    got.derive_lagrange()
    ref.derive_lagrange()
    derived = g16_pools(got)
    assert derived == g16_pools(ref) == [bytes(pk.lag_g1), bytes(pk.lag_g2)]
    assert abc(got.prove_rs(w, *rs[1])) == exp[1]
    # round trip: the derived pools in wire form = the host compression of the pools, point by point; uploaded again they are the same key
    stored = [bytes(got.pool_points(g, compressed=True)) for g in (1, 2)]
    assert stored == [w1(derived[0]), w2(derived[1])]
    for i in range(len(derived[0]) // 96):          # ... and zk_g1_compress itself, one point at a time (the identity included)
        assert stored[0][48 * i:48 * i + 48] == G1.to_compressed_bytes(derived[0][96 * i:96 * i + 96])
    for i in range(len(derived[1]) // 192):
        assert stored[1][96 * i:96 * i + 96] == G2.to_compressed_bytes(derived[1][192 * i:192 * i + 192])
    again = Groth16.from_compressed(cs, stored[0], stored[1], lagrange=True)
    assert g16_pools(again) == derived
    assert [abc(again.prove_rs(w, r, s)) for r, s in rs] == exp
    for p in (ref, got, refl, gotl, again):
        p.close()


IDENT48 = bytes([0xC0]) + bytes(47)


# ------------------------------------------------------------------------------------------------------------------ Pinocchio
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", ["readme", "n5", "n301", "unused"])
def test_pinocchio_handle_from_wire_bytes_is_the_uncompressed_handle(name, compact):
    cs, w, tox, pk = pin_key(name)
    ds = [(3, 5, 7), (0, 0, 0)]
    exp = [O.pinocchio_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, frs(w), frs(tox), *(P.fr_to_bytes(x) for x in d)) for d in ds]
    if cs.n <= 24:          # the literal restatement of pinocchio.ml:427-514 on the key's own points
        rc, lit = O.pinocchio_prove(O.QAP(cs.n, cs.m, *csrs(cs)), bytes(pk.g1), bytes(pk.g2), cs.mid, frs(w), *(P.fr_to_bytes(x) for x in ds[0]))
        assert rc == 0 and lit == exp[0]
    if not compact:
        set_option("ZK_PIN_COMPACT_H", 0)
    try:
        ref, got = PIN.ZK(cs, pk), PIN.ZK.from_compressed(cs, w1(pk.g1), w2(pk.g2))
        # the same pools, the h pool in the same form (compact: the upload's check admitted v_all | w_all on si -- the digest of the WIRE bytes seeds it here)
        assert got.pool_size(5) == ref.pool_size(5) == (cs.n + 1 if compact else cs.n + 1 + 2 * cs.m)
        assert pin_pools(got) == pin_pools(ref)
        for d, e in zip(ds, exp):
            assert got.prove_with(w, *d).to_bytes() == ref.prove_with(w, *d).to_bytes() == e
        got.derive_lagrange()
        ref.derive_lagrange()
        derived = pin_pools(got)
        assert derived == pin_pools(ref)
        assert got.prove_with(w, *ds[0]).to_bytes() == exp[0]
        # round trip: every pool in wire form = the host compression; the first n points of pool 5 are the h bases the key can be reloaded with
        for i in range(8):
            assert bytes(got.pool_points(i, compressed=True)) == (w1 if i < 6 else w2)(derived[i]), i
        hl = bytes(got.pool_points(5, compressed=True))[:48 * cs.n]
        again = PIN.ZK.from_compressed(cs, w1(pk.g1), w2(pk.g2), h_lagrange=hl)
        refl = PIN.ZK.from_lagrange(cs, pk, np.frombuffer(derived[5][:96 * cs.n], dtype=np.uint8))
        assert pin_pools(again) == pin_pools(refl) == derived
        assert [again.prove_with(w, *d).to_bytes() for d in ds] == exp
        for p in (ref, got, again, refl):
            p.close()
    finally:
        set_option("ZK_PIN_COMPACT_H", None)


# ------------------------------------------------------------------------------------------------------------------ resident bases
@pytest.mark.parametrize("n", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("grp", [G1, G2])
def test_resident_bases_from_wire_bytes_multiply_like_the_uncompressed_ones(grp, n):
    exps = [((i * 7919) % 13) * (0x1234567 + i) % P.R for i in range(n)]          # every 13th point is the identity
    pts = bytes(grp.of_Fr(RC.fr_bytes(exps)))
    wire = grp.to_compressed_bytes_many(pts)
    st = P.fr_stream(0xBA5E + n)
    with grp.resident(pts) as ref, grp.resident_compressed(wire) as got:
        assert (got.n, got.short_max) == (ref.n, ref.short_max) == (n, ref.short_max)
        full = RC.fr_bytes([next(st) for _ in range(n)])
        assert bytes(got.apply_powers(full)) == bytes(ref.apply_powers(full)) == bytes(grp.apply_powers(full, pts))          # the Pippenger chain
        lens = sorted({1, min(n, 2), min(n, int(ref.short_max)), max(1, n // 2), n})
        assert min(lens) <= ref.short_max          # the short path: two or more products of at most short_max scalars in ONE call
        many = [RC.fr_bytes([next(st) for _ in range(k)]) for k in lens] + [b""]
        a, b = got.apply_powers_many(many), ref.apply_powers_many(many)
        assert [bytes(x) for x in a] == [bytes(x) for x in b]
        if n > 1:          # nscalars < n: the first nscalars points
            part = RC.fr_bytes([next(st) for _ in range(n - 1)])
            assert bytes(got.apply_powers(part)) == bytes(ref.apply_powers(part)) == bytes(grp.apply_powers(part, pts[:grp.POINT_BYTES * (n - 1)]))


# ------------------------------------------------------------------------------------------------------------------ rejections
def torsion(group):
    """(compressed bytes, status) of every point of tests/golden/torsion_points.json in this group: on the curve, most outside the subgroup"""
    out = []
    for t in json.load(open(os.path.join(GOLDEN, "torsion_points.json")))["points"]:
        if t["group"] == group - 1:
            raw = bytes.fromhex(t["hex"])
            comp = (w1 if group == 1 else w2)(raw)
            v = (P.g1_decompress if group == 1 else P.g2_decompress)(comp)[0]
            assert (v == P.NOT_IN_SUBGROUP) == (t["verdict"] == 4) and v in (P.OK, P.NOT_IN_SUBGROUP), t["what"]
            out.append((comp, CODE[v]))
    assert any(rc == -2 for _, rc in out)
    return out


def good_list(group, n=300):
    grp = G1 if group == 1 else G2
    return grp.to_compressed_bytes_many(bytes(grp.of_Fr(RC.fr_bytes(list(range(1, n + 1))))))


def bases_upload(group, wire):
    h = C.c_uint64(0)
    a = np.frombuffer(wire, dtype=np.uint8)
    rc = _lib.lib().zk_bases_upload_compressed(C.c_int(group - 1), _p(a), C.c_size_t(len(wire) // (48 * group)), C.byref(h))
    if rc == 0:
        _lib.check(_lib.lib().zk_bases_free(h))
    else:
        assert h.value == 0
    return rc


@pytest.mark.parametrize("kind", ["flags", "range", "curve", "torsion"])
@pytest.mark.parametrize("group", [1, 2])
def test_a_bad_point_anywhere_in_a_list_gives_pyrefs_verdict(group, kind):
    size = 48 * group
    good = good_list(group)
    if kind == "torsion":
        rows = torsion(group)
    else:
        rows = [(c.data, CODE[v]) for c, v, _ in E.matrix(group, True) if c.kind == kind]
        assert rows and all(rc != 0 for _, rc in rows)
    for data, rc in rows:
        for idx in (0, 128, 299):
            assert bases_upload(group, put(good, size, idx, data)) == rc, (data.hex(), idx)
    assert bases_upload(group, good) == 0


@pytest.mark.parametrize("group", [1, 2])
def test_the_first_bad_point_decides_and_zero_bytes_are_no_identity(group):
    size = 48 * group
    good = good_list(group)
    by = {}
    for c, v, _ in E.matrix(group, True):
        if c.kind != "valid":
            by.setdefault(v, c.data)
    enc, cur, sub = by[P.BAD_ENCODING], by[P.NOT_ON_CURVE], by[P.NOT_IN_SUBGROUP]
    assert bases_upload(group, put(put(good, size, 5, cur), size, 200, enc)) == -2          # the earlier one, whatever its kind
    assert bases_upload(group, put(put(good, size, 5, enc), size, 200, cur)) == -1
    assert bases_upload(group, put(put(good, size, 130, sub), size, 131, enc)) == -2
    assert bases_upload(group, put(put(good, size, 129, enc), size, 131, sub)) == -1
    # the uncompressed uploads take 96 / 192 zero bytes for the identity; on the wire the string has no compression flag
    grp = G1 if group == 1 else G2
    pts = bytearray(bytes(grp.of_Fr(RC.fr_bytes([1, 2, 3]))))
    pts[2 * size:4 * size] = bytes(2 * size)
    grp.resident(bytes(pts)).close()
    assert bases_upload(group, put(good, size, 7, bytes(size))) == -1
    assert bases_upload(group, put(good, size, 7, bytes([0xC0]) + bytes(size - 1))) == 0          # THE identity
    with pytest.raises(ValueError, match="wire: bad point .*error -1"):
        grp.resident_compressed(put(good, size, 7, bytes(size)))


def _refused(fn, code):
    with pytest.raises(ValueError, match="wire: bad point") as e:
        fn()
    assert "error %d:" % code in str(e.value), str(e.value)


def _three_kinds():
    out = {}
    for group in (1, 2):
        by = {}
        for c, v, _ in E.matrix(group, True):
            if c.kind != "valid":
                by.setdefault(v, c.data)
        out[group] = [(by[P.BAD_ENCODING], -1), (by[P.NOT_ON_CURVE], -2), (by[P.NOT_IN_SUBGROUP], -2), (bytes(48 * group), -1)]
    return out


def test_groth16_keys_with_a_bad_point_are_refused_with_its_verdict():
    cs, w, tox, pk = g16_key("n301")
    kinds = _three_kinds()
    for lag in (False, True):
        g1, g2 = (w1(pk.lag_g1), w2(pk.lag_g2)) if lag else (w1(pk.g1), w2(pk.g2))
        for data, rc in kinds[1]:
            for idx in (0, 128, len(g1) // 48 - 1):
                _refused(lambda: Groth16.from_compressed(cs, put(g1, 48, idx, data), g2, lagrange=lag), rc)
        for data, rc in kinds[2]:          # a bad G2 point behind a good G1 list gives its own code
            for idx in (0, 128, len(g2) // 96 - 1):
                _refused(lambda: Groth16.from_compressed(cs, g1, put(g2, 96, idx, data), lagrange=lag), rc)
    # G1 before G2: an off-curve point at the END of the G1 list against a bad encoding at the START of the G2 list
    g1, g2 = w1(pk.g1), w2(pk.g2)
    _refused(lambda: Groth16.from_compressed(cs, put(g1, 48, len(g1) // 48 - 1, kinds[1][1][0]), put(g2, 96, 0, kinds[2][0][0])), -2)
    _refused(lambda: Groth16.from_compressed(cs, put(g1, 48, len(g1) // 48 - 1, kinds[1][0][0]), put(g2, 96, 0, kinds[2][1][0])), -1)
    # a wrong length stays what it was: ZK_ERR_DOMAIN, no point error
    with pytest.raises(_lib.ZkError) as e:
        Groth16.from_compressed(cs, g1[48:], g2)
    assert e.value.code == -8


def test_pinocchio_keys_with_a_bad_point_are_refused_with_its_verdict():
    cs, w, tox, pk = pin_key("n301")
    kinds = _three_kinds()
    g1, g2 = w1(pk.g1), w2(pk.g2)
    nm = int(np.count_nonzero(cs.mid))
    assert nm > 128
    for data, rc in kinds[1]:
        for idx in (0, 128, len(g1) // 48 - 1):
            _refused(lambda: PIN.ZK.from_compressed(cs, put(g1, 48, idx, data), g2), rc)
    for data, rc in kinds[2]:          # ww, waw and the two appended points are the G2 points the key keeps
        for idx in (0, 128, len(g2) // 96 - 1):
            _refused(lambda: PIN.ZK.from_compressed(cs, g1, put(g2, 96, idx, data)), rc)
    # order: the G1 list (a LATE point of it: the appended vt .. ybt, which the pools regroup) before the G2 list before h_lagrange
    last1 = len(g1) // 48 - 1
    _refused(lambda: PIN.ZK.from_compressed(cs, put(g1, 48, last1, kinds[1][1][0]), put(g2, 96, 0, kinds[2][0][0])), -2)
    _refused(lambda: PIN.ZK.from_compressed(cs, put(put(g1, 48, last1, kinds[1][0][0]), 48, 3, kinds[1][1][0]), g2), -2)          # index 3 (pool 0) before the last (pool 4)
    # vt is point last1 - 6 of the list but the LAST point of pool 0, which is built first; yy[0], point nm of the list, lies in pool 1: the list's order decides
    _refused(lambda: PIN.ZK.from_compressed(cs, put(put(g1, 48, last1 - 6, kinds[1][0][0]), 48, nm, kinds[1][1][0]), g2), -2)
    ref = PIN.ZK(cs, pk)
    ref.derive_lagrange()
    hl = w1(bytes(ref.pool_points(5))[:96 * cs.n])
    ref.close()
    for data, rc in kinds[1]:
        for idx in (0, 128, cs.n - 1):
            _refused(lambda: PIN.ZK.from_compressed(cs, g1, g2, h_lagrange=put(hl, 48, idx, data)), rc)
    _refused(lambda: PIN.ZK.from_compressed(cs, g1, put(g2, 96, 1, kinds[2][1][0]), h_lagrange=put(hl, 48, 0, kinds[1][0][0])), -2)
    PIN.ZK.from_compressed(cs, g1, g2, h_lagrange=hl).close()


# ------------------------------------------------------------------------------------------------------------------ ZK_KEY_SUBGROUP_CHECK=0
def test_without_the_subgroup_check_a_torsion_point_enters_the_pool():
    cs, w, tox, pk = g16_key("n5")
    g1, g2 = w1(pk.g1), w2(pk.g2)
    t1 = next(c for c, rc in torsion(1) if rc == -2)
    t2 = next(c for c, rc in torsion(2) if rc == -2)
    last1, last2 = len(g1) // 48 - 1, len(g2) // 96 - 1
    bad1, bad2 = put(g1, 48, last1, t1), put(g2, 96, last2, t2)
    _refused(lambda: Groth16.from_compressed(cs, bad1, bad2), -2)
    set_option("ZK_KEY_SUBGROUP_CHECK", 0)
    try:
        p = Groth16.from_compressed(cs, bad1, bad2)
        pools = g16_pools(p)
        assert bytes(p.pool_points(1, compressed=True)) == bad1 and bytes(p.pool_points(2, compressed=True)) == bad2
        p.close()
        assert bases_upload(1, put(good_list(1), 48, 128, t1)) == 0
        assert bases_upload(1, put(good_list(1), 48, 128, bytes(48))) == -1          # the encoding is checked all the same
    finally:
        set_option("ZK_KEY_SUBGROUP_CHECK", None)
    assert w1(pools[0]) == bad1 and w2(pools[1]) == bad2 and pools[0][:96 * last1] == bytes(pk.g1)[:96 * last1]
    assert P.g1_decode(pools[0][96 * last1:])[0] == P.NOT_IN_SUBGROUP and P.g2_decode(pools[1][192 * last2:])[0] == P.NOT_IN_SUBGROUP
    _refused(lambda: Groth16.from_compressed(cs, bad1, g2), -2)          # the option is back


# ------------------------------------------------------------------------------------------------------------------ device lists
def physical(devs):
    k = len(devs)
    return list(range(k)) if _lib.lib().zk_device_count() >= k else list(devs)


@pytest.mark.parametrize("devs", [[0, 0], [0, 0, 0]])
def test_device_lists_take_wire_bytes_for_both_protocols(devs):
    kinds = _three_kinds()
    cs, w, tox, pk = g16_key("n301")
    pcs, pw, ptox, ppk = pin_key("n301")
    rs, d = (11, 13), (3, 5, 7)
    exp = O.groth16_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, frs(w), frs(tox), P.fr_to_bytes(rs[0]), P.fr_to_bytes(rs[1]))
    pexp = O.pinocchio_prove_trapdoor(pcs.n, pcs.m, *csrs(pcs), pcs.mid, frs(pw), frs(ptox), *(P.fr_to_bytes(x) for x in d))
    g1, g2, q1, q2 = w1(pk.g1), w2(pk.g2), w1(ppk.g1), w2(ppk.g2)
    _lib.set_device_list(physical(devs))
    try:
        p = Groth16.from_compressed(cs, g1, g2)
        assert abc(p.prove_rs(w, *rs)) == exp and g16_pools(p) == [bytes(pk.g1), bytes(pk.g2)]
        assert bytes(p.pool_points(1, compressed=True)) == g1 and bytes(p.pool_points(2, compressed=True)) == g2
        p.derive_lagrange()
        assert abc(p.prove_rs(w, *rs)) == exp and g16_pools(p) == [bytes(pk.lag_g1), bytes(pk.lag_g2)]
        p.close()
        p = Groth16.from_compressed(cs, w1(pk.lag_g1), w2(pk.lag_g2), lagrange=True)
        assert abc(p.prove_rs(w, *rs)) == exp
        p.close()
        pp = PIN.ZK.from_compressed(pcs, q1, q2)
        ref = PIN.ZK(pcs, ppk)
        assert pp.prove_with(pw, *d).to_bytes() == pexp and pin_pools(pp) == pin_pools(ref)
        assert bytes(pp.pool_points(5, compressed=True)) == w1(pin_pools(ref)[5])
        pp.close(); ref.close()
        # a bad point in the LAST shard's slice: the code one device gives; and the first bad point of the lists decides across shards
        for data, rc in kinds[1]:
            _refused(lambda: Groth16.from_compressed(cs, put(g1, 48, len(g1) // 48 - 1, data), g2), rc)
            _refused(lambda: PIN.ZK.from_compressed(pcs, put(q1, 48, len(q1) // 48 - 1, data), q2), rc)
        for data, rc in kinds[2]:
            _refused(lambda: Groth16.from_compressed(cs, g1, put(g2, 96, len(g2) // 96 - 1, data)), rc)
            _refused(lambda: PIN.ZK.from_compressed(pcs, q1, put(q2, 96, len(q2) // 96 - 1, data)), rc)
        _refused(lambda: Groth16.from_compressed(cs, put(g1, 48, len(g1) // 48 - 1, kinds[1][1][0]), put(g2, 96, 0, kinds[2][0][0])), -2)   # last shard's G1 before first shard's G2
        _refused(lambda: Groth16.from_compressed(cs, put(put(g1, 48, len(g1) // 48 - 1, kinds[1][1][0]), 48, 2, kinds[1][0][0]), g2), -1)
        with pytest.raises(ValueError, match="wire: bad point .*single-device"):          # ZK_ERR_ARG, as for zk_pinocchio_pk_upload_lagrange
            PIN.ZK.from_compressed(pcs, q1, q2, h_lagrange=q1[:48 * pcs.n])
    finally:
        _lib.set_device_list([0])
