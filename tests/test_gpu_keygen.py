"""GPU parity of key generation in one call: zk_fr_lagrange_at against a plain product formula in Python integers, the key bytes of
zk_groth16_keygen / zk_pinocchio_keygen against the oracle's setup (literal at small n, exponents + spot-checked points at large n), the
pools of the returned handle against upload + derive_lagrange (an independent algorithm: NTTs in the exponent, no trapdoor), proofs from
the handle against the trapdoor oracles, zk_pinocchio_pk_upload_lagrange, every status code and the handle accounting."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import ref_programs as RP
from nonpow2_cases import product_formula          # the plain product formula in Python integers: the reference of zk_fr_lagrange_at below
from oracle import pyref as P
from zukelang_amd import _lib
from zukelang_amd import pinocchio as PIN
from zukelang_amd import r1cs as RC
from zukelang_amd.groth16 import Groth16, PKey, _csr, _p

pytestmark = pytest.mark.gpu

R = RC.FR_MODULUS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
frb = P.fr_to_bytes
frs = lambda xs: b"".join(frb(x) for x in xs)
csrs = lambda cs: [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
ZK_ERR_ARG, ZK_ERR_SCALAR_RANGE, ZK_ERR_HANDLE, ZK_ERR_DOMAIN = -1, -3, -7, -8
IDENT1, IDENT2 = b"\x40" + bytes(95), b"\x40" + bytes(191)


def _set_option(name, value):
    _lib.check(_lib.lib().zk_set_option(name.encode(), None if value is None else str(value).encode()))


# ------------------------------------------------------------------------------------------------------------------ zk_fr_lagrange_at
def lagrange_at(n, first, x):
    out = np.zeros(32 * n, dtype=np.uint8)
    z = np.zeros(32, dtype=np.uint8)
    _lib.check(_lib.lib().zk_fr_lagrange_at(n, first, _p(RC.fr_bytes([x])), _p(out), _p(z)))
    return RC.fr_ints(out), RC.fr_ints(z)[0]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 257, 4096, (1 << 16) + 3])
def test_lagrange_at_matches_the_product_formula(n):
    st = P.fr_stream(0x1A60 + n)
    for first in (0, n):
        dom = sorted({first, first + n // 2, first + n - 1})
        for x in [next(st), 0, R - 1] + dom:
            got, z = lagrange_at(n, first, x)
            idx = range(n) if n <= 4096 else sorted({0, 1, 31, 32, 33, 255, 256, 257, 8191, 8192, 8193, n // 2, n - 34, n - 2, n - 1})
            want, zw = product_formula(n, first, x, idx)
            assert z == zw, (n, first, x)
            assert all(got[i] == want[i] for i in idx), (n, first, x)
            assert sum(got) % R == 1                                # the basis sums to the constant 1 at every x
            if x in dom:
                hit = x - first                                   # a point of the domain: ONE value is 1, the rest 0, Z = 0 -- no division by x - i anywhere
                assert z == 0 and got[hit] == 1 and sum(1 for v in got if v) == 1, (n, first, x)


def test_lagrange_at_status_codes():
    L = _lib.lib()
    x = _p(RC.fr_bytes([5]))
    out = np.zeros(64, dtype=np.uint8)
    assert L.zk_fr_lagrange_at(2, 0, None, _p(out), None) == ZK_ERR_ARG
    assert L.zk_fr_lagrange_at(2, 0, x, None, None) == ZK_ERR_ARG
    assert L.zk_fr_lagrange_at(0, 0, x, _p(out), None) == ZK_ERR_ARG
    assert L.zk_fr_lagrange_at(2, 0xFFFFFFFF, x, _p(out), None) == ZK_ERR_ARG
    big = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8).copy()
    assert L.zk_fr_lagrange_at(2, 0, _p(big), _p(out), None) == ZK_ERR_SCALAR_RANGE
    assert L.zk_fr_lagrange_at(2, 0, x, _p(out), None) == 0     # z_out may be NULL
    assert RC.fr_ints(out) == [(1 - 5) % R, 5]


# ------------------------------------------------------------------------------------------------------------------ raw calls
def g16_sizes(cs):
    nm = int(np.count_nonzero(cs.mid))
    return 3 + (cs.n + 2) + (cs.n - 1) + nm, 2 + cs.n + 2, 1 + cs.m - nm, 3


def pin_sizes(cs):
    sz = O.pinocchio_sizes(cs.n, cs.m, cs.mid)
    return sz["pk_g1"], sz["pk_g2"], sz["vk_g1"], sz["vk_g2"]


def raw_keygen(proto, cs, toxic, form=1, want=(1, 1, 1, 1), handle=True, counts=None):
    """rc, [pk_g1, pk_g2, vk_g1, vk_g2] (bytes or None), handle value"""
    fn = _lib.lib().zk_groth16_keygen if proto == "groth16" else _lib.lib().zk_pinocchio_keygen
    sizes = g16_sizes(cs) if proto == "groth16" else pin_sizes(cs)
    bufs = [np.zeros(sz * (96, 192, 96, 192)[i], dtype=np.uint8) if want[i] else None for i, sz in enumerate(sizes)]
    ptr = [None if b is None else _p(b) for b in bufs]
    c1, c2 = counts if counts else sizes[:2]
    mid = np.ascontiguousarray(cs.mid, dtype=np.uint8)
    L, R_, Oo = _csr(cs.L), _csr(cs.R), _csr(cs.O)
    h = C.c_uint64(0)
    tox = np.frombuffer(bytes(toxic), dtype=np.uint8).copy()
    rc = fn(cs.n, cs.m, C.byref(L), C.byref(R_), C.byref(Oo), _p(mid), _p(tox), form, ptr[0], c1, ptr[1], c2, ptr[2], ptr[3], C.byref(h) if handle else None)
    return rc, [None if b is None else bytes(b) for b in bufs], h.value


def g16_pools(handle):
    out = []
    for group in (1, 2):
        cnt = C.c_size_t()
        _lib.check(_lib.lib().zk_groth16_pool_points(C.c_uint64(handle), group, None, C.c_size_t(0), C.byref(cnt)))
        buf = np.zeros(cnt.value * (96 if group == 1 else 192), dtype=np.uint8)
        _lib.check(_lib.lib().zk_groth16_pool_points(C.c_uint64(handle), group, _p(buf), C.c_size_t(cnt.value), C.byref(cnt)))
        out.append(bytes(buf))
    return out


def pin_pools(prover):
    return [bytes(prover.pool_points(i)) for i in range(8)]


CIRCUITS = {
    "readme": lambda: RC.readme_circuit(3),
    "n1": lambda: RC.random_r1cs(1, 6, 76, nnz=(1, 2)),                      # no lambda points, tiztd empty
    "cubic6": lambda: RC.iterated_cubic(6, 9),
    "unused": lambda: RC.random_r1cs(24, 40, 77),                            # m // 8 variables occur in no row: identity key points
    "no_one": lambda: RC.random_r1cs(48, 30, 78, one=False),
    "cubic64": lambda: RC.iterated_cubic(64, 10),
}


def all_public(maker):
    cs, w = maker()
    cs.mid = np.zeros(cs.m, dtype=np.uint8)                                  # I_mid empty: every variable is public
    return cs, w


def trapdoors(seed, cs, count, inside):
    """`count` trapdoor scalars; inside: tau (Groth16, index 4) resp. s (Pinocchio, index 2) is a point of the domain 0 .. n-1"""
    st = P.fr_stream(seed)
    tox = [next(st) for _ in range(count)]
    if inside:
        tox[4 if count == 5 else 2] = cs.n // 2
    return tox


# ------------------------------------------------------------------------------------------------------------------ key bytes, small
@pytest.mark.parametrize("name,inside", [(k, False) for k in CIRCUITS] + [("readme", True), ("cubic6", True), ("n1", True), ("mid0", False), ("mid0", True)])
def test_groth16_keygen_bytes_equal_the_literal_setup(name, inside):
    cs, w = all_public(CIRCUITS["cubic6"]) if name == "mid0" else CIRCUITS[name]()
    tox = trapdoors(0x6E16 + len(name), cs, 5, inside)
    q = O.QAP(cs.n, cs.m, *csrs(cs))
    want = q.groth16_setup(frs(tox), cs.mid)                                # orc_groth16_setup: Poly.apply on the dense QAP, per variable
    for form in (0, 1):
        rc, got, h = raw_keygen("groth16", cs, frs(tox), form=form)
        assert rc == 0 and tuple(got) == want, (name, form)
        _lib.check(_lib.lib().zk_groth16_pk_free(C.c_uint64(h)))
    pk1 = want[0]
    if inside and cs.n > 1:                                                # Z(tau) = 0: every tiztd point is the identity
        assert all(pk1[96 * (3 + cs.n + 2 + i):96 * (4 + cs.n + 2 + i)] == IDENT1 for i in range(cs.n - 1))
    if name == "unused":
        assert IDENT1 in [pk1[96 * i:96 * i + 96] for i in range(3 + 2 * cs.n + 1, len(pk1) // 96)]
    # bytes only (no handle), and each output on its own
    rc, got, _ = raw_keygen("groth16", cs, frs(tox), handle=False)
    assert rc == 0 and tuple(got) == want
    for i in range(4):
        rc, got, _ = raw_keygen("groth16", cs, frs(tox), want=[j == i for j in range(4)], handle=False)
        assert rc == 0 and got[i] == want[i]


@pytest.mark.parametrize("name,inside", [(k, False) for k in CIRCUITS] + [("readme", True), ("cubic6", True), ("n1", True), ("mid0", False), ("mid0", True)])
def test_pinocchio_keygen_bytes_equal_the_literal_exponents(name, inside):
    cs, w = all_public(CIRCUITS["cubic6"]) if name == "mid0" else CIRCUITS[name]()
    tox = trapdoors(0x9170 + len(name), cs, 8, inside)
    q = O.QAP(cs.n, cs.m, *csrs(cs))
    ex = O.pinocchio_keygen_exponents(q, cs.n, cs.m, *csrs(cs), cs.mid, frs(tox), True)          # literal = 1: Poly.apply per variable
    want = (O.points_of_exponents_g1(ex[0]), O.points_of_exponents_g2(ex[1]), O.points_of_exponents_g1(ex[2]), O.points_of_exponents_g2(ex[3]))
    for form in (0, 1):
        rc, got, h = raw_keygen("pinocchio", cs, frs(tox), form=form)
        assert rc == 0 and tuple(got) == want, (name, form)
        _lib.check(_lib.lib().zk_pinocchio_pk_free(C.c_uint64(h)))
    if inside:                                                             # t = Z(s) = 0: vt | yt | vavt | yayt | vbt | wbt | ybt and wt | wawt are the identity
        assert want[0][-96 * 7:] == IDENT1 * 7 and want[1][-192 * 2:] == IDENT2 * 2
    rc, got, _ = raw_keygen("pinocchio", cs, frs(tox), handle=False)
    assert rc == 0 and tuple(got) == want
    rc, got, h = raw_keygen("pinocchio", cs, frs(tox), want=(1, 0, 0, 1))          # no G2 key bytes: si2 is skipped on the device, everything else stands
    assert rc == 0 and got[0] == want[0] and got[3] == want[3]
    _lib.check(_lib.lib().zk_pinocchio_pk_free(C.c_uint64(h)))


# ------------------------------------------------------------------------------------------------------------------ key bytes and handles, large
def spot(points, exps, size, mul, gen, idx):
    for i in idx:
        if not 0 <= i < len(exps) // 32:
            continue
        assert bytes(points[size * i:size * i + size]) == mul(gen, exps[32 * i:32 * i + 32]), i


def check_groth16(cs, w, tox, cross_check):
    n, m = cs.n, cs.m
    toxic = frs(tox)
    e1, e2, eio = O.groth16_setup_exponents(n, m, *csrs(cs), cs.mid, toxic)
    rc, (pk1, pk2, vk1, vk2), h = raw_keygen("groth16", cs, toxic, form=1)
    assert rc == 0
    # EVERY point of the key is the fixed-base image of the oracle's exponent (at every size: zk_g1/g2_of_fr, itself spot-checked against the oracle below)
    from zukelang_amd.curve import G1, G2
    assert pk1 == bytes(G1.of_Fr(e1)) and pk2 == bytes(G2.of_Fr(e2)) and vk1[96:] == bytes(G1.of_Fr(eio))
    n1, n2 = len(e1) // 32, len(e2) // 32
    spot(pk1, e1, 96, O.g1_mul, O.g1_generator(), sorted({0, 1, 2, 3, 4, n + 4, n + 5, n + 6, 2 * n + 3, 2 * n + 4, 2 * n + 5, n1 // 2, n1 - 2, n1 - 1}))
    spot(pk2, e2, 192, O.g2_mul, O.g2_generator(), sorted({0, 1, 2, 3, n2 // 2, n2 - 1}))
    spot(vk1[96:], eio, 96, O.g1_mul, O.g1_generator(), range(len(eio) // 32))
    assert vk1[:96] == O.g1_generator() and vk2[:192] == O.g2_generator()
    assert vk2[192:384] == O.g2_mul(O.g2_generator(), frb(tox[2])) and vk2[384:] == pk2[192:384]
    pools = g16_pools(h)
    prover = Groth16.__new__(Groth16)
    prover.circuit, prover.rank, prover.world, prover._keep, prover.handle = cs, 0, 1, (cs,), C.c_uint64(h)
    st = P.fr_stream(0xAB + n)
    rs = [(next(st), next(st)) for _ in range(4)]
    exp = [O.groth16_prove_trapdoor(n, m, *csrs(cs), cs.mid, frs(w), toxic, frb(r), frb(s)) for r, s in rs]
    got = prover.prove_rs(w, *rs[0])
    assert (got.a, got.b, got.c) == exp[0]
    prover.set_witness(w)
    for slot in range(3):
        prover.prove_async(None, *rs[1 + slot], slot)
    for slot in range(3):
        got = prover.prove_wait(slot)
        assert (got.a, got.b, got.c) == exp[1 + slot], slot
    prover.close()
    # the tau-power handle == a plain upload of the key bytes
    rc, _, h0 = raw_keygen("groth16", cs, toxic, form=0, want=(0, 0, 0, 0))
    assert rc == 0
    assert g16_pools(h0) == [pk1, pk2]
    _lib.check(_lib.lib().zk_groth16_pk_free(C.c_uint64(h0)))
    if cross_check:
        up = Groth16(cs, PKey(np.frombuffer(pk1, dtype=np.uint8), np.frombuffer(pk2, dtype=np.uint8)))
        assert g16_pools(up.handle.value) == [pk1, pk2]
        up.derive_lagrange()                                                 # NTTs in the exponent over the key's own points: never sees tau
        assert g16_pools(up.handle.value) == pools
        up.close()


def check_pinocchio(cs, w, tox, cross_check, compact):
    n, m = cs.n, cs.m
    toxic = frs(tox)
    _set_option("ZK_PIN_COMPACT_H", None if compact else "0")
    try:
        e1, e2, v1, v2 = O.pinocchio_keygen_exponents(None, n, m, *csrs(cs), cs.mid, toxic, False)
        rc, (pk1, pk2, vk1, vk2), h = raw_keygen("pinocchio", cs, toxic, form=1)
        assert rc == 0
        from zukelang_amd.curve import G1, G2          # every point, at every size, as for Groth16 above
        assert pk1 == bytes(G1.of_Fr(e1)) and pk2 == bytes(G2.of_Fr(e2)) and vk1 == bytes(G1.of_Fr(v1)) and vk2 == bytes(G2.of_Fr(v2))
        n1, n2, nm = len(e1) // 32, len(e2) // 32, int(np.count_nonzero(cs.mid))
        spot(pk1, e1, 96, O.g1_mul, O.g1_generator(), sorted({0, nm - 1, nm, 3 * nm, 5 * nm - 1, 5 * nm, 5 * nm + 1, 5 * nm + n, 5 * nm + n + 1, 5 * nm + n + m, n1 - 8, n1 - 7, n1 - 1}))
        spot(pk2, e2, 192, O.g2_mul, O.g2_generator(), sorted({0, nm, 2 * nm - 1, 2 * nm, 2 * nm + n, n2 - 2, n2 - 1}))
        spot(vk1, v1, 96, O.g1_mul, O.g1_generator(), range(len(v1) // 32))
        spot(vk2, v2, 192, O.g2_mul, O.g2_generator(), range(len(v2) // 32))
        prover = PIN.ZK.__new__(PIN.ZK)
        prover.circuit, prover._keep, prover.handle = cs, (cs,), C.c_uint64(h)
        pools = pin_pools(prover)
        assert len(pools[5]) // 96 == (n + 2 if compact else n + 1 + 2 * m)
        st = P.fr_stream(0xCD + n)
        ds = [[next(st) for _ in range(3)] for _ in range(4)] + [[0, 0, 0]]                  # ZK, and NonZK = all zero
        exp = [O.pinocchio_prove_trapdoor(n, m, *csrs(cs), cs.mid, frs(w), toxic, *(frb(x) for x in d)) for d in ds]
        assert prover.prove_with(w, *ds[0]).to_bytes() == exp[0]
        assert prover.prove_with(w, *ds[4]).to_bytes() == exp[4]
        prover.set_witness(w)
        for slot in range(3):
            prover.prove_async(*ds[1 + slot], slot)
        for slot in range(3):
            assert prover.prove_wait(slot).to_bytes() == exp[1 + slot], slot
        prover.close()
        pk = PIN.PKey(np.frombuffer(pk1, dtype=np.uint8), np.frombuffer(pk2, dtype=np.uint8))
        rc, _, h0 = raw_keygen("pinocchio", cs, toxic, form=0, want=(0, 0, 0, 0))
        assert rc == 0
        p0 = PIN.ZK.__new__(PIN.ZK)
        p0.circuit, p0._keep, p0.handle = cs, (cs,), C.c_uint64(h0)
        tau_pools = pin_pools(p0)
        assert p0.prove_with(w, *ds[0]).to_bytes() == exp[0]
        p0.close()
        if cross_check:
            up = PIN.ZK(cs, pk)
            assert pin_pools(up) == tau_pools                                # ... == a plain upload
            up.derive_lagrange()
            assert pin_pools(up) == pools
            up.close()
        # zk_pinocchio_pk_upload_lagrange, fed the first n points of the Lagrange-form pool
        fl = PIN.ZK.from_lagrange(cs, pk, np.frombuffer(pools[5][:96 * n], dtype=np.uint8))
        assert pin_pools(fl) == pools
        assert fl.prove_with(w, *ds[0]).to_bytes() == exp[0]
        fl.close()
    finally:
        _set_option("ZK_PIN_COMPACT_H", None)


@pytest.mark.parametrize("log_n", [10, 12, 16])
def test_groth16_keygen_exponents_points_pools_and_proofs(log_n):
    n = 1 << log_n
    cs, w = RC.random_r1cs(n, n + n // 4, 0x6E00 + log_n, nnz=(1, 6))
    check_groth16(cs, w, trapdoors(0x77 + log_n, cs, 5, False), cross_check=True)


@pytest.mark.parametrize("log_n,compact", [(10, True), (10, False), (12, True), (12, False), (16, True), (16, False)])
def test_pinocchio_keygen_exponents_points_pools_and_proofs(log_n, compact):
    n = 1 << log_n
    cs, w = RC.random_r1cs(n, n + n // 4, 0x9100 + log_n, nnz=(1, 6))
    check_pinocchio(cs, w, trapdoors(0x88 + log_n, cs, 8, False), cross_check=True, compact=compact)


@pytest.mark.parametrize("name", ["readme", "n1", "unused", "mid0"])
def test_small_circuits_handles_and_proofs(name):
    cs, w = all_public(CIRCUITS["cubic6"]) if name == "mid0" else CIRCUITS[name]()
    # (a trapdoor inside the domain is held to the LITERAL setup in the byte tests above, and on every route to a handle in tests/test_gpu_degenerate_trapdoors.py)
    check_groth16(cs, w, trapdoors(0x51 + len(name), cs, 5, False), cross_check=True)
    for compact in (True, False):
        check_pinocchio(cs, w, trapdoors(0x52 + len(name), cs, 8, False), cross_check=True, compact=compact)


# ------------------------------------------------------------------------------------------------------------------ the reference's programs through generate
@pytest.mark.parametrize("name", RP.names())
def test_generate_proves_the_reference_programs(name):
    p = RP.program(name)
    cs = RP.circuit(p)
    m = cs.m
    tox, r, s = RP.groth16_params(p)
    q = O.QAP(cs.n, m, *csrs(cs))
    pk1, pk2, vk1, vk2 = q.groth16_setup(frs(tox), cs.mid)
    ws = RP.witnesses(p)
    for form in ("lagrange", "tau_powers"):
        it = iter(tox)
        pr, pk, vk = Groth16.generate(lambda: next(it), cs, form=form)
        assert bytes(pk.g1) == pk1 and bytes(pk.g2) == pk2 and vk.one1 + bytes(vk.ltgm_io) == vk1 and vk.one2 + vk.gm + vk.d == vk2
        for w, fix in zip(ws, p["witnesses"]):
            got = pr.prove_rs(w, r, s)
            assert (got.a, got.b, got.c) == RP.groth16_proof(fix), (name, form)             # the golden bytes ARE the literal oracle's (CPU test of this fixture)
            io = [w[k] for k in range(m) if not cs.mid[k]]
            assert Groth16.verify(io, vk, got)
        pr.close()
    ptox, (dv, dw, dy) = RP.pinocchio_params(p)
    ex = O.pinocchio_keygen_exponents(q, cs.n, m, *csrs(cs), cs.mid, frs(ptox), True)
    for form, cls in (("lagrange", PIN.ZK), ("tau_powers", PIN.NonZK)):
        it = iter(ptox)
        pp, ppk, pvk = cls.generate(lambda: next(it), cs, form=form)
        assert bytes(ppk.g1) == O.points_of_exponents_g1(ex[0]) and bytes(ppk.g2) == O.points_of_exponents_g2(ex[1])
        assert bytes(pvk.g1) == O.points_of_exponents_g1(ex[2]) and bytes(pvk.g2) == O.points_of_exponents_g2(ex[3])
        for w, fix in zip(ws, p["witnesses"]):
            got = pp.prove_with(w, dv, dw, dy)
            assert got.to_bytes() == RP.pinocchio_proof(fix, True), (name, form)
            assert pp.prove_with(w, 0, 0, 0).to_bytes() == RP.pinocchio_proof(fix, False)
            io = [w[k] for k in range(m) if not cs.mid[k]]
            assert PIN.ZK.verify(io, pvk, got)
        pp.close()


def test_generate_draws_like_keygen():
    """the same rng gives the same key bytes as the host-side keygen functions, which stay as they are"""
    cs, w = RC.iterated_cubic(30, 7)
    st = P.fr_stream(0xD0A); a = [next(st) for _ in range(6)]
    it = iter(a); pk, vk = Groth16.keygen(lambda: next(it), cs); assert next(it) == a[5]
    it = iter(a); pr, pk2, vk2 = Groth16.generate(lambda: next(it), cs); assert next(it) == a[5]
    assert bytes(pk.g1) == bytes(pk2.g1) and bytes(pk.g2) == bytes(pk2.g2) and vk.ab == vk2.ab and bytes(vk.ltgm_io) == bytes(vk2.ltgm_io)
    pr.close()
    a = [next(st) for _ in range(9)]
    it = iter(a); pk, vk = PIN.keygen(lambda: next(it), cs); assert next(it) == a[8]
    it = iter(a); pr, pk2, vk2 = PIN.generate(lambda: next(it), cs); assert next(it) == a[8]
    assert bytes(pk.g1) == bytes(pk2.g1) and bytes(pk.g2) == bytes(pk2.g2) and bytes(vk.g1) == bytes(vk2.g1) and bytes(vk.g2) == bytes(vk2.g2)
    assert isinstance(pr, PIN.ZK)
    pr.close()


# ------------------------------------------------------------------------------------------------------------------ errors and lifetime
@pytest.mark.parametrize("proto,ntox", [("groth16", 5), ("pinocchio", 8)])
def test_keygen_status_codes(proto, ntox):
    cs, w = RC.iterated_cubic(6, 9)
    L = _lib.lib()
    fn = L.zk_groth16_keygen if proto == "groth16" else L.zk_pinocchio_keygen
    tox = trapdoors(0xE0, cs, ntox, False)
    ok = frs(tox)
    sizes = g16_sizes(cs) if proto == "groth16" else pin_sizes(cs)
    assert raw_keygen(proto, cs, ok, form=2)[0] == ZK_ERR_ARG
    assert raw_keygen(proto, cs, ok, counts=(sizes[0] + 1, sizes[1]))[0] == ZK_ERR_DOMAIN
    assert raw_keygen(proto, cs, ok, counts=(sizes[0], sizes[1] - 1))[0] == ZK_ERR_DOMAIN
    for i in range(ntox):
        bad = list(tox); bad[i] = R
        assert raw_keygen(proto, cs, b"".join(x.to_bytes(32, "little") for x in bad))[0] == ZK_ERR_SCALAR_RANGE, i
    if proto == "groth16":
        for i in (2, 3):                                                  # gamma = 0, delta = 0: the reference raises (division by zero)
            bad = list(tox); bad[i] = 0
            assert raw_keygen(proto, cs, frs(bad))[0] == ZK_ERR_ARG
        for i in (0, 1, 4):                                               # alpha, beta, tau = 0 are served
            bad = list(tox); bad[i] = 0
            rc, got, h = raw_keygen(proto, cs, frs(bad))
            assert rc == 0 and tuple(got) == O.QAP(cs.n, cs.m, *csrs(cs)).groth16_setup(frs(bad), cs.mid)
            L.zk_groth16_pk_free(C.c_uint64(h))
    # null arguments
    mid = np.ascontiguousarray(cs.mid, dtype=np.uint8)
    A, B, Cc = _csr(cs.L), _csr(cs.R), _csr(cs.O)
    t = np.frombuffer(ok, dtype=np.uint8).copy()
    h = C.c_uint64()
    args = [cs.n, cs.m, C.byref(A), C.byref(B), C.byref(Cc), _p(mid), _p(t), 1, None, 0, None, 0, None, None, C.byref(h)]
    for i in (2, 3, 4, 5, 6):
        a = list(args); a[i] = None
        assert fn(*a) == ZK_ERR_ARG, i
    a = list(args); a[0] = 0
    assert fn(*a) == ZK_ERR_ARG
    # a coefficient >= r, a column out of range
    bad = RC.iterated_cubic(6, 9)[0]
    bad.L.val = bad.L.val.copy(); bad.L.val[:32] = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8)
    assert raw_keygen(proto, bad, ok)[0] == ZK_ERR_SCALAR_RANGE
    bad = RC.iterated_cubic(6, 9)[0]
    bad.R.col = bad.R.col.copy(); bad.R.col[0] = bad.m
    assert raw_keygen(proto, bad, ok)[0] == ZK_ERR_ARG


def test_handle_accounting_and_device_lists():
    cs, w = RC.iterated_cubic(6, 9)
    L = _lib.lib()
    g = frs(trapdoors(1, cs, 5, False)); p = frs(trapdoors(2, cs, 8, False))
    rc, _, h1 = raw_keygen("groth16", cs, g)
    rc2, _, h2 = raw_keygen("pinocchio", cs, p)
    assert rc == 0 and rc2 == 0 and h1 and h2
    devs = (C.c_int32 * 2)(0, 0)
    assert L.zk_set_device_list(devs, 2) == ZK_ERR_ARG                     # generated handles count as live key handles
    assert L.zk_groth16_pk_free(C.c_uint64(h1)) == 0 and L.zk_groth16_pk_free(C.c_uint64(h1)) == ZK_ERR_HANDLE
    assert L.zk_set_device_list(devs, 2) == ZK_ERR_ARG
    assert L.zk_pinocchio_pk_free(C.c_uint64(h2)) == 0 and L.zk_pinocchio_pk_free(C.c_uint64(h2)) == ZK_ERR_HANDLE
    try:
        _lib.set_device_list([0, 0])
        # a two-entry list: no handle, but the bytes can be had
        assert raw_keygen("groth16", cs, g)[0] == ZK_ERR_ARG
        assert raw_keygen("pinocchio", cs, p)[0] == ZK_ERR_ARG
        rc, got, _ = raw_keygen("groth16", cs, g, handle=False)
        assert rc == 0 and tuple(got) == O.QAP(cs.n, cs.m, *csrs(cs)).groth16_setup(g, cs.mid)
        rc, got, _ = raw_keygen("pinocchio", cs, p, handle=False)
        ex = O.pinocchio_keygen_exponents(None, cs.n, cs.m, *csrs(cs), cs.mid, p, False)
        assert rc == 0 and got[0] == O.points_of_exponents_g1(ex[0]) and got[3] == O.points_of_exponents_g2(ex[3])
        pk = PIN.PKey(np.frombuffer(got[0], dtype=np.uint8), np.frombuffer(got[1], dtype=np.uint8))
        with pytest.raises(_lib.ZkError) as e:
            PIN.ZK.from_lagrange(cs, pk, np.zeros(96 * cs.n, dtype=np.uint8))
        assert e.value.code == ZK_ERR_ARG
    finally:
        _lib.set_device_list([0])
    # zk_shutdown frees generated handles like uploaded ones
    rc, _, h1 = raw_keygen("groth16", cs, g)
    rc2, _, h2 = raw_keygen("pinocchio", cs, p)
    assert rc == 0 and rc2 == 0
    assert L.zk_shutdown() == 0
    _lib.check(L.zk_init(0))
    assert L.zk_groth16_pk_free(C.c_uint64(h1)) == ZK_ERR_HANDLE and L.zk_pinocchio_pk_free(C.c_uint64(h2)) == ZK_ERR_HANDLE
    _lib.set_device_list([0, 0]); _lib.set_device_list([0])                # nothing is alive any more


def test_upload_lagrange_checks_its_points():
    cs, w = RC.iterated_cubic(6, 9)
    it = iter(trapdoors(3, cs, 8, False))
    pr, pk, vk = PIN.ZK.generate(lambda: next(it), cs)
    hl = pr.pool_points(5)[:96 * cs.n].copy()
    pr.close()
    L = _lib.lib()
    bad = hl.copy(); bad[95] ^= 1                                          # off the curve
    with pytest.raises(_lib.ZkError) as e:
        PIN.ZK.from_lagrange(cs, pk, bad)
    assert e.value.code == -2
    bad = hl.copy(); bad[0] |= 0x80                                        # compression flag on an uncompressed point
    with pytest.raises(_lib.ZkError) as e:
        PIN.ZK.from_lagrange(cs, pk, bad)
    assert e.value.code == ZK_ERR_ARG
    with pytest.raises(ValueError):
        PIN.ZK.from_lagrange(cs, pk, hl[:-96])
    mid = np.ascontiguousarray(cs.mid, dtype=np.uint8)
    A, B, Cc = _csr(cs.L), _csr(cs.R), _csr(cs.O)
    h = C.c_uint64()
    g1, g2 = np.ascontiguousarray(pk.g1), np.ascontiguousarray(pk.g2)
    assert L.zk_pinocchio_pk_upload_lagrange(cs.n, cs.m, C.byref(A), C.byref(B), C.byref(Cc), _p(mid), _p(g1), len(g1) // 96, _p(g2), len(g2) // 192, None, C.byref(h)) == ZK_ERR_ARG
    assert L.zk_pinocchio_pk_upload_lagrange(cs.n, cs.m, C.byref(A), C.byref(B), C.byref(Cc), _p(mid), _p(g1), len(g1) // 96 - 1, _p(g2), len(g2) // 192, _p(hl), C.byref(h)) == ZK_ERR_DOMAIN
    assert L.zk_pinocchio_pk_upload_lagrange(cs.n, cs.m, C.byref(A), C.byref(B), C.byref(Cc), _p(mid), _p(g1), len(g1) // 96, _p(g2), len(g2) // 192, _p(hl), C.byref(h)) == 0
    assert L.zk_pinocchio_pk_free(h) == 0


# ------------------------------------------------------------------------------------------------------------------ C host
def test_c_host_uploads_the_lagrange_form_and_prints_the_golden_proof(tmp_path):
    """examples/c_pinocchio.c, the leg after the derivation: the README fixture key through zk_pinocchio_pk_upload_lagrange with the first-principles
    points of tests/golden/readme_pinocchio_h_lagrange.json; the proof it prints is the golden one."""
    import json
    libdir = os.path.join(ROOT, "zukelang_amd")
    exe = str(tmp_path / "c_pinocchio")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "examples"),
                           os.path.join(ROOT, "examples", "c_pinocchio.c"), "-o", exe, "-L" + libdir, "-lzkmi355x", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "readme_pinocchio_key.json")))["proof"]
    lines = out.stdout.decode().splitlines()
    assert lines[0].startswith("c-pinocchio ok (1 device entry)") and lines[1] == "proof (upload_lagrange): " + gold
