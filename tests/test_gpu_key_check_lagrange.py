"""zk_groth16_key_check_lagrange on the device against its specification, the integer model of tests/key_check_lagrange_model.py: Lagrange-form keys
are built from (edited) exponent lists through G1/G2.of_Fr, uploaded in that form, checked, and the mask must be the model's -- 0 for honest keys
whatever the seed, the route the handle came by and the size; the model's bits for every crafted key of tests/key_check_lagrange_cases.py.  Then the
call's contract: the handle is left as it was found (proof bytes), a proof from a checked handle verifies, and every refusal of include/zkmi355x.h."""
import ctypes as C
import functools

import numpy as np
import pytest

import key_check_lagrange_cases as LC
import key_check_lagrange_model as LM
from zukelang_amd import _lib, r1cs as RC
from zukelang_amd.curve import G1, G2, Pairing
from zukelang_amd.groth16 import Groth16, PKey, VKey
from zukelang_amd.r1cs import fr_bytes

pytestmark = pytest.mark.gpu

TOX = [0x1111 + 7919 * i + (i << 200) for i in range(1, 6)]
SEEDS = [bytes(range(32)), bytes([0xA5] * 32), (0x0123456789ABCDEF << 192 | 0xFEDCBA9876543210).to_bytes(32, "little")]


def zero_row_circuit():
    """gate 1 has an all-zero row in L and O; variable 5 appears in no gate"""
    L = RC.Matrix.from_rows([{3: 1}, {}, {2: 1, 3: 1, 0: 3}, {1: 2}])
    R = RC.Matrix.from_rows([{3: 1}, {3: 1}, {0: 1}, {0: 1}])
    O = RC.Matrix.from_rows([{1: 1}, {}, {4: 1}, {2: 1}])
    return RC.R1CS(4, 6, L, R, O, np.array([0, 1, 1, 1, 0, 1], dtype=np.uint8))


def readme_other():
    cs, _ = RC.readme_circuit(3)
    return RC.R1CS(cs.n, cs.m, RC.Matrix.from_rows([{3: 1}, {1: 1}, {2: 1, 3: 2, 0: 3}]), cs.R, cs.O, cs.mid)


CIRCUITS = {
    "readme": lambda: RC.readme_circuit(3)[0],
    "n1": lambda: RC.random_r1cs(1, 4, 9, nnz=(1, 2))[0],
    "n2": lambda: RC.random_r1cs(2, 6, 11, nnz=(1, 3))[0],
    "n5": lambda: RC.random_r1cs(5, 12, 3, nnz=(1, 3))[0],                  # no power of two
    "n13": lambda: RC.random_r1cs(13, 24, 4, nnz=(8, 8))[0],                # no power of two, 8 entries per row
    "n1025": lambda: RC.random_r1cs(1025, 1100, 5, nnz=(8, 8))[0],          # S = 4096: the first size whose convolution leaves the fused LDS kernel
    "zero_row": zero_row_circuit,
}


@functools.lru_cache(maxsize=None)
def circuit(name):
    return CIRCUITS[name]()


@functools.lru_cache(maxsize=None)
def honest(name):
    return LM.honest_lagrange_exponents(circuit(name), TOX)


def points(lx1, lx2, vk):
    """a PKey whose Lagrange-form pools are the points of lx1 / lx2 (its tau-power pools are not read by a Lagrange-form upload), and the VKey"""
    g1, g2 = G1.of_Fr(fr_bytes(lx1)), G2.of_Fr(fr_bytes(lx2))
    pk = PKey(g1, g2)
    pk.lag_g1, pk.lag_g2 = g1, g2
    v1 = G1.of_Fr(fr_bytes([vk["one1"]] + vk["ltgm_io"]))
    v2 = G2.of_Fr(fr_bytes([vk["one2"], vk["gm"], vk["d"]]))
    return pk, VKey(bytes(v1[:96]), v1[96:], bytes(v2[:192]), bytes(v2[192:384]), bytes(v2[384:]), Pairing.pairing(bytes(g1[:96]), bytes(g2[:192])))


def device_masks(cs, lx1, lx2, vk, seed=SEEDS[0]):
    pk, vkey = points(lx1, lx2, vk)
    prover = Groth16(cs, pk, lagrange=True)
    try:
        return prover.check_lagrange_key(seed=seed).failed, prover.check_lagrange_key(vkey, seed=seed).failed
    finally:
        prover.close()


def model_masks(cs, lx1, lx2, vk):
    return LM.lagrange_mask(cs, lx1, lx2), LM.lagrange_mask(cs, lx1, lx2, vk)


@pytest.fixture(autouse=True)
def _init_and_leave_nothing_behind():
    _lib.check(_lib.lib().zk_init(0))
    yield
    _lib.set_device_list([0])          # ZK_ERR_ARG while any key handle is alive


# ---------------------------------------------------------------- honest keys give 0
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_honest_key_is_well_formed_at_every_size(name):
    cs = circuit(name)
    lx1, lx2, vk = honest(name)
    assert model_masks(cs, lx1, lx2, vk) == (0, 0)
    assert device_masks(cs, lx1, lx2, vk) == (0, 0)


@pytest.mark.parametrize("name", ["readme", "n5", "zero_row"])
def test_honest_key_with_tau_inside_the_domain(name):
    """l1 and l2 are unit vectors, every hl is the identity: c = 0 in (i - tau) x_i = c w_i"""
    cs = circuit(name)
    lx1, lx2, vk = LC.honest_inside_domain(cs, TOX, tau=2)
    assert model_masks(cs, lx1, lx2, vk) == (0, 0)
    assert device_masks(cs, lx1, lx2, vk) == (0, 0)


def test_honest_key_under_every_seed_and_route():
    cs = circuit("readme")
    it = iter(TOX)
    pk, vk = Groth16.keygen(lambda: next(it), cs, lagrange=True)
    lx1, lx2, _ = honest("readme")
    assert bytes(pk.lag_g1) == bytes(G1.of_Fr(fr_bytes(lx1))) and bytes(pk.lag_g2) == bytes(G2.of_Fr(fr_bytes(lx2)))          # keygen's key IS the model's
    routes = [Groth16(cs, pk, lagrange=True)]
    it = iter(TOX)
    gen, gpk, gvk = Groth16.generate(lambda: next(it), cs, form="lagrange")
    assert bytes(gpk.g1) == bytes(pk.g1) and bytes(gvk.gm) == bytes(vk.gm)
    routes.append(gen)
    derived = Groth16(cs, pk)
    derived.derive_lagrange()
    routes.append(derived)
    cached = Groth16.from_compressed(cs, derived.pool_points(1, compressed=True), derived.pool_points(2, compressed=True), lagrange=True)
    routes.append(cached)
    for prover in routes:
        for seed in SEEDS + [None]:
            for v in (None, vk):
                res = prover.check_lagrange_key(v, seed=seed)
                assert res.ok and res.failed == 0 and res.names == [] and bool(res)
        prover.close()


@pytest.mark.parametrize("name", ["n1", "n2", "n5", "n13", "n1025"])
def test_a_derived_key_is_well_formed_at_every_size(name):
    """the route the key cache takes: tau-power upload, derivation on the device, the pools out and in again in wire form"""
    cs = circuit(name)
    it = iter(TOX)
    pk, vk = Groth16.keygen(lambda: next(it), cs)
    derived = Groth16(cs, pk)
    derived.derive_lagrange()
    assert derived.check_lagrange_key(vk, seed=SEEDS[1]).failed == 0
    cached = Groth16.from_compressed(cs, derived.pool_points(1, compressed=True), derived.pool_points(2, compressed=True), lagrange=True)
    derived.close()
    assert cached.check_lagrange_key(vk, seed=SEEDS[2]).failed == 0
    cached.close()


# ---------------------------------------------------------------- crafted keys give the model's bits
README_CASES = LC.crafted(RC.readme_circuit(3)[0], TOX, readme_other())


@pytest.mark.parametrize("name,lx1,lx2,vk", README_CASES, ids=[c[0] for c in README_CASES])
def test_crafted_readme_keys(name, lx1, lx2, vk):
    cs = circuit("readme")
    want = model_masks(cs, lx1, lx2, vk)
    assert want == LC.BITS[name]
    for seed in SEEDS[:2]:
        assert device_masks(cs, lx1, lx2, vk, seed) == want, name


@pytest.mark.parametrize("size", ["n2", "n5", "n13", "zero_row"])
def test_crafted_keys_at_other_sizes(size):
    cs = circuit(size)
    for name, lx1, lx2, vk in LC.crafted(cs, TOX):
        assert device_masks(cs, lx1, lx2, vk) == model_masks(cs, lx1, lx2, vk), name


def test_crafted_keys_at_1025():
    cs = circuit("n1025")
    cases = {c[0]: c for c in LC.crafted(cs, TOX)}
    for name in ("hl_opposite", "ltd_mid_opposite"):
        _, lx1, lx2, vk = cases[name]
        want = LM.lagrange_mask(cs, lx1, lx2, vk)
        assert want == LC.BITS[name][1]
        assert device_masks(cs, lx1, lx2, vk)[1] == want, name


def test_under_the_residue_number_system():
    """ZK_FR_RNS=1 at upload: the extrapolation of pi and of L mu, R mu, O mu runs through the other convolution (frstage_extrapolate's second branch)"""
    cs = circuit("n1025")
    cases = {c[0]: c for c in LC.crafted(cs, TOX)}
    _lib.check(_lib.lib().zk_set_option(b"ZK_FR_RNS", b"1"))
    try:
        assert device_masks(cs, *honest("n1025")) == (0, 0)
        _, lx1, lx2, vk = cases["hl_opposite"]
        assert device_masks(cs, lx1, lx2, vk) == LC.BITS["hl_opposite"]
    finally:
        _lib.check(_lib.lib().zk_set_option(b"ZK_FR_RNS", None))


def test_the_ab_bit():
    cs = circuit("readme")
    pk, vkey = points(*honest("readme"))
    prover = Groth16(cs, pk, lagrange=True)
    vkey.ab = Pairing.pairing(bytes(pk.g1[96:192]), bytes(pk.g2[:192]))          # e(d1, b2): not this key's ab
    res = prover.check_lagrange_key(vkey)
    assert not res.ok and res.failed == _lib.KEYCHK_AB and res.names == ["ab"]
    prover.close()


# ---------------------------------------------------------------- the contract
@pytest.mark.parametrize("name", ["readme", "n1025"])
def test_the_handle_is_left_as_it_was_found_and_its_proofs_verify(name):
    cs, w = RC.readme_circuit(3) if name == "readme" else RC.random_r1cs(1025, 1100, 5, nnz=(8, 8))
    pk, vkey = points(*honest(name))
    prover = Groth16(cs, pk, lagrange=True)
    before = prover.prove_rs(w, 5, 7)
    assert prover.check_lagrange_key(vkey).ok
    after = prover.prove_rs(w, 5, 7)
    assert (before.a, before.b, before.c) == (after.a, after.b, after.c)
    assert Groth16.verify([w[k] for k in range(cs.m) if not cs.mid[k]], vkey, after)
    prover.close()


def _raw(handle, v1, n_io, v2, seed, failed):
    p = lambda b: None if b is None else np.frombuffer(bytes(b), dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    keep = [v1, v2, seed]          # noqa: F841
    return _lib.lib().zk_groth16_key_check_lagrange(handle, p(v1), n_io, p(v2), p(seed), failed)


def test_refusals():
    cs, w = RC.readme_circuit(3)
    it = iter(TOX)
    pk, vkey = Groth16.keygen(lambda: next(it), cs, lagrange=True)
    v1, v2 = bytes(vkey.one1) + bytes(vkey.ltgm_io), bytes(vkey.one2) + bytes(vkey.gm) + bytes(vkey.d)
    n_io = cs.m - cs.n_mid
    failed = C.c_uint32(0)
    err = _lib.lib().zk_last_error
    prover = Groth16(cs, pk, lagrange=True)
    h = prover.handle
    assert _raw(h, v1, n_io, v2, SEEDS[0], C.byref(failed)) == 0 and failed.value == 0
    assert _raw(h, v1, n_io, v2, None, C.byref(failed)) == 0 and failed.value == 0          # the library draws the seed
    assert _raw(h, v1, n_io, v2, SEEDS[0], None) == -1 and b"failed" in err()                 # null failed
    assert _raw(h, v1, n_io, None, SEEDS[0], C.byref(failed)) == -1 and b"together" in err()  # exactly one of vk_g1 / vk_g2
    assert _raw(h, None, 0, v2, SEEDS[0], C.byref(failed)) == -1 and b"together" in err()
    assert _raw(h, v1[:-96], n_io - 1, v2, SEEDS[0], C.byref(failed)) == -1 and b"n_io" in err()          # n_io is not m - |mids|
    assert _raw(C.c_uint64(0xDEAD), v1, n_io, v2, SEEDS[0], C.byref(failed)) == -7            # unknown handle
    bad = bytearray(v1)
    bad[96 + 95] ^= 1                                                                         # ltgm_io[0] off the curve
    assert _raw(h, bytes(bad), n_io, v2, SEEDS[0], C.byref(failed)) == -2 and b"G1 point in the verification key" in err()
    bad = bytearray(v2)
    bad[192] |= 0x80                                                                          # gm: compression flag on an uncompressed point
    assert _raw(h, v1, n_io, bytes(bad), SEEDS[0], C.byref(failed)) == -1 and b"G2 point in the verification key" in err()
    prover.prove_async(w, 5, 7, 0)                                                            # a proof in flight
    assert _raw(h, None, 0, None, SEEDS[0], C.byref(failed)) == -1 and b"in flight" in err()
    prover.prove_wait(0)
    assert _raw(h, None, 0, None, SEEDS[0], C.byref(failed)) == 0 and failed.value == 0
    prover.close()
    powers = Groth16(cs, pk)                                                                  # a tau-power handle
    assert _raw(powers.handle, None, 0, None, SEEDS[0], C.byref(failed)) == -1
    assert b"tau powers" in err() and b"zk_groth16_key_check" in err().replace(b"zk_groth16_key_check_lagrange", b"")
    powers.derive_lagrange()
    powers.shard(0, 2)                                                                        # a shard
    assert _raw(powers.handle, None, 0, None, SEEDS[0], C.byref(failed)) == -1 and b"shard" in err()
    powers.close()
    _lib.check(_lib.lib().zk_set_option(b"key_subgroup_check", b"0"))
    try:
        unchecked = Groth16(cs, pk, lagrange=True)
        assert _raw(unchecked.handle, None, 0, None, SEEDS[0], C.byref(failed)) == -1
        assert b"SUBGROUP_CHECK" in err()
        unchecked.close()
    finally:
        _lib.check(_lib.lib().zk_set_option(b"key_subgroup_check", None))
    _lib.set_device_list([0, 0])                                                              # a multi-device handle
    try:
        multi = Groth16(cs, pk)
        multi.derive_lagrange()
        assert _raw(multi.handle, None, 0, None, SEEDS[0], C.byref(failed)) == -1 and b"multi-device" in err()
        multi.close()
    finally:
        _lib.set_device_list([0])
