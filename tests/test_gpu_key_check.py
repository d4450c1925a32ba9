"""zk_groth16_key_check on the device against its specification, the integer model of tests/key_check_model.py: keys are built from (edited)
exponent lists through G1/G2.of_Fr, uploaded, checked, and the mask must be the model's -- 0 for honest keys whatever the seed, the route the key
came by and the size; the model's bits for every crafted key of tests/key_check_cases.py.  Then the call's contract: the handle is left as it was
found (proof bytes), and every refusal of include/zkmi355x.h."""
import ctypes as C
import functools

import numpy as np
import pytest

import key_check_cases as KC
import key_check_model as KM
from zukelang_amd import _lib, r1cs as RC
from zukelang_amd.curve import G1, G2, Pairing
from zukelang_amd.groth16 import Groth16, PKey, VKey
from zukelang_amd.r1cs import fr_bytes

pytestmark = pytest.mark.gpu

TOX = [0x1111 + 7919 * i + (i << 200) for i in range(1, 6)]
SEEDS = [bytes(range(32)), bytes([0xA5] * 32), (0x0123456789ABCDEF << 192 | 0xFEDCBA9876543210).to_bytes(32, "little")]


def zero_row_circuit():
    """gate 1 has an all-zero row in L (0 * x = 0 * ONE); variable 5 appears in no gate"""
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
    "n5": lambda: RC.random_r1cs(5, 12, 3, nnz=(1, 3))[0],                  # no power of two
    "n13": lambda: RC.random_r1cs(13, 24, 4, nnz=(8, 8))[0],                # no power of two, 8 entries per row
    "n1025": lambda: RC.random_r1cs(1025, 1100, 5, nnz=(8, 8))[0],          # n2 = 2048: the first size whose tree levels leave k_tree_levels_fused
    "zero_row": zero_row_circuit,
}


@functools.lru_cache(maxsize=None)
def circuit(name):
    return CIRCUITS[name]()


@functools.lru_cache(maxsize=None)
def honest(name):
    return KM.honest_exponents(circuit(name), TOX)


def points(ex1, ex2, vk):
    pk = PKey(G1.of_Fr(fr_bytes(ex1)), G2.of_Fr(fr_bytes(ex2)))
    v1 = G1.of_Fr(fr_bytes([vk["one1"]] + vk["ltgm_io"]))
    v2 = G2.of_Fr(fr_bytes([vk["one2"], vk["gm"], vk["d"]]))
    return pk, VKey(bytes(v1[:96]), v1[96:], bytes(v2[:192]), bytes(v2[192:384]), bytes(v2[384:]), Pairing.pairing(bytes(pk.g1[:96]), bytes(pk.g2[:192])))


def device_masks(cs, ex1, ex2, vk, seed=SEEDS[0]):
    pk, vkey = points(ex1, ex2, vk)
    prover = Groth16(cs, pk)
    try:
        return prover.check_key(seed=seed).failed, prover.check_key(vkey, seed=seed).failed
    finally:
        prover.close()


@pytest.fixture(autouse=True)
def _init_and_leave_nothing_behind():
    _lib.check(_lib.lib().zk_init(0))
    yield
    _lib.set_device_list([0])          # ZK_ERR_ARG while any key handle is alive


# ---------------------------------------------------------------- honest keys give 0
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_honest_key_is_well_formed_at_every_size(name):
    cs = circuit(name)
    ex1, ex2, vk = honest(name)
    if name != "n1025":          # the model's O(n^2) interpolation: seconds at 1025, where honest_exponents has run it once already
        assert KM.key_check_mask(cs, ex1, ex2) == 0 and KM.key_check_mask(cs, ex1, ex2, vk) == 0
    assert device_masks(cs, ex1, ex2, vk) == (0, 0)


def test_honest_key_under_every_seed_and_route():
    cs = circuit("readme")
    it = iter(TOX)
    pk, vk = Groth16.keygen(lambda: next(it), cs)
    ex1, ex2, _ = honest("readme")
    assert bytes(pk.g1) == bytes(G1.of_Fr(fr_bytes(ex1)))          # keygen's key IS the model's honest key
    routes = [Groth16(cs, pk)]
    it = iter(TOX)
    gen, gpk, gvk = Groth16.generate(lambda: next(it), cs, form="tau_powers")
    assert bytes(gpk.g1) == bytes(pk.g1) and bytes(gvk.gm) == bytes(vk.gm)
    routes.append(gen)
    routes.append(Groth16.from_compressed(cs, G1.to_compressed_bytes_many(bytes(pk.g1)), G2.to_compressed_bytes_many(bytes(pk.g2))))
    for prover in routes:
        for seed in SEEDS + [None]:
            for v in (None, vk):
                res = prover.check_key(v, seed=seed)
                assert res.ok and res.failed == 0 and res.names == [] and bool(res)
        prover.close()


# ---------------------------------------------------------------- crafted keys give the model's bits
README_CASES = KC.crafted(RC.readme_circuit(3)[0], TOX, readme_other())


@pytest.mark.parametrize("name,ex1,ex2,vk", README_CASES, ids=[c[0] for c in README_CASES])
def test_crafted_readme_keys(name, ex1, ex2, vk):
    cs = circuit("readme")
    want = (KM.key_check_mask(cs, ex1, ex2), KM.key_check_mask(cs, ex1, ex2, vk))
    assert want == KC.BITS[name]
    for seed in SEEDS[:2]:
        assert device_masks(cs, ex1, ex2, vk, seed) == want, name


@pytest.mark.parametrize("size", ["n5", "n13", "zero_row"])
def test_crafted_keys_at_other_sizes(size):
    cs = circuit(size)
    for name, ex1, ex2, vk in KC.crafted(cs, TOX):
        want = (KM.key_check_mask(cs, ex1, ex2), KM.key_check_mask(cs, ex1, ex2, vk))
        assert device_masks(cs, ex1, ex2, vk) == want, name


def test_crafted_keys_at_1025():
    cs = circuit("n1025")
    cases = {c[0]: c for c in KC.crafted(cs, TOX)}
    for name in ("tiztd_one", "ltd_mid_opposite"):
        _, ex1, ex2, vk = cases[name]
        want = KM.key_check_mask(cs, ex1, ex2, vk)
        assert want == KC.BITS[name][1]
        assert device_masks(cs, ex1, ex2, vk)[1] == want, name


def test_generators_gamma_and_ab():
    cs = circuit("readme")
    ex1, ex2, vk = honest("readme")
    e1 = list(ex1)
    e1[3] = 2                                                   # ti1[0] = [2]: every tau relation shifts with it
    assert device_masks(cs, e1, ex2, vk) == (KM.key_check_mask(cs, e1, ex2), KM.key_check_mask(cs, e1, ex2, vk))
    assert KM.key_check_mask(cs, e1, ex2) & KM.GENERATORS
    v = dict(vk, gm=0)
    assert device_masks(cs, ex1, ex2, v)[1] == KM.key_check_mask(cs, ex1, ex2, v) == KM.GAMMA | KM.L
    v = dict(vk, one2=2)
    assert device_masks(cs, ex1, ex2, v)[1] == KM.key_check_mask(cs, ex1, ex2, v) == KM.GENERATORS
    pk, vkey = points(ex1, ex2, vk)
    prover = Groth16(cs, pk)
    vkey.ab = Pairing.pairing(bytes(pk.g1[96:192]), bytes(pk.g2[:192]))          # e(d1, b2): not this key's ab
    res = prover.check_key(vkey)
    assert not res.ok and res.failed == _lib.KEYCHK_AB and res.names == ["ab"]
    prover.close()


# ---------------------------------------------------------------- the contract
def test_the_handle_is_left_as_it_was_found():
    cs, w = RC.readme_circuit(3)
    pk, vkey = points(*honest("readme"))
    prover = Groth16(cs, pk)
    before = prover.prove_rs(w, 5, 7)
    assert prover.check_key(vkey).ok
    after = prover.prove_rs(w, 5, 7)
    assert (before.a, before.b, before.c) == (after.a, after.b, after.c)
    cs2, w2 = RC.random_r1cs(1025, 1100, 5, nnz=(8, 8))
    pk2, vkey2 = points(*honest("n1025"))
    prover2 = Groth16(cs2, pk2)
    before = prover2.prove_rs(w2, 5, 7)
    assert prover2.check_key(vkey2).ok
    after = prover2.prove_rs(w2, 5, 7)
    assert (before.a, before.b, before.c) == (after.a, after.b, after.c)
    prover.close()
    prover2.close()


def _raw(handle, v1, n_io, v2, seed, failed):
    p = lambda b: None if b is None else np.frombuffer(bytes(b), dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    keep = [v1, v2, seed]          # noqa: F841
    return _lib.lib().zk_groth16_key_check(handle, p(v1), n_io, p(v2), p(seed), failed)


def test_refusals():
    cs, w = RC.readme_circuit(3)
    pk, vkey = points(*honest("readme"))
    v1, v2 = bytes(vkey.one1) + bytes(vkey.ltgm_io), bytes(vkey.one2) + bytes(vkey.gm) + bytes(vkey.d)
    n_io = cs.m - cs.n_mid
    failed = C.c_uint32(0)
    prover = Groth16(cs, pk)
    h = prover.handle
    assert _raw(h, v1, n_io, v2, SEEDS[0], C.byref(failed)) == 0 and failed.value == 0
    assert _raw(h, v1, n_io, v2, None, C.byref(failed)) == 0 and failed.value == 0          # the library draws the seed
    assert _raw(h, v1, n_io, v2, SEEDS[0], None) == -1                                        # null failed
    assert _raw(h, v1, n_io, None, SEEDS[0], C.byref(failed)) == -1                           # exactly one of vk_g1 / vk_g2
    assert _raw(h, None, 0, v2, SEEDS[0], C.byref(failed)) == -1
    assert _raw(h, v1[:-96], n_io - 1, v2, SEEDS[0], C.byref(failed)) == -1                   # n_io is not m - |mids|
    assert _raw(C.c_uint64(0xDEAD), v1, n_io, v2, SEEDS[0], C.byref(failed)) == -7            # unknown handle
    bad = bytearray(v1)
    bad[96 + 95] ^= 1                                                                         # ltgm_io[0] off the curve
    assert _raw(h, bytes(bad), n_io, v2, SEEDS[0], C.byref(failed)) == -2
    bad = bytearray(v2)
    bad[192] |= 0x80                                                                          # gm: compression flag on an uncompressed point
    assert _raw(h, v1, n_io, bytes(bad), SEEDS[0], C.byref(failed)) == -1
    prover.prove_async(w, 5, 7, 0)                                                            # a proof in flight
    assert _raw(h, None, 0, None, SEEDS[0], C.byref(failed)) == -1
    prover.prove_wait(0)
    assert _raw(h, None, 0, None, SEEDS[0], C.byref(failed)) == 0 and failed.value == 0
    prover.derive_lagrange()                                                                  # Lagrange form
    assert _raw(h, None, 0, None, SEEDS[0], C.byref(failed)) == -1
    assert b"Lagrange" in _lib.lib().zk_last_error()
    prover.close()
    shard = Groth16(cs, pk, rank=0, world=2)                                                  # a shard
    assert _raw(shard.handle, None, 0, None, SEEDS[0], C.byref(failed)) == -1
    shard.close()
    _lib.check(_lib.lib().zk_set_option(b"key_subgroup_check", b"0"))
    try:
        unchecked = Groth16(cs, pk)
        assert _raw(unchecked.handle, None, 0, None, SEEDS[0], C.byref(failed)) == -1
        assert b"SUBGROUP_CHECK" in _lib.lib().zk_last_error()
        unchecked.close()
    finally:
        _lib.check(_lib.lib().zk_set_option(b"key_subgroup_check", None))
    _lib.set_device_list([0, 0])                                                              # a multi-device handle
    try:
        multi = Groth16(cs, pk)
        assert _raw(multi.handle, None, 0, None, SEEDS[0], C.byref(failed)) == -1
        multi.close()
    finally:
        _lib.set_device_list([0])
