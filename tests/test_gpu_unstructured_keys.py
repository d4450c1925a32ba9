"""Keys with no trapdoor behind them.  The reference's provers use the points of a key AS GIVEN (groth16.ml:116-161, pinocchio.ml:481-486): nothing in
them asks for a tau, alpha, beta or delta.  Here EVERY point of a key is an independent subgroup point -- G.of_Fr of seeded scalars, with a sprinkling
of identities, of repeated points and of P / -P pairs inside one pool -- so any short cut of the library that is valid only for keys a generator made
(a relation between pools, a pool rebuilt from another, a sort shared between pools with different identity patterns) shows as a proof that differs
from the literal oracle's on the same key bytes.  Exact bytes, every form the library proves in."""
import os

import numpy as np
import pytest

import oracle_lib as O
from oracle import pyref as P
from zukelang_amd import _lib, r1cs as RC
from zukelang_amd import pinocchio as PIN
from zukelang_amd.curve import G1, G2
from zukelang_amd.groth16 import Groth16, PKey
from test_gpu_multidevice import devices  # noqa: F401  (the fixture that restores the one-entry device list)

pytestmark = pytest.mark.gpu


def frs(xs):
    return b"".join(P.fr_to_bytes(x) for x in xs)


def csrs(cs):
    return [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]


def unstructured_points(grp, count, seed):
    """count independent subgroup points: seeded scalars, with (where the pool is long enough) identities, a repeated point and a P / -P pair."""
    st = P.fr_stream(seed)
    ks = [next(st) or 1 for _ in range(count)]
    if count >= 8:
        ks[2] = 0                                  # the identity
        ks[count - 2] = 0
        ks[5] = ks[1]                              # a repeated point
        ks[6] = (P.R - ks[3]) % P.R                # P and -P in one pool
    stats = {"identities": ks.count(0), "repeats": len(ks) - len(set(ks)), "negations": sum(1 for k in ks if k and (P.R - k) in ks)}
    return grp.of_Fr(RC.fr_bytes(ks)), stats


@pytest.mark.parametrize("maker,literal", [(lambda: RC.readme_circuit(3), 1), (lambda: RC.random_r1cs(24, 40, 0x6A11), 1), (lambda: RC.iterated_cubic(64, 0x6A12), 1),
                                           (lambda: RC.iterated_cubic(2048, 0x6A13), 0)])
def test_groth16_proves_from_a_key_of_independent_points(devices, maker, literal):
    cs, w = maker()
    n, m = cs.n, cs.m
    nm = sum(1 for k in range(m) if cs.mid[k])
    g1, s1 = unstructured_points(G1, 3 + (n + 2) + (n - 1) + nm, 0x0175 + n)
    g2, s2 = unstructured_points(G2, 2 + n + 2, 0x0275 + n)
    if n >= 24:
        assert all(s1.values()) and all(s2.values()), (s1, s2)
    pk = PKey(g1, g2)
    q = O.QAP(n, m, *csrs(cs))
    st = P.fr_stream(0x0375 + n)
    rs = [(next(st), next(st)) for _ in range(3)]
    want = []
    for r, s in rs:
        rc, a, b, c = q.groth16_prove(bytes(g1), bytes(g2), cs.mid, frs(w), P.fr_to_bytes(r), P.fr_to_bytes(s), literal)
        assert rc == 0
        want.append((a, b, c))
    abc = lambda p: (p.a, p.b, p.c)

    def run(prover, tag):
        assert [abc(prover.prove_rs(w, r, s)) for r, s in rs] == want, tag
        prover.set_witness(w)
        for slot, (r, s) in enumerate(rs):                                  # three pipelined slots
            prover.prove_async(None, r, s, slot)
        assert [abc(prover.prove_wait(slot)) for slot in range(len(rs))] == want, tag + ", pipelined"

    prover = Groth16(cs, pk)
    try:
        assert bytes(prover.pool_points(1)) == bytes(g1) and bytes(prover.pool_points(2)) == bytes(g2)
        run(prover, "as uploaded")
        old = os.environ.get("ZK_GRAPH")
        os.environ["ZK_GRAPH"] = "1"
        try:
            run(prover, "graph capture")
            run(prover, "graph replay")
        finally:
            if old is None:
                os.environ.pop("ZK_GRAPH", None)
            else:
                os.environ["ZK_GRAPH"] = old
        prover.derive_lagrange()                                            # linear in the points: the bytes must not move
        run(prover, "derived")
    finally:
        prover.close()
    devices([0, 0])
    prover = Groth16(cs, pk)
    try:
        run(prover, "device list [0, 0]")
        prover.derive_lagrange()
        run(prover, "device list [0, 0], derived")
    finally:
        prover.close()


@pytest.mark.parametrize("maker", [lambda: RC.readme_circuit(3), lambda: RC.random_r1cs(24, 40, 0x6A21), lambda: RC.iterated_cubic(64, 0x6A22)])
def test_pinocchio_proves_from_a_key_of_independent_points(devices, maker):
    """Such a key cannot pass the upload's consistency check of v_all | w_all against si: it keeps its full h pool and is used point by point as
    ZKCompute.f uses it (ZK: three blinding scalars; NonZK: all zero)."""
    cs, w = maker()
    n, m = cs.n, cs.m
    assert n <= 64                                                          # the literal oracle is the only one that takes key bytes
    nm = sum(1 for k in range(m) if cs.mid[k])
    g1, s1 = unstructured_points(G1, 5 * nm + (n + 1) + 2 * m + 7, 0x0475 + n)
    g2, s2 = unstructured_points(G2, 2 * nm + (n + 1) + 2, 0x0575 + n)
    assert all(s1.values()) and all(s2.values()), (s1, s2)
    # ONE point of an evaluation key is not free: ZKCompute.f subtracts `one * dy` with one = G1.one, the generator, not a point of the key
    # (pinocchio.ml:485), and the library lets that term ride on si[0].  With si[0] an arbitrary point the library's h differed from the literal
    # oracle's whenever dy != 0 (found by this test); zk_pinocchio_pk_upload now refuses such a key (a documented precondition, true of every key
    # KeyGen.generate makes) instead of proving other bytes from it.  Everything else stays independent.
    with pytest.raises(_lib.ZkError) as refusal:
        PIN.ZK(cs, PIN.PKey(g1, g2))
    assert refusal.value.code == -1 and "si[0]" in str(refusal.value)
    _lib.set_device_list([0])                                               # no handle left behind
    g1 = np.array(g1, copy=True)
    g1[96 * 5 * nm:96 * (5 * nm + 1)] = np.frombuffer(P.g1_to_bytes(P.G1), dtype=np.uint8)
    key = PIN.PKey(g1, g2)
    q = O.QAP(n, m, *csrs(cs))
    st = P.fr_stream(0x0675 + n)
    ds = [[next(st) for _ in range(3)] for _ in range(2)] + [[0, 0, 0]]     # ZK, ZK, NonZK
    want = []
    for d in ds:
        rc, ref = O.pinocchio_prove(q, bytes(g1), bytes(g2), cs.mid, frs(w), *(P.fr_to_bytes(x) for x in d))
        assert rc == 0
        want.append(ref)
    assert want[0] != want[2]

    def run(prover, tag):
        assert [prover.prove_with(w, *d).to_bytes() for d in ds] == want, tag
        prover.set_witness(w)
        for slot, d in enumerate(ds):
            prover.prove_async(*d, slot)
        assert [prover.prove_wait(slot).to_bytes() for slot in range(len(ds))] == want, tag + ", pipelined"

    prover = PIN.ZK(cs, key)
    try:
        assert bytes(prover.pool_points(5)) == bytes(g1[96 * 5 * nm:96 * (5 * nm + n + 1 + 2 * m)]), "a key that is not the image of its si keeps its full h pool"
        run(prover, "as uploaded")
        prover.derive_lagrange()
        assert prover.pool_size(5) == n + 1 + 2 * m
        run(prover, "derived")
    finally:
        prover.close()
    nz = PIN.NonZK(cs, key)
    try:
        assert nz.prove(None, w).to_bytes() == want[2]
    finally:
        nz.close()
    devices([0, 0])
    prover = PIN.ZK(cs, key)
    try:
        run(prover, "device list [0, 0]")
        prover.derive_lagrange()
        run(prover, "device list [0, 0], derived")
    finally:
        prover.close()
