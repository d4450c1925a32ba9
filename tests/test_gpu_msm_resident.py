"""GPU parity of the resident MSM bases (include/zkmi355x.h, "resident MSM bases"): every product of zk_msm_resident / _many == the oracle's left
fold (curve.ml:112-118) == zk_msm_g1/g2 on the same prefix, on both sides of short_max, in both groups; the error contract; sum_apply_powers
(groth16.ml:116-121) against the literal fold."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_lib as O
import ref_programs as RP
from oracle import pyref as P
from zukelang_amd import _lib, curve
from zukelang_amd import r1cs as RC
from zukelang_amd.curve import G1, G2

pytestmark = pytest.mark.gpu

NAIVE = {G1: O.g1_msm_naive, G2: O.g2_msm_naive}
FAST = {G1: O.fast_g1_msm, G2: O.fast_g2_msm}
MUL = {G1: O.g1_mul, G2: O.g2_mul}
ADD = {G1: O.g1_add, G2: O.g2_add}


def frb(x):
    return P.fr_to_bytes(x)


def _short_max(G):
    with G.resident(G.of_Fr(frb(1))) as rb:
        return rb.short_max


def _bases(G, n, seed):
    """n points of the group with the identity, a duplicate and a P, -P pair among them (where n allows)"""
    pts = np.array(G.of_Fr(RC.random_fr_bytes(n, seed)), dtype=np.uint8).reshape(n, G.POINT_BYTES)
    if n >= 3:
        pts[1] = 0
        pts[1, 0] = 0x40                                               # the identity
    if n >= 6:
        pts[4] = pts[3]                                                # a duplicate
        pts[5] = np.frombuffer(MUL[G](bytes(pts[3]), frb(P.R - 1)), dtype=np.uint8)   # -P
    return pts.reshape(-1)


def _scalars(k, seed):
    s = np.array(RC.random_fr_bytes(k, seed), dtype=np.uint8).reshape(k, 32) if k else np.zeros((0, 32), dtype=np.uint8)
    for i, v in zip(range(k), (0, 1, P.R - 1)):
        s[i] = np.frombuffer(frb(v), dtype=np.uint8)
    return s.reshape(-1)


def _oracle(G, bases, scalars, exact=True):
    k = len(scalars) // 32
    pts = bytes(bases[:k * G.POINT_BYTES])
    rc, ref = (NAIVE[G](pts, bytes(scalars)) if exact else FAST[G](pts, bytes(scalars), 16))
    assert rc == 0
    return ref


def _check(G, rb, bases, k, seed, exact=True):
    sc = _scalars(k, seed)
    got = bytes(rb.apply_powers(sc))
    assert got == bytes(G.apply_powers(sc, bases[:max(k, 1) * G.POINT_BYTES] if k else bases)), (k, "zk_msm")
    assert got == _oracle(G, bases, sc, exact), (k, "oracle")
    return sc, got


@pytest.mark.parametrize("G", [G1, G2])
def test_resident_sizes_and_prefixes_match_oracle_and_zk_msm(G):
    sm = _short_max(G)
    assert 1 <= sm <= 8192
    for n in sorted({1, 2, 3, 16, 255, 1024, sm + 1}):
        bases = _bases(G, n, 100 + n)
        with G.resident(bases) as rb:
            assert (rb.n, rb.short_max) == (n, sm)
            for k in sorted({0, 1, sm - 1, sm, sm + 1, n}):
                if k <= n:
                    _check(G, rb, bases, k, 200 + n + k)


@pytest.mark.parametrize("G", [G1, G2])
def test_resident_large_list(G):
    n = 1 << 16
    bases = _bases(G, n, 7)
    sm = _short_max(G)
    with G.resident(bases) as rb:
        for k in (1, sm, sm + 1, 5000, n):
            _check(G, rb, bases, k, 300 + k, exact=k <= 2048)
        cs = [_scalars(k, 800 + k) for k in (2, sm, 1, sm + 1, sm - 1)]          # several short products: the two-launch path
        many = [bytes(p) for p in rb.apply_powers_many(cs)]
        assert many == [bytes(rb.apply_powers(c)) for c in cs]
        assert many == [_oracle(G, bases, c) for c in cs]


@pytest.mark.parametrize("G", [G1, G2])
def test_resident_many_is_k_single_calls(G):
    """the short path (two or more short products in one call) against K single calls (a lone product takes the chain) and the oracle"""
    sm = _short_max(G)
    n = sm + 40
    bases = _bases(G, n, 11)
    lens = [0, 1, 3, sm, sm + 1, 0, 17, n, sm - 1, 2]
    cs = [_scalars(k, 400 + i) for i, k in enumerate(lens)]
    with G.resident(bases) as rb:
        many = [bytes(p) for p in rb.apply_powers_many(cs)]
        single = [bytes(rb.apply_powers(c)) for c in cs]
        assert many == single
        for c, got in zip(cs, many):
            assert got == _oracle(G, bases, c), len(c) // 32
        assert rb.apply_powers_many([]) == []


def test_resident_error_contract():
    L = _lib.lib()
    bases = _bases(G1, 20, 21)
    rb = G1.resident(bases)
    with pytest.raises(ValueError, match="apply_powers"):
        rb.apply_powers(_scalars(21, 1))                                # nscalars > n (curve.ml:116)
    with pytest.raises(ValueError, match="apply_powers"):
        rb.apply_powers_many([_scalars(3, 2), _scalars(21, 3)])
    inf = bytes([0x40]) + bytes(95)
    assert bytes(rb.apply_powers(b"")) == inf                          # curve.ml:115
    for k in (1, 20):                                                   # a scalar >= r: refused, handle still usable
        bad = _scalars(k, 4)
        bad[32 * (k - 1):32 * k] = np.frombuffer(P.R.to_bytes(32, "little"), dtype=np.uint8)      # r itself: not reduced
        with pytest.raises(_lib.ZkError) as e:
            rb.apply_powers(bad)
        assert e.value.code == -3
        with pytest.raises(_lib.ZkError) as e:
            rb.apply_powers_many([_scalars(2, 5), bad])
        assert e.value.code == -3
        _check(G1, rb, bases, k, 6 + k)
    h = rb.handle
    out = np.zeros(96, dtype=np.uint8)
    rb.close()
    sc = _scalars(2, 7)
    assert L.zk_msm_resident(C.c_uint64(h), curve._p(sc), C.c_size_t(2), curve._p(out)) == -7       # freed handle
    assert L.zk_bases_free(C.c_uint64(h)) == -7
    assert L.zk_bases_info(C.c_uint64(12345), None, None, None) == -7
    lens = (C.c_uint64 * 1)(2)
    assert L.zk_msm_resident_many(C.c_uint64(999), curve._p(sc), lens, C.c_uint32(1), curve._p(out)) == -7
    g = C.c_int(-1)
    with G2.resident(_bases(G2, 4, 8)) as r2:
        assert L.zk_bases_info(C.c_uint64(r2.handle), C.byref(g), None, None) == 0 and g.value == 1
    # a live handle pins the device list, as key handles do
    with G1.resident(bases) as r3:
        assert L.zk_set_device_list((C.c_int32 * 2)(0, 0), C.c_uint32(2)) == -1
        assert r3.n == 20


def _point_outside_the_subgroup():
    x = 0
    while True:
        x += 1
        y2 = (x ** 3 + 4) % P.P
        y = pow(y2, (P.P + 1) // 4, P.P)
        if y * y % P.P == y2:
            pt = (P.Fp1(x), P.Fp1(y))
            if P.pt_mul(pt, P.R) is not None:
                return pt


def _set_option(name, value):
    _lib.check(_lib.lib().zk_set_option(name.encode(), None if value is None else str(value).encode()))


def test_resident_upload_checks_and_the_subgroup_option():
    bases = _bases(G1, 40, 31)
    bad = np.array(bases, copy=True)
    bad[96 * 7:96 * 8] = np.frombuffer(P.g1_to_bytes(_point_outside_the_subgroup()), dtype=np.uint8)
    with pytest.raises(_lib.ZkError) as e:
        G1.resident(bad)
    assert e.value.code == -2 and "subgroup" in str(e.value)
    off = np.array(bases, copy=True)
    off[96 * 9 + 95] ^= 1
    with pytest.raises(_lib.ZkError) as e:
        G1.resident(off)
    assert e.value.code == -2
    _set_option("key_subgroup_check", "0")
    try:
        rb = G1.resident(bases)
    finally:
        _set_option("key_subgroup_check", None)
    with rb:                                                             # keeps its upload's verdict: no folded digits, same bytes
        for k in (0, 1, 39, 40):
            _check(G1, rb, bases, k, 500 + k)
        # the short path on this handle: 52 unfolded windows of the narrow table, its own recoding constant (scalars 0, 1, r - 1 lead every vector)
        cs = [_scalars(k, 550 + k) for k in (1, 0, 3, 2, 40, 17)]
        many = [bytes(p) for p in rb.apply_powers_many(cs)]
        for c, got in zip(cs, many):
            k = len(c) // 32
            assert got == _oracle(G1, bases, c), k
            assert got == bytes(G1.apply_powers(c, bases[:max(k, 1) * 96] if k else bases)), k


_FROM_BYTES = {G1: P.g1_from_bytes, G2: P.g2_from_bytes}
_TO_BYTES = {G1: P.g1_to_bytes, G2: P.g2_to_bytes}


@pytest.mark.parametrize("n", [2, 129])
@pytest.mark.parametrize("G", [G1, G2])
def test_zero_bytes_without_the_infinity_bit_are_the_identity_on_the_base_path(G, n):
    """96 / 192 zero bytes, the infinity bit NOT set, as the last base of a list: the decoder of key lists and MSM bases takes the string for the identity
    (it is how the library's own affine format spells it), where the verifiers' decoder calls it a point off the curve (tests/test_gpu_pairing.py,
    tests/test_gpu_subgroup_endo.py).  129 = one lane past a full 128-lane block of the decoder.  A product with a non-zero scalar on EVERY base is the
    product without that base, in oracle/pyref.py's integers (small scalars keep the Python fold short)."""
    pts = np.array(G.of_Fr(RC.random_fr_bytes(n, 60 + n)), dtype=np.uint8).reshape(n, G.POINT_BYTES)
    pts[n - 1] = 0
    scalars = [3 + 5 * i for i in range(n)]
    sc = np.frombuffer(b"".join(frb(s) for s in scalars), dtype=np.uint8)
    want = _TO_BYTES[G](P.msm([_FROM_BYTES[G](bytes(p)) for p in pts[:n - 1]], scalars[:n - 1]))
    with G.resident(pts.reshape(-1)) as rb:          # zk_bases_upload succeeds
        assert rb.n == n
        assert bytes(rb.apply_powers(sc)) == want


def _torsion_point(G):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torsion_points.json")) as f:
        recs = json.load(f)["points"]
    return next(bytes.fromhex(r["hex"]) for r in recs if r["group"] == (0 if G is G1 else 1) and r["verdict"] == 4)


@pytest.mark.parametrize("G", [G1, G2])
def test_bases_upload_reports_by_kind_priority_not_by_position(G):
    """zk_bases_upload reads one flag word per list: a bad encoding beats a point off the curve, and that beats a point outside the subgroup, wherever
    they sit (zk_g1/g2_decompress_batch reports the FIRST bad element instead: tests/test_gpu_decompress.py)."""
    B = G.POINT_BYTES
    good = np.array(G.of_Fr(RC.random_fr_bytes(3, 77)), dtype=np.uint8).reshape(3, B)
    off_curve = np.array(good[0], copy=True)
    off_curve[B - 1] ^= 1
    bad_encoding = np.array(good[2], copy=True)
    bad_encoding[0] |= 0x80                                            # the compression bit on an uncompressed point
    outside = np.frombuffer(_torsion_point(G), dtype=np.uint8)
    assert P.on_curve(_FROM_BYTES[G](bytes(outside)), P.B1 if G is G1 else P.B2) and not P._in_subgroup(_FROM_BYTES[G](bytes(outside)))
    with pytest.raises(_lib.ZkError) as e:
        G.resident(np.concatenate([off_curve, good[1], bad_encoding]))
    assert e.value.code == -1 and "encoding" in str(e.value), str(e.value)
    with pytest.raises(_lib.ZkError) as e:
        G.resident(np.concatenate([outside, good[1], off_curve]))
    assert e.value.code == -2 and "not on the curve" in str(e.value) and "subgroup" not in str(e.value), str(e.value)


def test_interleaved_handles_and_many_random_prefixes():
    sm = _short_max(G1)
    b1, b2, b3 = _bases(G1, 300, 41), _bases(G2, 50, 42), _bases(G1, sm + 8, 43)
    hs = [(G1, G1.resident(b1), b1), (G2, G2.resident(b2), b2), (G1, G1.resident(b3), b3)]
    for G, rb, b in hs:
        _check(G, rb, b, rb.n // 2, 600)
    rng = random.Random(0x5EED)
    G, rb, b = hs[2]
    want = {}
    for it in range(500):
        k = rng.choice([0, 1, 2, sm - 1, sm, sm + 1, rng.randrange(rb.n + 1)])
        sc = _scalars(k, 1000 + (it % 7))
        got = bytes(rb.apply_powers(sc))
        key = (k, it % 7)
        if key not in want:
            want[key] = bytes(G.apply_powers(sc, b)) if k else bytes([0x40]) + bytes(95)
        assert got == want[key], (it, k)
        if it % 100 == 0:
            _check(G1, hs[0][1], b1, rng.randrange(301), 700 + it)
            pair = [_scalars(rng.randrange(1, 51), 900 + it), _scalars(rng.randrange(1, 51), 901 + it)]
            assert [bytes(p) for p in hs[1][1].apply_powers_many(pair)] == [_oracle(G2, b2, c) for c in pair]
    for k in list(want)[:6]:
        assert want[k] == _oracle(G1, b3, _scalars(k[0], 1000 + k[1]))
    for _, rb, _ in hs:
        rb.close()


def _literal_fold(G, ti, ps, w):
    acc = bytes([0x40]) + bytes(G.POINT_BYTES - 1)
    for k in sorted(w):
        cs = bytes(ps[k])
        r = bytes([0x40]) + bytes(G.POINT_BYTES - 1)
        for i in range(len(cs) // 32):
            r = ADD[G](MUL[G](bytes(ti[i * G.POINT_BYTES:(i + 1) * G.POINT_BYTES]), cs[32 * i:32 * i + 32]), r)
        acc = ADD[G](MUL[G](r, bytes(w[k])), acc)
    return acc


@pytest.mark.parametrize("which", ["readme", "ref"])
def test_sum_apply_powers_is_the_literal_fold(which):
    if which == "readme":
        cs, w = RC.readme_circuit(3)
    else:
        p = RP.program(RP.names()[0])
        cs, w = RP.circuit(p), RP.witnesses(p)[0]
    csr = [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
    qap = O.QAP(cs.n, cs.m, *csr)
    tau = 0x1234567
    for G in (G1, G2):
        ti = np.array(G.powers(cs.n + 1, frb(tau)), dtype=np.uint8)           # n + 2 points, as the key's tau basis (groth16.ml:73)
        for which_poly in (0, 1):
            ps = {k: qap.poly(which_poly, k) for k in range(cs.m)}
            wm = {k: frb(v) for k, v in enumerate(w)}
            assert bytes(curve.sum_apply_powers(G, ti, ps, wm)) == _literal_fold(G, ti, ps, wm), (G.__name__, which_poly)


def test_many_across_batches_and_workspace_reuse():
    """more products than one batch holds (256), more scalars than one batch stages (64 full-length products), more long products than
    the four sort workspaces of one chain: every result lands where its product was"""
    G = G1
    sm = _short_max(G)
    n = sm + 8
    bases = _bases(G, n, 61)
    lens = [1] * 300 + [n] * 70 + [sm + 1] * 6 + [0, 2]
    rng = random.Random(62)
    rng.shuffle(lens)
    cs = [_scalars(k, 6000 + i) for i, k in enumerate(lens)]
    with G.resident(bases) as rb:
        many = [bytes(p) for p in rb.apply_powers_many(cs)]
        singles = {}
        for c, got in zip(cs, many):
            key = c.tobytes()
            if key not in singles:
                singles[key] = bytes(rb.apply_powers(c))
            assert got == singles[key], len(c) // 32
        for i in (0, lens.index(n), lens.index(sm + 1), lens.index(1)):
            assert many[i] == _oracle(G, bases, cs[i]), lens[i]


def test_close_after_shutdown_is_quiet(tmp_path):
    """zk_shutdown frees every resident handle; closing the Python object afterwards (or leaving its `with` block) is not an error.  In a child
    process: a shutdown in the suite's own process would free the handles of every other test."""
    import subprocess
    import sys
    code = (
        "import numpy as np\n"
        "from zukelang_amd import _lib\n"
        "from zukelang_amd.curve import G1\n"
        "from zukelang_amd import r1cs as RC\n"
        "pts = G1.of_Fr(RC.random_fr_bytes(8, 1))\n"
        "with G1.resident(pts) as rb:\n"
        "    _lib.check(_lib.lib().zk_shutdown())\n"
        "rb.close()\n"
        "with G1.resident(pts) as rb2:\n"
        "    assert bytes(rb2.apply_powers(RC.random_fr_bytes(8, 2))) == bytes(G1.apply_powers(RC.random_fr_bytes(8, 2), pts))\n"
        "print('ok')\n")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
