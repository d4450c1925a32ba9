"""GPU parity: zk_fr_ntt (HIP) == the oracle's restatement of FFT.ml:29-86, bit-exact."""
import random

import numpy as np
import pytest

import oracle_lib as O
from zukelang_amd import r1cs as RC
from zukelang_amd.curve import FFT_Fr

pytestmark = pytest.mark.gpu


def _rand_fr(n, seed):
    return bytes(RC.random_fr_bytes(n, seed))


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 8, 10, 11, 12, 13, 16, 6, 7, 9, 15, 17, 19])
def test_fft_matches_oracle(log_n):
    """Every pass plan of ntt.hip: one tile of fewer than 1024 elements with an odd or an even stage count (6, 7, 9), one strided pass of 5 or 7 stages
    in front of the tile (15, 17), and 19 -- the smallest size with two strided passes of unequal length (5 + 4 stages, row steps 2^5 and 2^6)."""
    data = _rand_fr(1 << log_n, 100 + log_n)
    assert bytes(FFT_Fr.fft(data, log_n)) == O.fr_ntt(data, log_n, False)
    assert bytes(FFT_Fr.ifft(data)) == O.fr_ntt(data, log_n, True)


@pytest.mark.parametrize("log_n", [4, 10, 12, 14, 19])
def test_fft_extreme_values(log_n):
    """Largest residues everywhere (and sparse mixes of 0, 1, r - 1): the lazily reduced 29-bit-limb butterflies
    (csrc/fr29.cuh) run at the top of their value bounds."""
    n = 1 << log_n
    top = (RC.FR_MODULUS - 1).to_bytes(32, "little")
    rnd = random.Random(7 + log_n)
    pool = [top, bytes(32), (1).to_bytes(32, "little"), (RC.FR_MODULUS - 2).to_bytes(32, "little"), ((1 << 254) + 5).to_bytes(32, "little")]
    patterns = [top * n, b"".join(rnd.choice(pool) for _ in range(n)), b"".join(top if i & 1 else bytes(32) for i in range(n))]
    if log_n == 19:          # the uneven two-pass plan: the oracle's six transforms of 2^19 cost more than any other case of this file, so without the alternating pattern
        patterns = patterns[:2]
    for data in patterns:
        assert bytes(FFT_Fr.fft(data, log_n)) == O.fr_ntt(data, log_n, False)
        assert bytes(FFT_Fr.ifft(data)) == O.fr_ntt(data, log_n, True)


@pytest.mark.parametrize("log_n", [18, 20, 22])
def test_fft_roundtrip_and_linearity_large(log_n):
    """Full benchmark sizes: fft o ifft = id (FFT.ml:88-96) and linearity -- size-independent."""
    n = 1 << log_n
    a = RC.random_fr_bytes(n, 7)
    b = RC.random_fr_bytes(n, 8)
    fa = FFT_Fr.fft(a, log_n)
    assert bytes(FFT_Fr.ifft(fa)) == bytes(a)
    # spot-check 4 outputs against the definition sum_j a_j w^(jk) using the oracle on a folded input:
    # out[k] for k = 0 is the plain sum of the inputs
    ints = np.frombuffer(bytes(a), dtype=np.uint8).reshape(n, 32)
    total = sum(int.from_bytes(bytes(row), "little") for row in ints[:: max(1, n // 4096)]) if n <= 1 << 12 else None
    if total is not None:
        assert int.from_bytes(bytes(fa[:32]), "little") == total % RC.FR_MODULUS
    # linearity: fft(a) + fft(b) == fft(a + b) checked on a strided sample
    fb = FFT_Fr.fft(b, log_n)
    P = RC.FR_MODULUS
    idx = random.Random(log_n).sample(range(n), 64)
    s = bytearray()
    A = np.frombuffer(bytes(a), dtype=np.uint8).reshape(n, 32)
    B = np.frombuffer(bytes(b), dtype=np.uint8).reshape(n, 32)
    # a + b computed with numpy object ints only on the host for the whole vector is slow; do it in C-order chunks
    ai = [int.from_bytes(bytes(r), "little") for r in A]
    bi = [int.from_bytes(bytes(r), "little") for r in B]
    ab = RC.fr_bytes([(x + y) % P for x, y in zip(ai, bi)])
    fab = FFT_Fr.fft(ab, log_n)
    for k in idx:
        x = int.from_bytes(bytes(fa[32 * k:32 * k + 32]), "little")
        y = int.from_bytes(bytes(fb[32 * k:32 * k + 32]), "little")
        z = int.from_bytes(bytes(fab[32 * k:32 * k + 32]), "little")
        assert (x + y) % P == z


def test_non_canonical_input_is_rejected():
    from zukelang_amd._lib import ZkError
    bad = (RC.FR_MODULUS).to_bytes(32, "little") + bytes(32)
    with pytest.raises(ZkError) as e:
        FFT_Fr.fft(bad, 1)
    assert e.value.code == -3


@pytest.mark.parametrize("log_n", [18, 20])
def test_fft_large_matches_oracle_on_a_strided_sample(log_n):
    """beyond 2^16 the transform was property-tested only.  The oracle's O(n log n) restatement of
    FFT.ml:29-67 handles 2^20 in seconds: compare 256 strided outputs (plus both ends) of fft and ifft bit for bit."""
    n = 1 << log_n
    data = _rand_fr(n, 900 + log_n)
    for inverse, got in ((False, bytes(FFT_Fr.fft(data, log_n))), (True, bytes(FFT_Fr.ifft(data)))):
        ref = O.fr_ntt(data, log_n, inverse)
        idx = list(range(0, n, n // 256)) + [1, n - 1, n // 2 + 1]
        for k in idx:
            assert got[32 * k:32 * k + 32] == ref[32 * k:32 * k + 32], (log_n, inverse, k)
        if log_n == 18:
            assert got == ref


@pytest.mark.parametrize("na,nb", [(1, 1), (1, 7), (2, 2), (3, 5), (17, 1), (64, 64), (100, 29), (255, 257), (1000, 1), (1024, 1024), (4096, 3000), (4096, 4096)])
def test_polynomial_mul_matches_oracle(na, nb):
    """zk_fr_poly_mul == FFT.polynomial_mul (FFT.ml:98-105) == Polynomial.mul (polynomial.ml:124-131, the oracle's
    schoolbook restatement): unequal lengths, sizes that are not powers of two, normalized output."""
    a, b = _rand_fr(na, 5000 + na), _rand_fr(nb, 6000 + nb)
    assert bytes(FFT_Fr.polynomial_mul(a, b)) == O.poly_mul(a, b)
    assert bytes(FFT_Fr.polynomial_mul(b, a)) == O.poly_mul(a, b)


def _horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % RC.FR_MODULUS
    return acc


@pytest.mark.parametrize("na,nb", [(9000, 5000), (20000, 9001), (70000, 50001), (300000, 100000), (262145, 1), (262144, 262145)])
def test_polynomial_mul_large_by_evaluation(na, nb):
    """zk_fr_poly_mul beyond the reach of the schoolbook oracle: transforms of 2^14, 2^15, 2^17 and 2^19 (the data-form table of ntt_mul_table, k_ntt_mid
    between strided passes), (262145, 1) one coefficient past 2^18 and na + nb - 1 = 2^19 exactly.  c(x) = a(x) b(x) mod r at two points from a fixed
    seed (a wrong coefficient survives one evaluation with probability below 2^19 / r), the two end coefficients exactly, one middle coefficient by
    its defining sum, and the length."""
    P = RC.FR_MODULUS
    n = na + nb - 1
    assert 1 << ((n - 1).bit_length()) in (1 << 14, 1 << 15, 1 << 17, 1 << 19)
    a, b = RC.fr_ints(_rand_fr(na, 15000 + na)), RC.fr_ints(_rand_fr(nb, 16000 + nb))
    a[0], b[0] = a[0] or 1, b[0] or 1
    a[-1], b[-1] = a[-1] or 1, b[-1] or 1                     # no trailing zero: the normalized product has every one of its n coefficients
    got = bytes(FFT_Fr.polynomial_mul(RC.fr_bytes(a), RC.fr_bytes(b)))
    assert len(got) == 32 * n
    c = RC.fr_ints(got)
    assert all(v < P for v in c[:: max(1, n // 1024)])
    assert c[0] == a[0] * b[0] % P and c[n - 1] == a[-1] * b[-1] % P
    k = n // 2 + 1
    assert c[k] == sum(a[i] * b[k - i] for i in range(max(0, k - nb + 1), min(na, k + 1))) % P
    rnd = random.Random(0xE7A1 + na)
    for _ in range(2):
        x = rnd.randrange(2, P)
        assert _horner(c, x) == _horner(a, x) * _horner(b, x) % P
    if nb == 1:
        assert c == [v * b[0] % P for v in a]


def test_polynomial_mul_normalizes_like_the_reference():
    """Polynomial.normalize (polynomial.ml:100-107): trailing zero coefficients are stripped, the zero polynomial is []."""
    one = (1).to_bytes(32, "little")
    zero = bytes(32)
    top = (RC.FR_MODULUS - 1).to_bytes(32, "little")
    a = _rand_fr(9, 1) + zero * 7                      # trailing zeros in an operand
    b = _rand_fr(5, 2) + zero * 3
    ref = O.poly_mul(a, b)
    assert bytes(FFT_Fr.polynomial_mul(a, b)) == ref and len(ref) == 32 * (9 + 5 - 1)
    assert bytes(FFT_Fr.polynomial_mul(zero * 4, a)) == b"" == O.poly_mul(zero * 4, a)      # 0 * f = []
    assert bytes(FFT_Fr.polynomial_mul(b"", a)) == b""
    assert bytes(FFT_Fr.polynomial_mul(one, a)) == O.poly_mul(one, a) == a[:32 * 9]
    assert bytes(FFT_Fr.polynomial_mul(top * 33, top * 31)) == O.poly_mul(top * 33, top * 31)   # extreme values: (r-1)^2 sums
    # polynomial.ml:135-139 KAT over Fr: (1 + x)(1 - x) = 1 - x^2
    p1, p2 = one + one, one + top
    assert bytes(FFT_Fr.polynomial_mul(p1, p2)) == one + zero + top


def test_rns_convolution_engine_gives_the_same_field_elements():
    """csrc/rns_ntt.hip (round 4, an OPTION: ZK_FR_RNS=1 when a key is uploaded): the products of the Fr stage as integer convolutions modulo 18 NTT-friendly
    31-bit primes, carried back to Fr by the Chinese remainder theorem -- exact arithmetic, so Polynomial.mul (polynomial.ml:124-131), QAP.eval
    (QAP.ml:120-135) and the proofs (groth16.ml:123-161) must come out byte for byte as through the Fr transforms: polynomial products incl. the extreme
    values (r-1)^2 sums, tau-power keys below and above the fused tree levels (n = 4096: levels 11, 12 go through the residue system), a Lagrange-form
    key, 2^16 constraints, Pinocchio."""
    import os
    from oracle import pyref as P
    from zukelang_amd import pinocchio as PIN
    from zukelang_amd.groth16 import Groth16
    old = os.environ.get("ZK_FR_RNS")
    os.environ["ZK_FR_RNS"] = "1"
    try:
        top = (RC.FR_MODULUS - 1).to_bytes(32, "little")
        for na, nb in ((1, 7), (3, 5), (100, 29), (255, 257), (1024, 1024), (4096, 3000), (20000, 12000)):
            a, b = _rand_fr(na, 7000 + na), _rand_fr(nb, 8000 + nb)
            if na * nb <= 4096 * 4096:
                assert bytes(FFT_Fr.polynomial_mul(a, b)) == O.poly_mul(a, b), (na, nb)
            else:                                   # too long for the oracle's schoolbook product: against the Fr transforms
                os.environ["ZK_FR_RNS"] = "0"
                ref = bytes(FFT_Fr.polynomial_mul(a, b))
                os.environ["ZK_FR_RNS"] = "1"
                assert bytes(FFT_Fr.polynomial_mul(a, b)) == ref, (na, nb)
        assert bytes(FFT_Fr.polynomial_mul(top * 1500, top * 1400)) == O.poly_mul(top * 1500, top * 1400)
        frs = lambda xs: b"".join(P.fr_to_bytes(x) for x in xs)
        for n in (2, 6, 300, 1000, 4096, 1 << 16):
            cs, w = RC.iterated_cubic(n, 0x515 + n)
            st = P.fr_stream(0x5EED0A00 + n)
            toxic = [next(st) for _ in range(5)]
            it = iter(toxic)
            pk, _ = Groth16.keygen(lambda: next(it), cs, lagrange=True)
            csr = [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
            r, s = next(st), next(st)
            exp = O.groth16_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), frs(toxic), P.fr_to_bytes(r), P.fr_to_bytes(s))
            for lag in (False, True):
                prover = Groth16(cs, pk, lagrange=lag)          # the switch is read when the key is uploaded (tables) and per proof
                got = prover.prove_rs(w, r, s)
                assert (got.a, got.b, got.c) == exp, (n, lag)
                if not lag and n <= 4096:
                    os.environ["ZK_FR_RNS"] = "0"
                    ref = [bytes(x) for x in prover.qap_eval(w)]          # the SAME key through the Fr transforms
                    os.environ["ZK_FR_RNS"] = "1"
                    assert [bytes(x) for x in prover.qap_eval(w)] == ref, n
                w_bad = list(w)
                w_bad[n // 2] = (w_bad[n // 2] + 1) % RC.FR_MODULUS
                with pytest.raises(AssertionError):
                    prover.prove_rs(w_bad, r, s)
                prover.close()
        cs, w = RC.iterated_cubic(1000, 11)
        st = P.fr_stream(0x5EED0003)
        tox = [next(st) for _ in range(11)]
        it = iter(tox)
        pk, _ = PIN.ZK.keygen(lambda: next(it), cs)
        prover = PIN.ZK(cs, pk)
        proof = prover.prove(lambda: next(it), w)
        csr = [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
        assert proof.to_bytes() == O.pinocchio_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), frs(tox[:8]), *(P.fr_to_bytes(x) for x in tox[8:]))
        prover.close()
    finally:
        if old is None:
            os.environ.pop("ZK_FR_RNS", None)
        else:
            os.environ["ZK_FR_RNS"] = old
