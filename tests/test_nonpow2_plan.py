"""CPU half of the non-power-of-two cases (tests/nonpow2_cases.py): the restated plan of the Fr stage is the library's (by text), every size of the
table does what its reason says (a change of NTT_LOG_T, FCH or LEAD_BLOCKS that hollows a case out fails HERE), the product formula interpolates, and the
six degenerate witnesses are what their names say on the oracle alone: literal QAP.eval / prove == trapdoor prove (QAP.ml:120-135, groth16.ml:123-161,
pinocchio.ml:427-514)."""
import os
import re

import pytest

import nonpow2_cases as NP
import oracle_lib as O
from oracle import pyref as P
from zukelang_amd import r1cs as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = RC.FR_MODULUS
frb = P.fr_to_bytes
frs = lambda xs: bytes(RC.fr_bytes(xs))
csrs = lambda cs: [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]


def _src(name):
    return open(os.path.join(ROOT, "zukelang_amd", "csrc", name)).read()


def test_the_restated_plan_is_the_librarys():
    lds, fr, cuh, ntt = _src("ntt_lds.cuh"), _src("frstage.hip"), _src("frstage.cuh"), _src("ntt.hip")
    assert "static constexpr int NTT_LOG_T = %d;" % NP.NTT_LOG_T in lds and "static constexpr int NTT_T = 1 << NTT_LOG_T;" in lds
    assert "static constexpr uint32_t FCH = %d;" % NP.FCH in fr
    assert "static constexpr uint32_t LEAD_THREADS = %d;" % NP.LEAD_THREADS in fr
    assert "static constexpr uint32_t LEAD_BLOCKS = %d;" % NP.LEAD_BLOCKS in cuh
    for line in (
            "f.log_n2 = ceil_log2(n); f.n2 = 1u << f.log_n2;",
            "f.log_S = f.log_n2 + 1; f.S = 1u << f.log_S;",
            "f.rns_first_level = (f.log_n2 < (uint32_t)NTT_LOG_T ? f.log_n2 : (uint32_t)NTT_LOG_T) + 1;",
            "        if (n == n2) {\n            HIPCHK(hipMemcpyAsync(f.z.p, q.p, 32 * (size_t)n, hipMemcpyDeviceToDevice, s));",
            "            ZKCHK(tree_convert(f, sc0.d.p, 1, f.log_n2, sc0.tmp.p, s));",
            "const uint64_t need = n - 1;",
            "while (prec < need) {",
            "uint64_t p2 = prec * 2 < need ? prec * 2 : need;",
            "if (got < p2) HIPCHK(hipMemsetAsync(",
            # tree_convert: the fused levels and the loop over the rest
            "const uint32_t log_T = log_total < (uint32_t)NTT_LOG_T ? log_total : NTT_LOG_T;",
            "const uint32_t fused = levels < log_T ? levels : log_T;",
            "for (uint32_t l = fused + 1; l <= levels; l++) {",
            "l >= f.rns_first_level",
            # k_zt
            "const uint32_t lo = c * FCH, hi = min((c + 1) * FCH, cnt);",
            "const uint32_t j0 = n + lo, ch = j0 / FCH;",
            "for (uint32_t e = ch * FCH; e <= j0; e++)",
            "g1d((n - 1 + FCH - 1) / FCH, 64), dim3(64), 0, s, FRP(f.zt), (const uint32_t*)FRP(prod), (const uint32_t*)FRP(f.invfact), n, n - 1);",
            # k_lag_scale / k_lead_partial: the sign of c_i
            "if ((n - 1 - i) & 1) r = fe_neg(r);",
            "if ((n - 1 - i) & 1) c = fe_neg(c);",
            # the leading coefficients
            "for (uint64_t i = (uint64_t)blockIdx.x * LEAD_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LEAD_THREADS) {",
            "uint32_t blocks = (n + LEAD_THREADS - 1) / LEAD_THREADS;",
            "if (blocks > LEAD_BLOCKS) blocks = LEAD_BLOCKS;",
            # the two windows of the quotient
            "(uint64_t)(2 * (uint64_t)n - 2), (uint64_t)n - 1, (uint64_t)S);",
            "(uint64_t)n - 2, (uint64_t)n - 1, (uint64_t)n - 1);"):
        assert line in fr, line
    for line in ("uint32_t s_last = log_len < log_T ? log_len : log_T;", "const uint32_t smax = log_T - 2;", "uint32_t np = (rem + smax - 1) / smax;",
                 "uint32_t s = (rem + (np - p) - 1) / (np - p);"):
        assert line in ntt, line
    assert re.search(r"static inline uint32_t ceil_log2\(uint64_t x\) \{\s*uint32_t l = 0;\s*while \(\(\(uint64_t\)1 << l\) < x\) l\+\+;\s*return l;", _src("zk_common.h"))
    assert [NP.ceil_log2(n) for n in (1, 2, 3, 1024, 1025, 2047, 2048, 40000)] == [0, 1, 2, 10, 11, 11, 11, 16]


def test_every_size_does_what_its_reason_says():
    T = 1 << NP.NTT_LOG_T
    pl = {n: NP.plan(n) for n in NP.SIZES}
    assert sorted(NP.SIZES) == [1025, 2047, 3000, 8193, 40000]
    for n, p in pl.items():
        assert p["z_from_newton"] and p["n2"] > T and p["unfused_levels"], n            # Z through tree_convert, and its loop over unfused levels runs
        assert p["unfused_levels"][0] == p["rns_first_level"] == NP.NTT_LOG_T + 1
        assert p["passes_S"][0], n                                                   # a strided pass in front of the tile
    # the power-series inverse ends on a step that is no doubling wherever n - 1 is no power of two: three of the five sizes (1025 and 8193 have
    # n - 1 = 2^k; they are in the table for the tree)
    assert [n for n, p in sorted(pl.items()) if not p["last_inverse_step_is_a_doubling"]] == [2047, 3000, 40000]
    # the largest counts the other files collect stay inside one tile: what this table adds
    for n in (600, 1000):
        p = NP.plan(n)
        assert p["n2"] == T and not p["unfused_levels"] and p["z_from_newton"]
    for n in (2048, 4096, 1 << 16):
        p = NP.plan(n)
        assert not p["z_from_newton"]                                                # Z is a copy of the root product: all the suite had above one tile
    p = pl[1025]
    assert p["n"] & 1 and p["unfused_levels"] == [11] and p["log_S"] == 12 and p["empty_leaves"] == 1023
    assert NP.plan(1024)["unfused_levels"] == []                                     # ... the FIRST size with one
    p = pl[2047]
    assert p["n"] & 1 and p["empty_leaves"] == 1 and p["unfused_levels"] == [11] and p["inverse_precisions"][-2:] == [1024, 2046]
    p = pl[3000]
    assert not p["n"] & 1 and p["inverse_precisions"][-2:] == [2048, 2999] and 3000 % NP.FCH and p["unfused_levels"] == [11, 12]
    assert p["zt_ragged"] and p["zt_chunks"] == 12 and p["zt_last_chunk"] == 2999 - 11 * 256 and p["zt_catch_up_steps"] == 3000 % 256 + 1 > 1
    p = pl[8193]
    assert p["n"] & 1 and p["unfused_levels"] == [11, 12, 13, 14] and p["log_S"] == 15 and p["passes_S"] == ([5], 10) and p["zt_catch_up_steps"] == 2
    p = pl[40000]
    assert p["log_S"] == 17 and p["lead_blocks"] == NP.LEAD_BLOCKS and (p["lead_full_trips"], p["lead_tail"]) == (1, 7232)
    assert 0 < p["lead_tail"] < NP.LEAD_BLOCKS * NP.LEAD_THREADS                      # two trips, the second partial
    assert p["zt_catch_up_steps"] == 40000 % 256 + 1 > 1 and p["zt_ragged"]
    # every size: k_zt's catch-up loop runs more than one step; the old power-of-two sizes: exactly one
    assert all(q["zt_catch_up_steps"] > 1 for q in pl.values()) and NP.plan(2048)["zt_catch_up_steps"] == 1
    # below the cap one trip, at 2^16 exactly two full ones (what the suite had)
    assert (NP.plan(3000)["lead_full_trips"], NP.plan(3000)["lead_tail"], NP.plan(3000)["lead_blocks"]) == (0, 3000, 12)
    assert (NP.plan(1 << 16)["lead_full_trips"], NP.plan(1 << 16)["lead_tail"]) == (2, 0)


def test_inverse_precisions_are_the_newton_iterations():
    """the sequence restated from `while (prec < need)`: doublings, then one last step to n - 1"""
    assert NP.plan(1025)["inverse_precisions"] == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]            # need = 1024: every step doubles
    assert NP.plan(2047)["inverse_precisions"][-3:] == [512, 1024, 2046]
    assert NP.plan(8193)["inverse_precisions"][-2:] == [4096, 8192]
    assert NP.plan(40000)["inverse_precisions"][-2:] == [32768, 39999]


@pytest.mark.parametrize("n", [1, 2, 7, 33])
def test_product_formula_interpolates(n):
    st = P.fr_stream(0xE7A1 + n)
    coeffs = [next(st) for _ in range(n)]
    values = [NP.horner(coeffs, i) for i in range(n)]
    for x in (next(st), 0, n - 1, n, R - 1):
        assert NP.eval_by_values(values, x) == NP.horner(coeffs, x)
        lag, z = NP.product_formula(n, 0, x, range(n))
        assert z == NP.vanishing_at(n, x) and sum(lag.values()) % R == 1
    # one value through a plain loop with its own inversion
    x = next(st)
    for i in {0, n // 2, n - 1}:
        num = den = 1
        for j in range(n):
            if j != i:
                num, den = num * (x - j) % R, den * (i - j) % R
        assert NP.product_formula(n, 0, x, [i])[0][i] == num * pow(den, R - 2, R) % R


def test_free_circuit_shape():
    cs = NP.free_circuit(5)
    assert (cs.n, cs.m) == (5, 16) and [k for k in range(cs.m) if not cs.mid[k]] == [0, 15]
    assert 0 not in set(cs.L.col) | set(cs.R.col) | set(cs.O.col)                   # ONE occurs in no row
    w = NP.witness_of([2, 3, 4, 5, 6], [7, 8, 9, 10, 11])
    assert cs.check(w) and NP.sparse_products(cs, w) == [[2, 3, 4, 5, 6], [7, 8, 9, 10, 11], [14, 24, 36, 50, 66]]
    w[15] += 1
    assert not cs.check(w)


@pytest.mark.parametrize("n", [2, 8, 33])
@pytest.mark.parametrize("name", list(NP.DEGENERATE))
def test_degenerate_witnesses_on_the_oracle(name, n):
    cs = NP.free_circuit(n)
    w, kind = NP.degenerate_witness(name, n)
    assert cs.check(w)
    sol = frs(w)
    q = O.QAP(cs.n, cs.m, *csrs(cs))
    rc, p_ref, h_ref = q.eval(sol)
    assert rc == 0
    h = RC.fr_ints(h_ref)
    if kind == "zero":
        assert h == []
    elif kind == "one":
        assert h == [1]
    else:
        assert len(h) == n - 1 and all(h)
    v_ref, w_ref, y_ref = q.eval_vwy(sol)
    a, b, c = NP.sparse_products(cs, w)
    for x in (5, n + 3, R - 2):
        assert NP.horner(RC.fr_ints(v_ref), x) == NP.eval_by_values(a, x) and NP.horner(RC.fr_ints(w_ref), x) == NP.eval_by_values(b, x)
        assert NP.horner(RC.fr_ints(y_ref), x) == NP.eval_by_values(c, x)
    if name == "zero":
        assert not any(v_ref) and not any(w_ref) and not any(y_ref) and not any(sol)
    if name == "v_constant":
        assert any(v_ref) and any(w_ref) and any(y_ref)
    st = P.fr_stream(0xDE6E + n)
    tox = [next(st) for _ in range(5)]
    r, s = frb(next(st)), frb(next(st))
    pk1, pk2, _, _ = q.groth16_setup(frs(tox), cs.mid)
    rc, pa, pb, pc = q.groth16_prove(pk1, pk2, cs.mid, sol, r, s, 1)
    assert rc == 0 and (pa, pb, pc) == O.groth16_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, sol, frs(tox), r, s)
    if n <= 16:                                                                     # the literal Pinocchio oracle's reach (tests/test_random_r1cs.py)
        ptox = [next(st) for _ in range(8)]
        ex = O.pinocchio_keygen_exponents(q, cs.n, cs.m, *csrs(cs), cs.mid, frs(ptox), True)
        ppk1, ppk2 = O.points_of_exponents_g1(ex[0]), O.points_of_exponents_g2(ex[1])
        for d in ([next(st) for _ in range(3)], [0, 0, 0]):
            db = [frb(x) for x in d]
            rc, pr = O.pinocchio_prove(q, ppk1, ppk2, cs.mid, sol, *db)
            assert rc == 0 and pr == O.pinocchio_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, sol, frs(ptox), *db)
