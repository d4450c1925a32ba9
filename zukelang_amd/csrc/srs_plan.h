// Host half of zk_groth16_srs_check and zk_groth16_srs_contribute (srs.hip): the argument and length checks, and where every coefficient of the
// check's eight scalar vectors comes from -- which index of which list carries which element of the seed's expansion, and which carry zero.  Plain
// C++, no device code: tests/host/srs_plan_main.cpp holds it to a naive enumeration of the relations under AddressSanitizer + UBSan.
//
// A string is tau1[N1] | alpha_tau1[NAB] | beta_tau1[NAB] in G1 and beta2 | tau2[N2] in G2.  With rho the expansion (N1 scalars), the relations are
//   TAU_G1   sum_{i < N1-1}  rho_i (tau1[i+1]       - tau  tau1[i])       = 0        vectors TAU1_HI, TAU1_LO over tau1
//   ALPHA    sum_{i < NAB-1} rho_i (alpha_tau1[i+1] - tau  alpha_tau1[i]) = 0        vectors ALPHA_HI, ALPHA_LO over alpha_tau1
//   BETA     sum_{i < NAB}   rho_i (beta_tau1[i]    - beta tau1[i])       = 0        vectors BETA over beta_tau1, TAU1_AB over tau1
//   TAU_G2   sum_{i < N2}    rho_i (tau1[i] g2      - g1 tau2[i])         = 0        vectors TAU1_G2 over tau1, TAU2 over tau2
// A vector over a list of `len` points holds rho_(i - shift) at the indices lo <= i < hi and zero at every other index below len: the shifted copy of a
// relation is the SAME expansion moved by one, and a sum that stops before its list does is the long sum with zero coefficients.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zk {

enum SrsList { SRS_TAU1 = 0, SRS_ALPHA = 1, SRS_BETA = 2, SRS_TAU2 = 3, SRS_LISTS = 4 };
enum SrsVec { SRSV_TAU1_HI = 0, SRSV_TAU1_LO, SRSV_TAU1_AB, SRSV_TAU1_G2, SRSV_ALPHA_HI, SRSV_ALPHA_LO, SRSV_BETA, SRSV_TAU2, SRS_VECS };

// the codes of include/zkmi355x.h (this header includes nothing of the library; srs.hip asserts they agree)
static constexpr int SRS_OK = 0, SRS_ERR_ARG = -1, SRS_ERR_SCALAR_RANGE = -3, SRS_ERR_DOMAIN = -8;
static constexpr uint64_t SRS_MAX_TAU1 = (uint64_t)1 << 25;          // zk_groth16_srs_sizes at n = 2^24

struct SrsVecPlan {
    uint32_t list;          // SrsList: the base list the vector runs over
    uint32_t shift;         // index i carries rho_(i - shift)
    uint64_t len;           // points of that list = scalars of the vector
    uint64_t lo, hi;        // the indices that carry a coefficient; lo == hi: the relation has no index, the sum is the identity
    uint64_t first;         // the vector's first scalar in the one buffer that holds all eight, back to back
};
struct SrsPlan {
    uint64_t n1, nab, n2;
    uint64_t total;         // scalars of all vectors
    SrsVecPlan v[SRS_VECS];
};

// The lengths of a string, refusals in the header's order: counts below the minima -> ARG, then NAB > N1, N2 > N1, N1 > 2^25 -> DOMAIN.
// *why: a static text for the error record.
static inline int srs_lengths_check(uint64_t n1, uint64_t nab, uint64_t n2, const char** why) {
    if (n1 < 2 || n2 < 2 || nab < 1) { *why = "a string holds at least 2 points of tau1, 2 of tau2 and 1 of alpha_tau1 / beta_tau1"; return SRS_ERR_ARG; }
    if (nab > n1) { *why = "more alpha_tau1 / beta_tau1 points than tau1 points (BETA compares against tau1[i])"; return SRS_ERR_DOMAIN; }
    if (n2 > n1) { *why = "more tau2 points than tau1 points (TAU_G2 compares against tau1[i])"; return SRS_ERR_DOMAIN; }
    if (n1 > SRS_MAX_TAU1) { *why = "more than 2^25 tau1 points"; return SRS_ERR_DOMAIN; }
    *why = "";
    return SRS_OK;
}

static inline int srs_plan_make(SrsPlan& p, uint64_t n1, uint64_t nab, uint64_t n2, const char** why) {
    const int rc = srs_lengths_check(n1, nab, n2, why);
    if (rc != SRS_OK) return rc;
    p.n1 = n1; p.nab = nab; p.n2 = n2;
    const uint64_t len[SRS_LISTS] = {n1, nab, nab, n2};
    auto set = [&](int q, uint32_t list, uint32_t shift, uint64_t lo, uint64_t hi) {
        p.v[q].list = list; p.v[q].shift = shift; p.v[q].len = len[list]; p.v[q].lo = lo; p.v[q].hi = hi;
    };
    set(SRSV_TAU1_HI, SRS_TAU1, 1, 1, n1);              // rho_i on tau1[i+1], i < N1-1
    set(SRSV_TAU1_LO, SRS_TAU1, 0, 0, n1 - 1);          // rho_i on tau1[i],   i < N1-1: the last point carries zero
    set(SRSV_TAU1_AB, SRS_TAU1, 0, 0, nab);
    set(SRSV_TAU1_G2, SRS_TAU1, 0, 0, n2);
    set(SRSV_ALPHA_HI, SRS_ALPHA, 1, 1, nab);           // NAB = 1: lo == hi, no index
    set(SRSV_ALPHA_LO, SRS_ALPHA, 0, 0, nab - 1);
    set(SRSV_BETA, SRS_BETA, 0, 0, nab);
    set(SRSV_TAU2, SRS_TAU2, 0, 0, n2);
    uint64_t at = 0;
    for (int q = 0; q < SRS_VECS; q++) { p.v[q].first = at; at += p.v[q].len; }
    p.total = at;
    return SRS_OK;
}

// Scalar g of the buffer: which vector, which index of its list, and the element of the expansion it carries (-1: zero).  g < p.total.
// The coefficient kernel calls exactly this function per lane: the unit that launches it defines SRS_PLAN_FN as the qualifiers its compiler wants.
#ifndef SRS_PLAN_FN
#define SRS_PLAN_FN static inline
#endif
struct SrsCoef { int vec; uint64_t index; int64_t rho; };
SRS_PLAN_FN SrsCoef srs_plan_coef(const SrsPlan& p, uint64_t g) {
    int q = 0;
    while (q + 1 < SRS_VECS && g >= p.v[q + 1].first) q++;
    const SrsVecPlan& v = p.v[q];
    const uint64_t i = g - v.first;
    return {q, i, i >= v.lo && i < v.hi ? (int64_t)(i - v.shift) : (int64_t)-1};
}

// The three factors of a contribution, canonical little-endian Fr each: 0 -> ARG, >= r -> SCALAR_RANGE, the first bad factor in the order alpha', beta', tau'.
static inline int srs_factors_check(const uint8_t mul[96], const char** why) {
    static const uint64_t R[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
    for (int f = 0; f < 3; f++) {
        uint64_t w[4];
        for (int k = 0; k < 4; k++) {
            w[k] = 0;
            for (int b = 7; b >= 0; b--) w[k] = (w[k] << 8) | mul[32 * f + 8 * k + b];
        }
        if ((w[0] | w[1] | w[2] | w[3]) == 0) { *why = "a factor of a contribution is 0"; return SRS_ERR_ARG; }
        bool below = false;
        for (int k = 3; k >= 0; k--)
            if (w[k] != R[k]) { below = w[k] < R[k]; break; }
        if (!below) { *why = "a factor of a contribution is >= r"; return SRS_ERR_SCALAR_RANGE; }
    }
    *why = "";
    return SRS_OK;
}

}  // namespace zk
