// The host half of zk_groth16_srs_check / zk_groth16_srs_contribute on its own (csrc/srs_plan.h: no HIP in it), built by tests/test_srs_plan_host.py
// with -fsanitize=address,undefined.  For every (N1, NAB, N2) of a small exhaustive range, and at the bounds, the plan's coefficient of every scalar of
// every vector equals a NAIVE enumeration of the four relations written here a second time, index by index; every refusal is the specified one, in the
// specified order; the factor checks read the bytes the C-ABI takes.
#include "../../zukelang_amd/csrc/srs_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace zk;

static int fails = 0;
#define EXPECT(cond, ...)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                  \
    } while (0)

// relation by relation, term by term: want[vector][index of its list] = the element of the expansion the term carries, -1 where no term lands
static void naive(uint64_t n1, uint64_t nab, uint64_t n2, std::vector<int64_t> want[SRS_VECS]) {
    const uint64_t len[SRS_VECS] = {n1, n1, n1, n1, nab, nab, nab, n2};
    for (int q = 0; q < SRS_VECS; q++) want[q].assign(len[q], -1);
    for (uint64_t i = 0; i + 1 < n1; i++) {          // TAU_G1: rho_i (tau1[i+1] - tau tau1[i])
        want[SRSV_TAU1_HI][i + 1] = (int64_t)i;
        want[SRSV_TAU1_LO][i] = (int64_t)i;
    }
    for (uint64_t i = 0; i + 1 < nab; i++) {         // ALPHA: rho_i (alpha_tau1[i+1] - tau alpha_tau1[i])
        want[SRSV_ALPHA_HI][i + 1] = (int64_t)i;
        want[SRSV_ALPHA_LO][i] = (int64_t)i;
    }
    for (uint64_t i = 0; i < nab; i++) {             // BETA: rho_i (beta_tau1[i] - beta tau1[i])
        want[SRSV_BETA][i] = (int64_t)i;
        want[SRSV_TAU1_AB][i] = (int64_t)i;
    }
    for (uint64_t i = 0; i < n2; i++) {              // TAU_G2: rho_i (tau1[i] g2 - g1 tau2[i])
        want[SRSV_TAU1_G2][i] = (int64_t)i;
        want[SRSV_TAU2][i] = (int64_t)i;
    }
}

static void check_lengths(uint64_t n1, uint64_t nab, uint64_t n2) {
    SrsPlan p;
    const char* why = nullptr;
    const int rc = srs_plan_make(p, n1, nab, n2, &why);
    EXPECT(rc == SRS_OK && why && !*why, "plan(%llu, %llu, %llu) refused: %d", (unsigned long long)n1, (unsigned long long)nab, (unsigned long long)n2, rc);
    if (rc != SRS_OK) return;
    std::vector<int64_t> want[SRS_VECS];
    naive(n1, nab, n2, want);
    const uint32_t list[SRS_VECS] = {SRS_TAU1, SRS_TAU1, SRS_TAU1, SRS_TAU1, SRS_ALPHA, SRS_ALPHA, SRS_BETA, SRS_TAU2};
    uint64_t at = 0;
    for (int q = 0; q < SRS_VECS; q++) {
        EXPECT(p.v[q].first == at && p.v[q].len == want[q].size() && p.v[q].list == list[q], "vector %d: first / len / list", q);
        EXPECT(p.v[q].lo <= p.v[q].hi && p.v[q].hi <= p.v[q].len && p.v[q].shift <= p.v[q].lo, "vector %d: range", q);
        at += want[q].size();
    }
    EXPECT(p.total == at && p.total == 4 * n1 + 3 * nab + n2, "total");
    for (uint64_t g = 0; g < p.total; g++) {
        const SrsCoef c = srs_plan_coef(p, g);
        EXPECT(c.vec >= 0 && c.vec < SRS_VECS && p.v[c.vec].first + c.index == g && c.index < p.v[c.vec].len, "scalar %llu: not inside its vector", (unsigned long long)g);
        if (c.vec < 0 || c.vec >= SRS_VECS || c.index >= want[c.vec].size()) continue;
        EXPECT(c.rho == want[c.vec][c.index], "(%llu, %llu, %llu) vector %d index %llu: rho %lld, the relations say %lld", (unsigned long long)n1, (unsigned long long)nab,
               (unsigned long long)n2, c.vec, (unsigned long long)c.index, (long long)c.rho, (long long)want[c.vec][c.index]);
    }
}

static void check_refusal(uint64_t n1, uint64_t nab, uint64_t n2, int want) {
    SrsPlan p;
    memset(&p, 0x5a, sizeof p);
    const SrsPlan before = p;
    const char* why = nullptr;
    EXPECT(srs_plan_make(p, n1, nab, n2, &why) == want && why && *why, "(%llu, %llu, %llu): not refused with %d", (unsigned long long)n1, (unsigned long long)nab, (unsigned long long)n2, want);
    EXPECT(memcmp(&p, &before, sizeof p) == 0, "a refused plan was written");
    EXPECT(srs_lengths_check(n1, nab, n2, &why) == want, "lengths_check disagrees");
}

static void put(uint8_t* mul, int f, const uint64_t w[4]) {
    for (int k = 0; k < 4; k++)
        for (int b = 0; b < 8; b++) mul[32 * f + 8 * k + b] = (uint8_t)(w[k] >> (8 * b));
}

int main() {
    for (uint64_t n1 = 2; n1 <= 9; n1++)
        for (uint64_t nab = 1; nab <= n1; nab++)
            for (uint64_t n2 = 2; n2 <= n1; n2++) check_lengths(n1, nab, n2);
    check_lengths(300, 7, 9);
    check_lengths(257, 257, 2);
    // at the bound: the plan itself (no enumeration of 2^27 scalars), and the scalars at every vector's ends
    {
        const uint64_t n1 = SRS_MAX_TAU1, nab = (uint64_t)1 << 24, n2 = ((uint64_t)1 << 24) + 2;
        SrsPlan p;
        const char* why = nullptr;
        EXPECT(srs_plan_make(p, n1, nab, n2, &why) == SRS_OK, "the bound itself is refused");
        EXPECT(p.total == 4 * n1 + 3 * nab + n2, "total at the bound");
        SrsCoef c = srs_plan_coef(p, 0);
        EXPECT(c.vec == SRSV_TAU1_HI && c.index == 0 && c.rho == -1, "TAU1_HI[0] carries zero");
        c = srs_plan_coef(p, n1 - 1);
        EXPECT(c.vec == SRSV_TAU1_HI && c.index == n1 - 1 && c.rho == (int64_t)(n1 - 2), "TAU1_HI's last index");
        c = srs_plan_coef(p, 2 * n1 - 1);
        EXPECT(c.vec == SRSV_TAU1_LO && c.index == n1 - 1 && c.rho == -1, "TAU1_LO's last index carries zero");
        c = srs_plan_coef(p, 2 * n1 - 2);
        EXPECT(c.vec == SRSV_TAU1_LO && c.rho == (int64_t)(n1 - 2), "TAU1_LO's last coefficient");
        c = srs_plan_coef(p, 2 * n1 + nab);
        EXPECT(c.vec == SRSV_TAU1_AB && c.index == nab && c.rho == -1, "TAU1_AB past NAB carries zero");
        c = srs_plan_coef(p, 3 * n1 + n2 - 1);
        EXPECT(c.vec == SRSV_TAU1_G2 && c.rho == (int64_t)(n2 - 1), "TAU1_G2's last coefficient");
        c = srs_plan_coef(p, p.total - 1);
        EXPECT(c.vec == SRSV_TAU2 && c.index == n2 - 1 && c.rho == (int64_t)(n2 - 1), "the last scalar");
    }
    // refusals, in the header's order: the minima (ARG) before the comparisons (DOMAIN)
    check_refusal(1, 1, 2, SRS_ERR_ARG);
    check_refusal(0, 0, 0, SRS_ERR_ARG);
    check_refusal(2, 0, 2, SRS_ERR_ARG);
    check_refusal(2, 1, 1, SRS_ERR_ARG);
    check_refusal(1, 5, 9, SRS_ERR_ARG);                 // below a minimum AND out of proportion: the minimum decides
    check_refusal(((uint64_t)1 << 25) + 1, 0, 2, SRS_ERR_ARG);
    check_refusal(3, 4, 2, SRS_ERR_DOMAIN);
    check_refusal(3, 1, 4, SRS_ERR_DOMAIN);
    check_refusal(((uint64_t)1 << 25) + 1, 1, 2, SRS_ERR_DOMAIN);
    check_refusal(~(uint64_t)0, ~(uint64_t)0, ~(uint64_t)0, SRS_ERR_DOMAIN);
    // the factors: alpha' | beta' | tau'
    {
        const uint64_t R[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
        const uint64_t one[4] = {1, 0, 0, 0}, zero[4] = {0, 0, 0, 0}, rm1[4] = {R[0] - 1, R[1], R[2], R[3]}, rp1[4] = {R[0] + 1, R[1], R[2], R[3]};
        const uint64_t top[4] = {~0ull, ~0ull, ~0ull, ~0ull}, hi[4] = {0, 0, 0, R[3] + 1}, lowbig[4] = {~0ull, ~0ull, ~0ull, R[3] - 1};
        uint8_t mul[96];
        const char* why = nullptr;
        auto run = [&](const uint64_t* a, const uint64_t* b, const uint64_t* t) {
            put(mul, 0, a); put(mul, 1, b); put(mul, 2, t);
            return srs_factors_check(mul, &why);
        };
        EXPECT(run(one, one, one) == SRS_OK, "(1, 1, 1)");
        EXPECT(run(rm1, rm1, rm1) == SRS_OK, "r - 1");
        EXPECT(run(lowbig, one, rm1) == SRS_OK, "a factor with a smaller top word and full low words");
        for (int f = 0; f < 3; f++) {
            const uint64_t* x[3] = {one, rm1, one};
            x[f] = zero;
            EXPECT(run(x[0], x[1], x[2]) == SRS_ERR_ARG, "factor %d = 0", f);
            x[f] = R;
            EXPECT(run(x[0], x[1], x[2]) == SRS_ERR_SCALAR_RANGE, "factor %d = r", f);
            x[f] = rp1;
            EXPECT(run(x[0], x[1], x[2]) == SRS_ERR_SCALAR_RANGE, "factor %d = r + 1", f);
            x[f] = top;
            EXPECT(run(x[0], x[1], x[2]) == SRS_ERR_SCALAR_RANGE, "factor %d = 2^256 - 1", f);
            x[f] = hi;
            EXPECT(run(x[0], x[1], x[2]) == SRS_ERR_SCALAR_RANGE, "factor %d above r in the top word only", f);
        }
        EXPECT(run(R, zero, one) == SRS_ERR_SCALAR_RANGE && run(zero, R, one) == SRS_ERR_ARG, "the first bad factor decides");
    }
    if (fails) {
        printf("%d failures\n", fails);
        return 1;
    }
    printf("srs_plan ok\n");
    return 0;
}
