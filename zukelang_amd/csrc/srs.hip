// A phase-1 string judged and contributed to: zk_groth16_srs_check and zk_groth16_srs_contribute (include/zkmi355x.h).
//
// The check.  tau1[N1] | alpha_tau1[NAB] | beta_tau1[NAB] and beta2 | tau2[N2] are decoded once into dense affine points, every list through the
// endomorphism subgroup test (a pairing does not see a cofactor component: the test is part of the verdict, whatever ZK_KEY_SUBGROUP_CHECK says).  Each
// of the four relations is ONE equation between two pairing products over sums with coefficients from the seed's expansion (seed_expand.cuh, the
// generator of the key checks).  Which index of which list carries which coefficient is srs_plan.h's, plain C++ held to a naive enumeration on the
// host; k_srs_coefficients writes all eight vectors from that plan in one launch.  The sums are products on the Pippenger chain over base sets that live
// for the call: the four vectors over tau1 are four jobs of ONE chain of sort and accumulate launches, the two over alpha_tau1 two jobs of another.
//
// The contribution.  tau'^i, alpha' tau'^i and beta' tau'^i come from keygen's power scan (power_run), the multiplications go through
// points_scale_tabmul on both curves, the link's G2 points through fixed_base_mul.  No kernel of the call's own.
// Nothing outlives either call.
#include "ec.cuh"
#include "groth16_key.cuh"
#include "seed_expand.cuh"
#define SRS_PLAN_FN static inline __host__ __device__          // srs_plan_coef runs in k_srs_coefficients as it stands
#include "srs_plan.h"

#include <string.h>
#include <vector>

// 1: the sums run over window tables (the measurement of DESIGN 2t; never the default)
#ifndef ZK_SRS_PRECOMP
#define ZK_SRS_PRECOMP 0
#endif

namespace zk {

static_assert(SRS_ERR_ARG == ZK_ERR_ARG && SRS_ERR_SCALAR_RANGE == ZK_ERR_SCALAR_RANGE && SRS_ERR_DOMAIN == ZK_ERR_DOMAIN && SRS_OK == ZK_OK, "srs_plan.h restates the header's codes");

static inline dim3 g1d(uint64_t n, unsigned t = 256) { return dim3((unsigned)((n + t - 1) / t)); }

// All coefficient vectors of the check in one launch (canonical scalars): the expansion, its shifted copies, zeros past each relation's last index.
// Which element of the expansion scalar g carries is srs_plan_coef's answer, the function the host test holds to the relations.
__global__ void k_srs_coefficients(uint32_t* __restrict__ out, SrsPlan p, KeychkSeed seed) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= p.total) return;
    const SrsCoef c = srs_plan_coef(p, g);
    Fr x = fe_zero<FrParams>();
    if (c.rho >= 0) x = seed_expand_at(seed, (uint64_t)c.rho);
    fe_store<FrParams>(out + 8 * g, x);
}
// k[0..2] <- Montgomery forms of three canonical scalars
__global__ void k_srs_factors_to_mont(uint32_t* __restrict__ out, const uint32_t* __restrict__ in) {
    const uint32_t i = threadIdx.x;
    if (blockIdx.x || i >= 3) return;
    fe_store<FrParams>(out + 8 * i, fe_to_mont(fe_load<FrParams>(in + 8 * i)));
}

static inline bool is_identity_bytes(const uint8_t* p) { return (p[0] & 0x40) != 0; }

// One list of the string: host bytes -> dense affine points at d_dense with an upload's verdicts (encoding, curve), then -- `subgroup` -- the
// endomorphism test over the decoded list.  The list's first failing kind decides: encoding, curve, subgroup.  Waits.
static int srs_list_decode(Curve cv, const uint8_t* bytes, uint64_t n, uint8_t* d_dense, bool subgroup, const char* family, DevBuf& verdict, std::vector<uint8_t>& hv, hipStream_t s) {
    {
        ScopedTimer t(family, s);
        ScopedTimer t1((std::string(family) + ":decode").c_str(), s);
        ZKCHK(points_from_bytes_checked(cv, bytes, n, d_dense, false, s));
    }
    if (!subgroup) return ZK_OK;
    HIPCHK(hipMemsetAsync(verdict.p, 0, n, s));
    {
        ScopedTimer t(family, s);
        ScopedTimer t1((std::string(family) + ":subgroup").c_str(), s);
        ZKCHK(points_subgroup_verdicts(cv, d_dense, n, verdict.as<uint8_t>(), SUBGROUP_ENDO, s));
    }
    hv.resize(n);
    HIPCHK(hipMemcpyAsync(hv.data(), verdict.p, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (memchr(hv.data(), 4, n)) ZK_FAIL(ZK_ERR_NOT_ON_CURVE, "a point of the string is on the curve but outside the prime-order subgroup");
    return ZK_OK;
}
// The five lists in the order tau1, alpha_tau1, beta_tau1, beta2 | tau2 into s1 / s2 (allocated here), the first bad list deciding.
static int srs_decode(const uint8_t* srs_g1, const uint8_t* srs_g2, uint64_t n1, uint64_t nab, uint64_t n2, bool subgroup, const char* family, DevBuf& s1, DevBuf& s2, hipStream_t s) {
    ZKCHK(s1.alloc(96 * (n1 + 2 * nab)));
    ZKCHK(s2.alloc(192 * (1 + n2)));
    DevBuf verdict;
    std::vector<uint8_t> hv;
    if (subgroup) ZKCHK(verdict.alloc(n1));          // the longest list
    uint8_t *d1 = s1.as<uint8_t>(), *d2 = s2.as<uint8_t>();
    ZKCHK(srs_list_decode(CURVE_G1, srs_g1, n1, d1, subgroup, family, verdict, hv, s));
    ZKCHK(srs_list_decode(CURVE_G1, srs_g1 + 96 * n1, nab, d1 + 96 * n1, subgroup, family, verdict, hv, s));
    ZKCHK(srs_list_decode(CURVE_G1, srs_g1 + 96 * (n1 + nab), nab, d1 + 96 * (n1 + nab), subgroup, family, verdict, hv, s));
    ZKCHK(srs_list_decode(CURVE_G2, srs_g2, 1, d2, subgroup, family, verdict, hv, s));
    ZKCHK(srs_list_decode(CURVE_G2, srs_g2 + 192, n2, d2 + 192, subgroup, family, verdict, hv, s));
    return ZK_OK;
}

// `count` products over one list (dense affine points on the device) as jobs of one chain of sort and accumulate launches and one chain of reduction
// launches: result j = sum_i scal[j][i] pts[i] as dense XYZZ at outs[j].  The base set and the workspaces live for this function.  Waits.
static int srs_sums(Curve cv, const uint8_t* d_pts, uint64_t n, const void* const* scal, void* const* outs, uint32_t count, hipStream_t s) {
    MsmBases b;
    MsmWorkspace w[MAX_SORT_JOBS];
    MsmWorkspace* ws[MAX_SORT_JOBS];
    ZKCHK(msm_bases_from_device_affine(b, cv, d_pts, n, 0, ZK_SRS_PRECOMP != 0, s, true));          // in_subgroup: the endomorphism test has passed every point
    for (uint32_t j = 0; j < count; j++) {
        ZKCHK(msm_workspace_alloc(w[j], b));
        ws[j] = &w[j];
    }
    ZKCHK(msm_sort_accumulate_many(b, ws, scal, count, s));
    ZKCHK(msm_reduce(b, ws, outs, count, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}

static int srs_check_run(const SrsPlan& p, const uint8_t* srs_g1, const uint8_t* srs_g2, const uint8_t* seed, uint32_t* failed) {
    Ctx& c = ctx();
    hipStream_t s = c.stream;
    HIPCHK(hipGetLastError());
    const KeychkSeed sd = seed_take(seed);
    const uint64_t n1 = p.n1, nab = p.nab, n2 = p.n2;
    DevBuf s1, s2;
    ZKCHK(srs_decode(srs_g1, srs_g2, n1, nab, n2, true, "srs_check", s1, s2, s));
    uint8_t *d_tau1 = s1.as<uint8_t>(), *d_at1 = d_tau1 + 96 * n1, *d_bt1 = d_at1 + 96 * nab, *d_b2 = s2.as<uint8_t>(), *d_tau2 = d_b2 + 192;
    // ---- the eight coefficient vectors
    DevBuf scal, res1, res2;
    ZKCHK(scal.alloc(32 * p.total));
    const size_t g1x = xyzz_bytes(CURVE_G1), g2x = xyzz_bytes(CURVE_G2);
    ZKCHK(res1.alloc(g1x * 7));
    ZKCHK(res2.alloc(g2x));
    HIPCHK(hipMemsetAsync(res1.p, 0, res1.bytes, s));          // zz = 0: the identity, for a relation that has no index
    HIPCHK(hipMemsetAsync(res2.p, 0, res2.bytes, s));
    {
        ScopedTimer t("srs_check", s);
        hipLaunchKernelGGL(k_srs_coefficients, g1d(p.total), dim3(256), 0, s, scal.as<uint32_t>(), p, sd);
        HIPCHK(hipGetLastError());
    }
    auto vec = [&](int q) -> const void* { return scal.as<uint8_t>() + 32 * p.v[q].first; };
    auto sum1 = [&](int q) -> void* { return res1.as<uint8_t>() + g1x * q; };          // the G1 sums in SrsVec order (0..6)
    {
        ScopedTimer t("srs_check", s);
        ScopedTimer t1("srs_check:sums", s);
        const void* st[4] = {vec(SRSV_TAU1_HI), vec(SRSV_TAU1_LO), vec(SRSV_TAU1_AB), vec(SRSV_TAU1_G2)};
        void* ot[4] = {sum1(SRSV_TAU1_HI), sum1(SRSV_TAU1_LO), sum1(SRSV_TAU1_AB), sum1(SRSV_TAU1_G2)};
        ZKCHK(srs_sums(CURVE_G1, d_tau1, n1, st, ot, 4, s));
        if (p.v[SRSV_ALPHA_HI].lo < p.v[SRSV_ALPHA_HI].hi) {          // NAB = 1: ALPHA has no index and holds
            const void* sa[2] = {vec(SRSV_ALPHA_HI), vec(SRSV_ALPHA_LO)};
            void* oa[2] = {sum1(SRSV_ALPHA_HI), sum1(SRSV_ALPHA_LO)};
            ZKCHK(srs_sums(CURVE_G1, d_at1, nab, sa, oa, 2, s));
        }
        const void* sb[1] = {vec(SRSV_BETA)};
        void* ob[1] = {sum1(SRSV_BETA)};
        ZKCHK(srs_sums(CURVE_G1, d_bt1, nab, sb, ob, 1, s));
        const void* s2v[1] = {vec(SRSV_TAU2)};
        void* o2[1] = {res2.p};
        ZKCHK(srs_sums(CURVE_G2, d_tau2, n2, s2v, o2, 1, s));
    }
    // ---- the string's single points and the generators, as bytes: tau1[0] | alpha_tau1[0] | [1]_1, beta2 | tau2[0] | tau2[1] | [1]_2
    DevBuf dn1, dn2, one;
    ZKCHK(dn1.alloc(96 * 3 * 2));
    ZKCHK(dn2.alloc(192 * 4 * 2));
    ZKCHK(one.alloc(32));
    const uint8_t one_le[32] = {1};
    HIPCHK(hipMemcpyAsync(one.p, one_le, 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dn1.p, d_tau1, 96, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(dn1.as<uint8_t>() + 96, d_at1, 96, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(dn2.p, d_b2, 192 * 3, hipMemcpyDeviceToDevice, s));          // beta2 | tau2[0] | tau2[1]: N2 >= 2
    ZKCHK(fixed_base_mul(CURVE_G1, dn1.as<uint8_t>() + 96 * 2, one.p, 1, s));
    ZKCHK(fixed_base_mul(CURVE_G2, dn2.as<uint8_t>() + 192 * 3, one.p, 1, s));
    ZKCHK(points_affine_to_bytes(CURVE_G1, dn1.as<uint8_t>() + 96 * 3, dn1.p, 3, s));
    ZKCHK(points_affine_to_bytes(CURVE_G2, dn2.as<uint8_t>() + 192 * 4, dn2.p, 4, s));
    uint8_t kp1[3][96], kp2[4][192], sm1[7][96], sm2[1][192];
    HIPCHK(hipMemcpyAsync(kp1, dn1.as<uint8_t>() + 96 * 3, sizeof kp1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(kp2, dn2.as<uint8_t>() + 192 * 4, sizeof kp2, hipMemcpyDeviceToHost, s));
    ZKCHK(points_xyzz_to_bytes(CURVE_G1, res1.p, 7, &sm1[0][0], s));          // synchronises
    ZKCHK(points_xyzz_to_bytes(CURVE_G2, res2.p, 1, &sm2[0][0], s));
    const uint8_t *t1_0 = kp1[0], *a_0 = kp1[1], *gen1 = kp1[2];
    const uint8_t *b2 = kp2[0], *t2_0 = kp2[1], *t2_1 = kp2[2], *gen2 = kp2[3];
    // ---- the eight pairing products: relation j holds iff product 2j equals product 2j + 1
    std::vector<uint8_t> P, Q, gt;
    std::vector<uint64_t> lens;
    auto product = [&](const uint8_t* g1p, const uint8_t* g2p) {
        P.insert(P.end(), g1p, g1p + 96);
        Q.insert(Q.end(), g2p, g2p + 192);
        lens.push_back(1);
    };
    product(sm1[SRSV_TAU1_HI], gen2);   product(sm1[SRSV_TAU1_LO], t2_1);          // TAU_G1
    product(sm1[SRSV_TAU1_G2], gen2);   product(gen1, sm2[0]);                     // TAU_G2
    product(sm1[SRSV_ALPHA_HI], gen2);  product(sm1[SRSV_ALPHA_LO], t2_1);         // ALPHA
    product(sm1[SRSV_BETA], gen2);      product(sm1[SRSV_TAU1_AB], b2);            // BETA
    {
        ScopedTimer t("srs_check", s);
        ScopedTimer t1("srs_check:pairings", s);
        ZKCHK(keychk_pairing_products(P, Q, lens, gt, s));
    }
    auto differ = [&](int j) { return memcmp(gt.data() + 576 * (2 * j), gt.data() + 576 * (2 * j + 1), 576) != 0; };
    uint32_t f = 0;
    if (memcmp(t1_0, gen1, 96) || memcmp(t2_0, gen2, 192)) f |= ZK_SRSCHK_GENERATORS;
    if (differ(0)) f |= ZK_SRSCHK_TAU_G1;
    if (differ(1)) f |= ZK_SRSCHK_TAU_G2;
    if (differ(2)) f |= ZK_SRSCHK_ALPHA;
    if (differ(3)) f |= ZK_SRSCHK_BETA;
    if (is_identity_bytes(t2_1) || is_identity_bytes(a_0) || is_identity_bytes(b2)) f |= ZK_SRSCHK_TRIVIAL;
    *failed = f;
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}

static constexpr uint64_t SRS_SCALE_SLAB = (uint64_t)1 << 18;          // points per chain of launches of the multiplications (contribute.hip: SCALE_SLAB)
static int srs_scale_list(Curve cv, uint8_t* d_pts, const uint8_t* d_k, uint64_t n, hipStream_t s) {
    for (uint64_t i0 = 0; i0 < n; i0 += SRS_SCALE_SLAB) {
        const uint64_t cnt = n - i0 < SRS_SCALE_SLAB ? n - i0 : SRS_SCALE_SLAB;
        uint8_t* q = d_pts + aff_bytes(cv) * i0;
        ZKCHK(points_scale_tabmul(cv, q, q, d_k + 32 * i0, cnt, s));          // waits
    }
    return ZK_OK;
}

static int srs_contribute_run(uint64_t n1, uint64_t nab, uint64_t n2, const uint8_t* srs_g1, const uint8_t* srs_g2, const uint8_t* mul, uint8_t* out_g1, uint8_t* out_g2,
                              uint8_t* link_g1, uint8_t* link_g2) {
    Ctx& c = ctx();
    hipStream_t s = c.stream;
    HIPCHK(hipGetLastError());
    const bool chk = key_subgroup_check();
    DevBuf s1, s2;
    ZKCHK(srs_decode(srs_g1, srs_g2, n1, nab, n2, chk, "srs_contribute", s1, s2, s));
    uint8_t *d_tau1 = s1.as<uint8_t>(), *d_at1 = d_tau1 + 96 * n1, *d_bt1 = d_at1 + 96 * nab, *d_b2 = s2.as<uint8_t>(), *d_tau2 = d_b2 + 192;
    // ---- the scalars: tau'^i (N1 of them; tau2 reads the first N2), alpha' tau'^i, beta' tau'^i (NAB each), canonical
    DevBuf fac, pw, lk1, lk2;
    ZKCHK(fac.alloc(32 * 6));          // canonical alpha' | beta' | tau', then their Montgomery forms
    ZKCHK(pw.alloc(32 * (n1 + 2 * nab)));
    ZKCHK(lk1.alloc(96 * 6 * 2));
    ZKCHK(lk2.alloc(192 * 3 * 2));
    HIPCHK(hipMemcpyAsync(fac.p, mul, 96, hipMemcpyHostToDevice, s));
    uint32_t* mont = fac.as<uint32_t>() + 8 * 3;
    uint32_t *p_t = pw.as<uint32_t>(), *p_a = p_t + 8 * n1, *p_b = p_a + 8 * nab;
    {
        ScopedTimer t("srs_contribute", s);
        ScopedTimer t1("srs_contribute:scalars", s);
        hipLaunchKernelGGL(k_srs_factors_to_mont, dim3(1), dim3(64), 0, s, mont, (const uint32_t*)fac.as<uint32_t>());
        HIPCHK(hipGetLastError());
        ZKCHK(power_run(p_t, mont + 16, nullptr, n1, s, "srs_contribute:powers"));
        ZKCHK(power_run(p_a, mont + 16, mont, nab, s, "srs_contribute:powers"));
        ZKCHK(power_run(p_b, mont + 16, mont + 8, nab, s, "srs_contribute:powers"));
        ZKCHK(fr_from_mont(pw.p, pw.p, n1 + 2 * nab, s));
    }
    // the link's "before" points, then the multiplications in place
    uint8_t* l1 = lk1.as<uint8_t>();
    HIPCHK(hipMemcpyAsync(l1, d_tau1 + 96, 96, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(l1 + 192, d_at1, 96, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(l1 + 384, d_bt1, 96, hipMemcpyDeviceToDevice, s));
    int rc;
    {
        ScopedTimer t("srs_contribute", s);
        ScopedTimer t1("srs_contribute:multiply", s);
        rc = srs_scale_list(CURVE_G1, d_tau1, (const uint8_t*)p_t, n1, s);
        if (rc == ZK_OK) rc = srs_scale_list(CURVE_G1, d_at1, (const uint8_t*)p_a, nab, s);
        if (rc == ZK_OK) rc = srs_scale_list(CURVE_G1, d_bt1, (const uint8_t*)p_b, nab, s);
        if (rc == ZK_OK) rc = srs_scale_list(CURVE_G2, d_b2, fac.as<uint8_t>() + 32, 1, s);          // beta2 <- beta' beta2
        if (rc == ZK_OK) rc = srs_scale_list(CURVE_G2, d_tau2, (const uint8_t*)p_t, n2, s);
    }
    if (rc == ZK_OK) {
        HIPCHK(hipMemcpyAsync(l1 + 96, d_tau1 + 96, 96, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(l1 + 288, d_at1, 96, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(l1 + 480, d_bt1, 96, hipMemcpyDeviceToDevice, s));
        // [tau']_2 | [alpha']_2 | [beta']_2 from the canonical factors alpha' | beta' | tau'
        rc = fixed_base_mul(CURVE_G2, lk2.p, fac.as<uint8_t>() + 64, 1, s);
        if (rc == ZK_OK) rc = fixed_base_mul(CURVE_G2, lk2.as<uint8_t>() + 192, fac.p, 2, s);
    }
    // the factors are a contributor's secret: nothing of them stays behind in freed device memory
    HIPCHK(hipMemsetAsync(fac.p, 0, fac.bytes, s));
    HIPCHK(hipMemsetAsync(pw.p, 0, pw.bytes, s));
    HIPCHK(hipStreamSynchronize(s));
    if (rc != ZK_OK) return rc;
    // ---- out: everything is encoded on the device first, then copied down -- an output may be the input's own memory, which has been read
    DevBuf b1, b2;
    ZKCHK(b1.alloc(96 * (n1 + 2 * nab)));
    ZKCHK(b2.alloc(192 * (1 + n2)));
    ZKCHK(points_affine_to_bytes(CURVE_G1, b1.p, s1.p, n1 + 2 * nab, s));
    ZKCHK(points_affine_to_bytes(CURVE_G2, b2.p, s2.p, 1 + n2, s));
    ZKCHK(points_affine_to_bytes(CURVE_G1, l1 + 96 * 6, l1, 6, s));
    ZKCHK(points_affine_to_bytes(CURVE_G2, lk2.as<uint8_t>() + 192 * 3, lk2.p, 3, s));
    HIPCHK(hipStreamSynchronize(s));          // every launch has succeeded before the first byte is written
    HIPCHK(hipMemcpyAsync(out_g1, b1.p, 96 * (n1 + 2 * nab), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_g2, b2.p, 192 * (1 + n2), hipMemcpyDeviceToHost, s));
    if (link_g1) HIPCHK(hipMemcpyAsync(link_g1, l1 + 96 * 6, 96 * 6, hipMemcpyDeviceToHost, s));
    if (link_g2) HIPCHK(hipMemcpyAsync(link_g2, lk2.as<uint8_t>() + 192 * 3, 192 * 3, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}

}  // namespace zk

using namespace zk;
extern "C" {

int zk_groth16_srs_check(const uint8_t* srs_g1, size_t tau1_points, size_t ab_points, const uint8_t* srs_g2, size_t tau2_points, const uint8_t* seed, uint32_t* failed) {
    if (!srs_g1 || !srs_g2 || !failed) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_srs_check: null argument");
    SrsPlan plan;
    const char* why = "";
    const int rc = srs_plan_make(plan, tau1_points, ab_points, tau2_points, &why);
    if (rc != SRS_OK) return ::zk::set_error(rc, (std::string("zk_groth16_srs_check: ") + why).c_str(), __FILE__, __LINE__);
    ZKCHK(ensure_init());
    if (ctx_count() > 1) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_srs_check: a string is checked on a device list of one entry");
    return srs_check_run(plan, srs_g1, srs_g2, seed, failed);
}

int zk_groth16_srs_contribute(const uint8_t* srs_g1, size_t tau1_points, size_t ab_points, const uint8_t* srs_g2, size_t tau2_points, const uint8_t* mul, uint8_t* out_g1,
                              uint8_t* out_g2, uint8_t* link_g1, uint8_t* link_g2) {
    if (!srs_g1 || !srs_g2 || !mul || !out_g1 || !out_g2) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_srs_contribute: null argument");
    const char* why = "";
    int rc = srs_lengths_check(tau1_points, ab_points, tau2_points, &why);
    if (rc == SRS_OK) rc = srs_factors_check(mul, &why);
    if (rc != SRS_OK) return ::zk::set_error(rc, (std::string("zk_groth16_srs_contribute: ") + why).c_str(), __FILE__, __LINE__);
    ZKCHK(ensure_init());
    if (ctx_count() > 1) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_srs_contribute: a string is contributed to on a device list of one entry");
    return srs_contribute_run(tau1_points, ab_points, tau2_points, srs_g1, srs_g2, mul, out_g1, out_g2, link_g1, link_g2);
}

}  // extern "C"
