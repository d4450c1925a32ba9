// Pairings in batches on the device (scope row f1; include/zkmi355x.h: zk_pairing_product_many, zk_groth16_verify_many, zk_pinocchio_verify_many):
// many products of pairings -- many proofs' verifications -- per call.  The single-proof verifiers stay on the host (pairing_host.hip, which this
// file does not touch: the host-only sanitizer library is built from it alone); a stream of proofs is checked here.  Same definitions, same bytes:
// Pairing.pairing of curve.mli:46-54, Groth16.verify of groth16.ml:163-173, Verify.f of pinocchio.ml:254-420.
//
//   bytes -> affine + one verdict per point    k_bytes_to_affine_verdict, k_subgroup_verdict by [r] P = O (msm_points.hip: one lane per point); which
//                                               bad point decides a proof's or the call's status: verdict_order.h
//   sums over the public inputs                 the resident short products of msm_resident.hip: the key's points uploaded once per call, one product per proof
//   Miller loops                                k_miller: one group of 8 lanes per PAIR (pairing_tower.cuh), inversion-free, 63 steps
//   products + final exponentiations            k_final_exp: one group per PRODUCT multiplies its pairs' Miller values and raises to (p^12 - 1) / r
//   one long product (the folded verifier)      k_gt_tree_mul: one group per RUN of GT_TREE_RUN raw Miller values, level after level until one is left;
//                                               k_gt_pow: a GT encoding raised to an exponent read from device memory (square and multiply, both every bit)
//
// A batch is bound by latency, not by the multipliers: one G2 subgroup check is ~15 k base-field products on one lane, a Miller loop ~2.6 k and a
// final exponentiation ~7 k per lane of a group, and every pair and product of the batch does them side by side (profiles/verify_many.json).
#include "pairing_tower.cuh"

#include "msm.cuh"
#include "pairing_consts.h"
#include "verdict_order.h"

#include <string.h>
#include <vector>

namespace zk {

static constexpr uint32_t F12_RAW_WORDS = f12::EW;          // a Miller value between the two kernels: 6 coefficients x 28 limbs
static_assert(F12_RAW_WORDS * 4 == PAIRING_RAW_BYTES, "msm.cuh: the size of a raw Miller value");

// pair g of n: P = g1[g], Q = g2[g] (dense affine, checked); out[g] = the conjugated Miller value, 1 when either point is the identity
__global__ __launch_bounds__(64) void k_miller(const uint8_t* __restrict__ g1, const uint8_t* __restrict__ g2, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t g = blockIdx.x * f12::GROUPS_PER_WAVE + threadIdx.x / f12::GROUP;
    const bool live = g < n;
    const uint32_t gi = live ? g : n - 1;          // the spare groups of the last workgroup walk along: the barriers are the workgroup's
    const Aff<Fp> P = aff_load<Fp>(g1 + 96 * (size_t)gi);
    const Aff<Fp2> Q = aff_load<Fp2>(g2 + 192 * (size_t)gi);
    const bool skip = aff_is_inf(P) || aff_is_inf(Q);          // on (0, 0) the loop computes some value without harm (no inversion, no branch on data)
    f12::miller(P, Q);
    const uint32_t k = f12::coef();
    const f12::F12C one = f12::sel<1>(k == 0, fp2_zero(), fp2_one());
    const f12::F12C x = f12::sel<256>(skip, f12::ld<256>(f12::reg_cell(0, k)), one);
    if (live) f12::st(out + (size_t)F12_RAW_WORDS * g + k * f12::CW, x);
}
// product q of n: the Miller values [off[q], off[q + 1]) multiplied, then the final exponentiation, then the GT encoding (576 B)
__global__ __launch_bounds__(64) void k_final_exp(const uint32_t* __restrict__ miller, const uint32_t* __restrict__ off, uint32_t n, uint8_t* __restrict__ gt) {
    const uint32_t first = blockIdx.x * f12::GROUPS_PER_WAVE, g = first + threadIdx.x / f12::GROUP;
    const bool live = g < n;
    const uint32_t gi = live ? g : n - 1;
    const uint32_t lo = off[gi], len = off[gi + 1] - lo;
    uint32_t most = 0;                               // the longest product of this workgroup: every group takes that many steps
    for (uint32_t q = first; q < first + f12::GROUPS_PER_WAVE && q < n; q++) most = max(most, off[q + 1] - off[q]);
    f12::set_one(0);
    const uint32_t k = f12::coef();
    const f12::F12C one = f12::sel<1>(k == 0, fp2_zero(), fp2_one());
    for (uint32_t j = 0; j < most; j++) {
        const bool have = j < len;
        const f12::F12C x = f12::sel<256>(!have, f12::ld<256>(miller + (size_t)F12_RAW_WORDS * (have ? lo + j : 0) + k * f12::CW), one);
        __syncthreads();
        f12::st(f12::reg_cell(1, k), x);
        __syncthreads();
        f12::mul(0, 0, 1);
    }
    f12::final_exp();
    f12::store_gt(gt + 576 * (size_t)gi, 0, live);
}
// One level of the product tree over raw Miller values: out[g] = in[R g] in[R g + 1] ... (a ragged last run is shorter), R = GT_TREE_RUN.  k_final_exp
// multiplies a product's values in ONE group, serially: for thousands of values that loop would be the call; here every level is R - 1 dependent
// products whatever n is.  Every group takes R - 1 steps (a short run multiplies by 1: chosen by sel, the barriers are the workgroup's).
static constexpr uint32_t GT_TREE_RUN = 4;
__global__ __launch_bounds__(64) void k_gt_tree_mul(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t nout = (n + GT_TREE_RUN - 1) / GT_TREE_RUN;
    const uint32_t g = blockIdx.x * f12::GROUPS_PER_WAVE + threadIdx.x / f12::GROUP;
    const bool live = g < nout;
    const uint32_t gi = live ? g : nout - 1;
    const uint32_t lo = gi * GT_TREE_RUN, len = n - lo < GT_TREE_RUN ? n - lo : GT_TREE_RUN;          // 1 <= len
    const uint32_t k = f12::coef();
    const f12::F12C one = f12::sel<1>(k == 0, fp2_zero(), fp2_one());
    f12::load_raw(0, in + (size_t)F12_RAW_WORDS * lo);
    for (uint32_t j = 1; j < GT_TREE_RUN; j++) {
        const bool have = j < len;
        const f12::F12C x = f12::sel<256>(!have, f12::ld<256>(in + (size_t)F12_RAW_WORDS * (have ? lo + j : lo) + k * f12::CW), one);
        __syncthreads();
        f12::st(f12::reg_cell(1, k), x);
        __syncthreads();
        f12::mul(0, 0, 1);
    }
    f12::store_raw(out + (size_t)F12_RAW_WORDS * gi, 0, live);
}
// out = base^e: base a GT encoding (576 B), e the low `bits` bits of the little-endian words at `e`, out a GT encoding.  Square and multiply from the top
// bit; BOTH products are taken at every bit and the result is chosen by sel -- no branch on a bit of e (the rule of pairing_tower.cuh; the eight groups
// of the one workgroup all compute the same power, group 0 writes it).  *bad |= 1 when a coefficient of base is >= p (the power is then of no use).
__global__ __launch_bounds__(64) void k_gt_pow(const uint8_t* __restrict__ base, const uint32_t* __restrict__ e, uint32_t bits, uint8_t* __restrict__ out,
                                               uint32_t* __restrict__ bad) {
    const bool ok = f12::load_gt(2, base);
    if (!ok) *bad = 1;                               // no barrier inside; every writer stores the same word
    f12::set_one(0);
    const uint32_t k = f12::coef();
    for (uint32_t i = bits; i-- > 0;) {
        const bool bit = (e[i >> 5] >> (i & 31)) & 1;
        f12::mul(0, 0, 0);
        f12::mul(1, 0, 2);
        const f12::F12C x = f12::sel<256>(bit, f12::ld<256>(f12::reg_cell(0, k)), f12::ld<256>(f12::reg_cell(1, k)));
        __syncthreads();
        f12::st(f12::reg_cell(0, k), x);
        __syncthreads();
    }
    f12::store_gt(out, 0, threadIdx.x / f12::GROUP == 0);
}
// zk_selftest_fp12: element g of n through the device functions above
__global__ __launch_bounds__(64) void k_selftest_fp12(int op, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint32_t n, uint8_t* __restrict__ out, int* flag) {
    const uint32_t g = blockIdx.x * f12::GROUPS_PER_WAVE + threadIdx.x / f12::GROUP;
    const bool live = g < n;
    const uint32_t gi = live ? g : n - 1;
    bool ok = f12::load_gt(0, a + 576 * (size_t)gi);
    if (op == 0 || op == 6) ok = f12::load_gt(1, b + 576 * (size_t)gi) && ok;
    if (!ok) *flag = 1;
    switch (op) {          // uniform
    case 0: f12::mul(0, 0, 1); break;
    case 1: f12::mul(0, 0, 0); break;
    case 2: f12::inv(5, 0, 2, 3, 4); f12::copy(0, 5); break;
    case 3: f12::conj(0, 0); break;
    case 4: f12::frob(0, 0); break;
    case 5: f12::frob(0, 0); f12::frob(0, 0); break;
    case 6: {              // b's coefficients of w^0, w^3, w^5 as a line.  The Miller cells overlay registers 1..: take the three out of register 1 first
        const Fp2B<2> l0 = f12::ld<2>(f12::reg_cell(1, 0)), l3 = f12::ld<2>(f12::reg_cell(1, 3)), l5 = f12::ld<2>(f12::reg_cell(1, 5));
        __syncthreads();
        f12::st(f12::cell(f12::C_L0), l0);
        f12::st(f12::cell(f12::C_L3), l3);
        f12::st(f12::cell(f12::C_L5), l5);
        __syncthreads();
        f12::mul_line(0, 0, f12::C_L0);
        break;
    }
    default: f12::final_exp(); break;
    }
    f12::store_gt(out + 576 * (size_t)gi, 0, live);
}

// ================================================================== host side
static constexpr uint32_t MAX_PROOFS = 1u << 24;          // 13 pairs each stay inside the 31-bit pair index

// The two pairing kernels on buffers that are ALREADY on the device: npairs checked dense affine pairs (d_g1: 96 B each, d_g2: 192 B), product q = the
// pairs [d_off[q], d_off[q + 1]) -> count GT encodings in d_gt (576 B each).  d_miller: F12_RAW_WORDS words per pair.  Enqueues, does not wait.
size_t pairing_miller_bytes(uint64_t npairs) { return (size_t)F12_RAW_WORDS * 4 * npairs; }
int pairing_miller_device(const uint8_t* d_g1, const uint8_t* d_g2, uint64_t npairs, uint32_t* d_miller, hipStream_t s) {
    if (npairs >= ((uint64_t)1 << 31)) ZK_FAIL(ZK_ERR_ARG, "pairing products: too many pairs for one call");
    if (!npairs) return ZK_OK;
    ScopedTimer t("pairing_miller", s);
    hipLaunchKernelGGL(k_miller, grid_for(npairs, f12::GROUPS_PER_WAVE), dim3(64), 0, s, d_g1, d_g2, (uint32_t)npairs, d_miller);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
int pairing_final_exp_device(const uint32_t* d_miller, const uint32_t* d_off, uint32_t count, uint8_t* d_gt, hipStream_t s) {
    ScopedTimer t("pairing_final_exp", s);
    hipLaunchKernelGGL(k_final_exp, grid_for(count, f12::GROUPS_PER_WAVE), dim3(64), 0, s, d_miller, d_off, count, d_gt);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
int pairing_products_device(const uint8_t* d_g1, const uint8_t* d_g2, uint64_t npairs, const uint32_t* d_off, uint32_t count, uint32_t* d_miller, uint8_t* d_gt, hipStream_t s) {
    ZKCHK(pairing_miller_device(d_g1, d_g2, npairs, d_miller, s));
    return pairing_final_exp_device(d_miller, d_off, count, d_gt, s);
}
// The n >= 1 raw Miller values of d_a multiplied to ONE, written to d_out: levels of k_gt_tree_mul that alternate between d_a (overwritten) and d_b
// (room for pairing_tree_scratch(n) values).  d_out may lie in neither.
uint64_t pairing_tree_scratch(uint64_t n) { return (n + GT_TREE_RUN - 1) / GT_TREE_RUN; }
int pairing_tree_product_device(uint32_t* d_a, uint32_t n, uint32_t* d_b, uint32_t* d_out, hipStream_t s) {
    ScopedTimer t("verify_fold_tree", s);
    const uint32_t* src = d_a;
    bool into_b = true;
    do {
        const uint32_t nout = (n + GT_TREE_RUN - 1) / GT_TREE_RUN;
        uint32_t* dst = nout == 1 ? d_out : into_b ? d_b : d_a;
        hipLaunchKernelGGL(k_gt_tree_mul, grid_for(nout, f12::GROUPS_PER_WAVE), dim3(64), 0, s, src, n, dst);
        HIPCHK(hipGetLastError());
        src = dst;
        n = nout;
        into_b = !into_b;
    } while (n > 1);
    return ZK_OK;
}
int pairing_gt_pow_device(const uint8_t* d_base, const uint32_t* d_exp, uint32_t bits, uint8_t* d_out, uint32_t* d_bad, hipStream_t s) {
    ScopedTimer t("verify_fold_pow", s);
    hipLaunchKernelGGL(k_gt_pow, dim3(1), dim3(64), 0, s, d_base, d_exp, bits, d_out, d_bad);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

// count products over npairs = sum lens pairs (host bytes) -> count GT encodings.  test: every point's subgroup membership too (SUBGROUP_NONE: encoding
// and curve only, the caller has checked them).  v1 / v2: the verdicts, one per pair and side; a rejected point counts as the identity.
static int run_products(const uint8_t* g1, const uint8_t* g2, uint64_t npairs, const uint64_t* lens, uint32_t count, SubgroupTest test, std::vector<uint8_t>& v1,
                        std::vector<uint8_t>& v2, uint8_t* gt_out, hipStream_t s) {
    v1.assign(npairs, 0);
    v2.assign(npairs, 0);
    if (npairs >= ((uint64_t)1 << 31)) ZK_FAIL(ZK_ERR_ARG, "pairing products: too many pairs for one call");
    std::vector<uint32_t> off(count + 1);
    uint64_t run = 0;
    for (uint32_t k = 0; k < count; k++) { off[k] = (uint32_t)run; run += lens[k]; }
    off[count] = (uint32_t)run;
    DevBuf b1, b2, a1, a2, dv, dm, doff, dgt;
    ZKCHK(b1.alloc(96 * npairs));
    ZKCHK(b2.alloc(192 * npairs));
    ZKCHK(a1.alloc(96 * npairs));
    ZKCHK(a2.alloc(192 * npairs));
    ZKCHK(dv.alloc(2 * npairs));
    ZKCHK(dm.alloc((size_t)F12_RAW_WORDS * 4 * npairs));
    ZKCHK(doff.alloc(4 * (size_t)(count + 1)));
    ZKCHK(dgt.alloc(576 * (size_t)count));
    HIPCHK(hipMemcpyAsync(doff.p, off.data(), 4 * (size_t)(count + 1), hipMemcpyHostToDevice, s));
    if (npairs) {
        HIPCHK(hipMemcpyAsync(b1.p, g1, 96 * npairs, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(b2.p, g2, 192 * npairs, hipMemcpyHostToDevice, s));
        {
            ScopedTimer t("pairing_point_checks", s);
            ZKCHK(points_decode_verdicts(CURVE_G2, a2.p, b2.p, npairs, dv.as<uint8_t>() + npairs, test, s));
            ZKCHK(points_decode_verdicts(CURVE_G1, a1.p, b1.p, npairs, dv.as<uint8_t>(), test, s));
        }
        HIPCHK(hipMemcpyAsync(v1.data(), dv.p, npairs, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(v2.data(), dv.as<uint8_t>() + npairs, npairs, hipMemcpyDeviceToHost, s));
    }
    ZKCHK(pairing_products_device(a1.as<uint8_t>(), a2.as<uint8_t>(), npairs, doff.as<uint32_t>(), count, dm.as<uint32_t>(), dgt.as<uint8_t>(), s));
    HIPCHK(hipMemcpyAsync(gt_out, dgt.p, 576 * (size_t)count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}

// ---- byte-level point helpers of the verifiers (the encodings are canonical: they passed the checks or came from the device's encoder)
static void be48_p(uint8_t out[48]) {
    for (int i = 0; i < 6; i++)
        for (int k = 0; k < 8; k++) out[8 * (5 - i) + k] = (uint8_t)(HP_P[i] >> (8 * (7 - k)));
}
// -P of a G1 encoding: y -> p - y (the identity, and y = 0, stay)
static void g1_neg_bytes(uint8_t out[96], const uint8_t in[96]) {
    memcpy(out, in, 96);
    if (in[0] & 0x40) return;
    uint8_t any = 0;
    for (int i = 48; i < 96; i++) any |= in[i];
    if (!any) return;
    uint8_t p[48];
    be48_p(p);
    int borrow = 0;
    for (int i = 47; i >= 0; i--) {
        const int d = (int)p[i] - (int)in[48 + i] - borrow;
        out[48 + i] = (uint8_t)(d & 0xff);
        borrow = d < 0 ? 1 : 0;
    }
}
static void g1_identity(uint8_t out[96]) { memset(out, 0, 96); out[0] = 0x40; }
static void g2_identity(uint8_t out[192]) { memset(out, 0, 192); out[0] = 0x40; }
static bool fr_canonical(const uint8_t* b) {          // 32-byte little-endian < r
    for (int i = 3; i >= 0; i--) {
        uint64_t w = 0;
        for (int k = 7; k >= 0; k--) w = (w << 8) | b[8 * i + k];
        if (w < HP_R[i]) return true;
        if (w > HP_R[i]) return false;
    }
    return false;
}
// out[i] = sum_k scalars[i][k] * points[k] for count scalar vectors of n over ONE point list (G.dot, curve.ml:91-103): the list goes up once as
// resident bases, one product per proof.  live[i] = 0: vector i is not multiplied (its proof is already rejected; it may hold scalars >= r).
static int dot_many(int group, const uint8_t* points, size_t n, const uint8_t* scalars, uint32_t count, const std::vector<uint8_t>& live, uint8_t* out) {
    const size_t ab = group ? 192 : 96;
    if (!n) {
        for (uint32_t i = 0; i < count; i++) { memset(out + ab * i, 0, ab); out[ab * i] = 0x40; }
        return ZK_OK;
    }
    std::vector<uint8_t> sc(scalars, scalars + 32 * n * (size_t)count);
    for (uint32_t i = 0; i < count; i++)
        if (!live[i]) memset(sc.data() + 32 * n * i, 0, 32 * n);
    const std::vector<uint64_t> lens(count, n);
    uint64_t h = 0;
    ZKCHK(zk_bases_upload(group, points, n, &h));
    const int rc = zk_msm_resident_many(h, sc.data(), lens.data(), count, out);
    (void)zk_bases_free(h);
    return rc;
}
// The front half of both verifiers.  Every point of the call through the decoder and [r] P = O, once: the proofs' points laid out per proof as the plan
// says (G1 point q of proof i at n1 i + q: the layout of k_vk_gather), the key's k1 / k2 points behind them.  A defect of the key is the call's; else
// st[i] = proof i's status (its first bad point in the host's order, then its public inputs: verdict_order.h), live[i] = its pairings are still to be taken.
static int check_call(const VkPlan& p, const uint8_t* proofs, uint32_t count, const uint8_t* key1, size_t k1, const uint8_t* key2, size_t k2,
                      KeyDefect (*key_defect)(const uint8_t*, const uint8_t*, size_t), size_t n_io, const uint8_t* io_scalars, std::vector<int32_t>& st,
                      std::vector<uint8_t>& live, hipStream_t s) {
    const size_t c = count;
    std::vector<uint8_t> p1(96 * (p.n1 * c + k1)), p2(192 * (p.n2 * c + k2)), v1, v2, bad(c, 0);
    for (size_t i = 0; i < c; i++) {
        for (uint32_t q = 0; q < p.n1; q++) memcpy(&p1[96 * (p.n1 * i + q)], proofs + p.stride * i + p.off1[q], 96);
        for (uint32_t q = 0; q < p.n2; q++) memcpy(&p2[192 * (p.n2 * i + q)], proofs + p.stride * i + p.off2[q], 192);
        for (size_t k = 0; k < n_io && !bad[i]; k++) bad[i] = !fr_canonical(io_scalars + 32 * (n_io * i + k));
    }
    if (k1) memcpy(&p1[96 * p.n1 * c], key1, 96 * k1);
    memcpy(&p2[192 * p.n2 * c], key2, 192 * k2);
    DevBuf a1, a2;          // the decoded points are not kept: the pairs go up as bytes again
    ZKCHK(points_decode_two_lists(p1.data(), p.n1 * c + k1, p2.data(), p.n2 * c + k2, "pairing_point_checks", SUBGROUP_ORDER, a1, a2, v1, v2, s));
    const KeyDefect kd = key_defect(v1.data() + p.n1 * c, v2.data() + p.n2 * c, n_io);
    if (kd.verdict) ZK_FAIL(verdict_code(kd.verdict), kd.what);
    for (uint32_t i = 0; i < count; i++) {
        st[i] = verdict_code(proof_code(p, v1.data(), v2.data(), bad.data(), i));
        live[i] = st[i] == ZK_OK;
    }
    return ZK_OK;
}

}  // namespace zk

using namespace zk;
extern "C" {

int zk_pairing_product_many(const uint8_t* g1_points, const uint8_t* g2_points, const uint64_t* lens, uint32_t count, uint8_t* gt_out) {
    if (!count) return ZK_OK;
    if (!lens || !gt_out) ZK_FAIL(ZK_ERR_ARG, "zk_pairing_product_many: null argument");
    uint64_t npairs = 0;
    for (uint32_t k = 0; k < count; k++) npairs += lens[k];
    if (npairs && (!g1_points || !g2_points)) ZK_FAIL(ZK_ERR_ARG, "zk_pairing_product_many: null argument");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    std::vector<uint8_t> v1, v2;
    ZKCHK(run_products(g1_points, g2_points, npairs, lens, count, SUBGROUP_ORDER, v1, v2, gt_out, ctx().stream));
    for (uint64_t i = 0; i < npairs; i++) {          // the host's decoding order: G1 of pair i, then G2 of pair i
        if (v1[i]) ZK_FAIL(verdict_code(v1[i]), "zk_pairing_product_many: bad G1 point (encoding, curve or subgroup)");
        if (v2[i]) ZK_FAIL(verdict_code(v2[i]), "zk_pairing_product_many: bad G2 point (encoding, curve or subgroup)");
    }
    return ZK_OK;
}

// groth16.ml:163-173:  e(A, B) = ab * e(sum_k w_k ltgm_io_k, gm) * e(C, d), as zk_groth16_verify decides it: e(A, B) e(-acc, gm) e(-C, d) == ab on bytes
int zk_groth16_verify_many(const uint8_t ab[576], const uint8_t* ltgm_io, size_t n_io, const uint8_t gm[192], const uint8_t d[192], const uint8_t* io_scalars,
                           const uint8_t* proofs, uint32_t count, uint8_t* ok, int32_t* status) {
    if (!ab || !gm || !d || (n_io && !ltgm_io)) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_verify_many: null argument");
    if (!count) return ZK_OK;
    if (!proofs || !ok || (n_io && !io_scalars)) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_verify_many: null argument");
    if (count > MAX_PROOFS) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_verify_many: more than 2^24 proofs in one call");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    uint8_t key2[384];
    memcpy(key2, gm, 192);
    memcpy(key2 + 192, d, 192);
    std::vector<int32_t> st(count);
    std::vector<uint8_t> live(count), v1, v2;
    ZKCHK(check_call(PLAN_GROTH16, proofs, count, ltgm_io, n_io, key2, 2, groth16_key_defect, n_io, io_scalars, st, live, s));
    std::vector<uint8_t> acc(96 * (size_t)count);
    ZKCHK(dot_many(0, ltgm_io, n_io, io_scalars, count, live, acc.data()));
    std::vector<uint8_t> q1(96 * 3 * (size_t)count), q2(192 * 3 * (size_t)count), gt(576 * (size_t)count);
    for (uint32_t i = 0; i < count; i++) {
        uint8_t* a = &q1[96 * 3 * (size_t)i];
        uint8_t* b = &q2[192 * 3 * (size_t)i];
        if (!live[i]) {          // three pairs that contribute 1
            for (int k = 0; k < 3; k++) { g1_identity(a + 96 * k); g2_identity(b + 192 * k); }
            continue;
        }
        memcpy(a, proofs + 384 * (size_t)i, 96);
        g1_neg_bytes(a + 96, &acc[96 * (size_t)i]);
        g1_neg_bytes(a + 192, proofs + 384 * (size_t)i + 288);
        memcpy(b, proofs + 384 * (size_t)i + 96, 192);
        memcpy(b + 192, gm, 192);
        memcpy(b + 384, d, 192);
    }
    const std::vector<uint64_t> lens(count, 3);
    ZKCHK(run_products(q1.data(), q2.data(), 3 * (uint64_t)count, lens.data(), count, SUBGROUP_NONE, v1, v2, gt.data(), s));
    for (uint32_t i = 0; i < count; i++) {
        ok[i] = live[i] && memcmp(&gt[576 * (size_t)i], ab, 576) == 0 ? 1 : 0;
        if (status) status[i] = st[i];
    }
    return ZK_OK;
}

// Verify.f, pinocchio.ml:254-420, as zk_pinocchio_verify decides it: five products of pairings, each equal to 1.
//   vk_g1 = one | aw | bgm | vv_io[n_io] | yy_io[n_io]      vk_g2 = one2 | av | ay | gm2 | bgm2 | yt | ww_io[n_io]
//   proof = vv | ww (G2) | yy | h | vavv | waww (G2) | yayy | bvwy
int zk_pinocchio_verify_many(const uint8_t* vk_g1, const uint8_t* vk_g2, size_t n_io, const uint8_t* io_scalars, const uint8_t* proofs, uint32_t count, uint8_t* ok,
                             int32_t* status) {
    if (!vk_g1 || !vk_g2) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_verify_many: null argument");
    if (!count) return ZK_OK;
    if (!proofs || !ok || (n_io && !io_scalars)) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_verify_many: null argument");
    if (count > MAX_PROOFS) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_verify_many: more than 2^24 proofs in one call");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    const size_t c = count;
    std::vector<int32_t> st(count);
    std::vector<uint8_t> live(count), v1, v2;
    ZKCHK(check_call(PLAN_PINOCCHIO, proofs, count, vk_g1, 3 + 2 * n_io, vk_g2, 6 + n_io, pinocchio_key_defect, n_io, io_scalars, st, live, s));
    // vio, yio, wio (G.dot over the public inputs), then vio + vv, yio + yy, wio + ww
    std::vector<uint8_t> vio(96 * c), yio(96 * c), wio(192 * c), pv(96 * c), py(96 * c), pw(192 * c);
    ZKCHK(dot_many(0, vk_g1 + 96 * 3, n_io, io_scalars, count, live, vio.data()));
    ZKCHK(dot_many(0, vk_g1 + 96 * (3 + n_io), n_io, io_scalars, count, live, yio.data()));
    ZKCHK(dot_many(1, vk_g2 + 192 * 6, n_io, io_scalars, count, live, wio.data()));
    for (size_t i = 0; i < c; i++) {
        if (live[i]) {
            memcpy(&pv[96 * i], proofs + 960 * i, 96);
            memcpy(&py[96 * i], proofs + 960 * i + 288, 96);
            memcpy(&pw[192 * i], proofs + 960 * i + 96, 192);
        } else {
            g1_identity(&pv[96 * i]);
            g1_identity(&py[96 * i]);
            g2_identity(&pw[192 * i]);
        }
    }
    std::vector<uint8_t> vsum(96 * c), ysum(96 * c), wsum(192 * c);
    ZKCHK(points_add_pairs(CURVE_G1, vio.data(), pv.data(), c, vsum.data(), s));
    ZKCHK(points_add_pairs(CURVE_G1, yio.data(), py.data(), c, ysum.data(), s));
    ZKCHK(points_add_pairs(CURVE_G2, wio.data(), pw.data(), c, wsum.data(), s));
    // the five equations, 13 pairs per proof
    const uint8_t *one = vk_g1, *aw = vk_g1 + 96, *bgm = vk_g1 + 192;
    const uint8_t *one2 = vk_g2, *av = vk_g2 + 192, *ay = vk_g2 + 384, *gm2 = vk_g2 + 576, *bgm2 = vk_g2 + 768, *yt = vk_g2 + 960;
    std::vector<uint8_t> q1(96 * 13 * c), q2(192 * 13 * c), gt(576 * 5 * c);
    std::vector<uint64_t> lens(5 * c);
    for (size_t i = 0; i < c; i++) {
        uint8_t* a = &q1[96 * 13 * i];
        uint8_t* b = &q2[192 * 13 * i];
        static const uint64_t L[5] = {2, 2, 2, 4, 3};
        for (int q = 0; q < 5; q++) lens[5 * i + q] = L[q];
        if (!live[i]) {
            for (int k = 0; k < 13; k++) { g1_identity(a + 96 * k); g2_identity(b + 192 * k); }
            continue;
        }
        const uint8_t* pr = proofs + 960 * i;
        const uint8_t *vv = pr, *ww = pr + 96, *yy = pr + 288, *h = pr + 384, *vavv = pr + 480, *waww = pr + 576, *yayy = pr + 768, *bvwy = pr + 864;
        int k = 0;
        auto pair = [&](const uint8_t* g1p, bool neg, const uint8_t* g2p) {
            if (neg) g1_neg_bytes(a + 96 * k, g1p);
            else memcpy(a + 96 * k, g1p, 96);
            memcpy(b + 192 * k, g2p, 192);
            k++;
        };
        pair(vv, false, av); pair(vavv, true, one2);                                                         // :285
        pair(aw, false, ww); pair(one, true, waww);                                                          // :298
        pair(yy, false, ay); pair(yayy, true, one2);                                                         // :311
        pair(bvwy, false, gm2); pair(vv, true, bgm2); pair(bgm, true, ww); pair(yy, true, bgm2);             // :361-366
        pair(&vsum[96 * i], false, &wsum[192 * i]); pair(&ysum[96 * i], true, one2); pair(h, true, yt);      // :418-420
    }
    ZKCHK(run_products(q1.data(), q2.data(), 13 * (uint64_t)c, lens.data(), 5 * count, SUBGROUP_NONE, v1, v2, gt.data(), s));
    uint8_t gt_one[576];
    gt_one_bytes(gt_one);
    for (size_t i = 0; i < c; i++) {
        bool good = live[i] != 0;
        for (int q = 0; q < 5; q++) good = good && memcmp(&gt[576 * (5 * i + q)], gt_one, 576) == 0;
        ok[i] = good ? 1 : 0;
        if (status) status[i] = st[i];
    }
    return ZK_OK;
}

int zk_selftest_fp12(int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) {
    if (!a || !out || !n || op < 0 || op > 7 || ((op == 0 || op == 6) && !b) || n >= ((size_t)1 << 24))
        ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp12: null argument, no elements, or an operation outside 0..7");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    DevBuf da, db, dout, flag;
    ZKCHK(da.alloc(576 * n));
    ZKCHK(db.alloc(576 * n));
    ZKCHK(dout.alloc(576 * n));
    ZKCHK(flag.alloc(4));
    HIPCHK(hipMemsetAsync(flag.p, 0, 4, s));
    HIPCHK(hipMemcpyAsync(da.p, a, 576 * n, hipMemcpyHostToDevice, s));
    if (b) HIPCHK(hipMemcpyAsync(db.p, b, 576 * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_selftest_fp12, grid_for(n, f12::GROUPS_PER_WAVE), dim3(64), 0, s, op, (const uint8_t*)da.as<uint8_t>(), (const uint8_t*)db.as<uint8_t>(), (uint32_t)n,
                       dout.as<uint8_t>(), flag.as<int>());
    HIPCHK(hipGetLastError());
    int h = 0;
    HIPCHK(hipMemcpyAsync(&h, flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out, dout.p, 576 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp12: a coefficient is >= p");
    return ZK_OK;
}
}
