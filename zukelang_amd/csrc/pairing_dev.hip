// Pairings in batches on the device (scope row f1): many products of pairings per call.  This file holds the pairing kernels, the pairing_*_device entries
// that enqueue them on device buffers, zk_pairing_product_many (include/zkmi355x.h) and zk_selftest_fp12 -- and no verifier: the batched and the resident
// verifiers are one pipeline in verify_resident.hip, which calls the entries below.  The single-proof verifiers stay on the host (pairing_host.hip, which
// this file does not touch: the host-only sanitizer library is built from it alone).  Same definition, same bytes: Pairing.pairing of curve.mli:46-54.
//
//   bytes -> affine + one verdict per point    (zk_pairing_product_many) k_bytes_to_affine_verdict, k_subgroup_verdict by [r] P = O (msm_points.hip: one lane
//                                               per point); the first bad point in the host's decoding order fails the call
//   Miller loops                                k_miller: one group of 8 lanes per PAIR (pairing_tower.cuh), inversion-free, 63 steps
//   products + final exponentiations            k_final_exp: one group per PRODUCT multiplies its pairs' Miller values and raises to (p^12 - 1) / r
//   one long product (the folded verifier)      k_gt_tree_mul: one group per RUN of GT_TREE_RUN raw Miller values, level after level until one is left;
//                                               k_gt_pow: a GT encoding raised to an exponent read from device memory (square and multiply, both every bit)
//
// A batch is bound by latency, not by the multipliers: one G2 subgroup check is ~15 k base-field products on one lane, a Miller loop ~2.6 k and a
// final exponentiation ~7 k per lane of a group, and every pair and product of the batch does them side by side (profiles/verify_many.json).
#include "pairing_tower.cuh"

#include "msm.cuh"
#include "verdict_order.h"

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

}  // namespace zk

using namespace zk;
extern "C" {

// count products over npairs = sum lens pairs (host bytes) -> count GT encodings (Pairing.pairing, curve.mli:46-54): every point decoded and held to the
// curve and the subgroup once, then the two kernels; a rejected point counts as the identity and fails the call
int zk_pairing_product_many(const uint8_t* g1_points, const uint8_t* g2_points, const uint64_t* lens, uint32_t count, uint8_t* gt_out) {
    if (!count) return ZK_OK;
    if (!lens || !gt_out) ZK_FAIL(ZK_ERR_ARG, "zk_pairing_product_many: null argument");
    uint64_t npairs = 0;
    for (uint32_t k = 0; k < count; k++) npairs += lens[k];
    if (npairs && (!g1_points || !g2_points)) ZK_FAIL(ZK_ERR_ARG, "zk_pairing_product_many: null argument");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    if (npairs >= ((uint64_t)1 << 31)) ZK_FAIL(ZK_ERR_ARG, "pairing products: too many pairs for one call");
    std::vector<uint32_t> off(count + 1);
    uint64_t run = 0;
    for (uint32_t k = 0; k < count; k++) { off[k] = (uint32_t)run; run += lens[k]; }
    off[count] = (uint32_t)run;
    DevBuf a1, a2, dm, doff, dgt;
    std::vector<uint8_t> v1, v2;
    ZKCHK(points_decode_two_lists(g1_points, npairs, g2_points, npairs, "pairing_point_checks", SUBGROUP_ORDER, a1, a2, v1, v2, s));
    ZKCHK(dm.alloc(pairing_miller_bytes(npairs)));
    ZKCHK(doff.alloc(4 * (size_t)(count + 1)));
    ZKCHK(dgt.alloc(576 * (size_t)count));
    HIPCHK(hipMemcpyAsync(doff.p, off.data(), 4 * (size_t)(count + 1), hipMemcpyHostToDevice, s));
    ZKCHK(pairing_products_device(a1.as<uint8_t>(), a2.as<uint8_t>(), npairs, doff.as<uint32_t>(), count, dm.as<uint32_t>(), dgt.as<uint8_t>(), s));
    HIPCHK(hipMemcpyAsync(gt_out, dgt.p, 576 * (size_t)count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < npairs; i++) {          // the host's decoding order: G1 of pair i, then G2 of pair i
        if (v1[i]) ZK_FAIL(verdict_code(v1[i]), "zk_pairing_product_many: bad G1 point (encoding, curve or subgroup)");
        if (v2[i]) ZK_FAIL(verdict_code(v2[i]), "zk_pairing_product_many: bad G2 point (encoding, curve or subgroup)");
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
