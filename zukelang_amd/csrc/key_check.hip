// zk_groth16_key_check (include/zkmi355x.h): a tau-power proving key, as it lies in a handle, against its circuit and -- when given -- the
// verification key its proofs will be judged under.
//
// Every relation of the key (groth16.ml:45-108) is an equation between exponents, one per index; each family of them is tested as ONE random linear
// combination over all its indices, which holds for every index or fails with probability 1 - 1/r over the coefficients:
//   rho   (n + 2)  the tau powers           sigma (n - 1)  the h bases [tau^i Z(tau) / delta]           mu (m)  the per-variable points [L_k(tau) / delta | gamma]
// The sums over the pools are products over the handle's own window tables (msm_run; eight in G1, three in G2: the work of four proofs); the coefficient
// vectors of sum_k mu_k v_k, w_k, y_k come from the prover's own Fr stage with mu in the witness's place (pinocchio.hip: pin_compact_check does the same
// for Pinocchio's compact pool), y through the stage's interpolation entry; the two sides of each equation are pairing products on the device
// (pairing_dev.hip) compared as GT bytes.  Nothing of the handle is written: scratch, workspaces and scalar vectors live for the call.
// zk_groth16_key_check_lagrange, the same for a Lagrange-form handle, follows it below: other relations, the same shape.
#include "ec.cuh"
#include "groth16_key.cuh"
#include "seed_expand.cuh"
#include "verdict_order.h"

#include <string.h>
#include <vector>

namespace zk {

static inline dim3 g1d(uint64_t n, unsigned t = 256) { return dim3((unsigned)((n + t - 1) / t)); }

// out[i]: the seed's expansion (seed_expand.cuh: pseudo-random canonical scalars below 2^254).  Elements from mu_first on are the per-variable
// coefficients mu_k; with zero_io those of the variables outside mids are 0 (no verification key: their points are not in the proving key).
__global__ void k_keychk_expand(uint32_t* __restrict__ out, uint64_t count, uint64_t mu_first, const uint8_t* __restrict__ is_mid, int zero_io, KeychkSeed seed) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    Fr r = seed_expand_at(seed, i);
    if (zero_io && i >= mu_first && !is_mid[i - mu_first]) r = fe_zero<FrParams>();
    fe_store<FrParams>(out + 8 * i, r);
}
// All scalar vectors of the check over the pool layouts g1 = a | d1 | b1 | ti1[n+2] | tiztd[n-1] | ltd_mid, g2 = b2 | d2 | ti2[n+2], in one pass (canonical).
//   G1, vector q at out1 + 8 q p1:  0: rho_(i-1) on ti1[i], 1 <= i <= n+1     1: rho_i on ti1[i], i <= n     2: rho_i on ti1[i], i <= n+1     3: sigma on tiztd
//                                    4: sigma_i on ti1[i], i < n-1    5: mu on ltd_mid    6: coefficients of sum mu_k v_k on ti1    7: of sum mu_k y_k on ti1
//   G2, vector q at out2 + 8 q p2:  0: rho_i on ti2[i], i <= n+1     1: the coefficients of Z on ti2     2: coefficients of sum mu_k w_k on ti2
// rnd = rho | sigma | mu (canonical); vco, wco, yco, z in Montgomery form.
static constexpr int KEYCHK_G1_VECS = 8, KEYCHK_G2_VECS = 3;
struct KeychkVecs {
    const uint32_t *rnd, *vco, *wco, *yco, *z, *mid_idx;
    uint32_t n, n_mid;
};
__global__ void k_keychk_scalars(uint32_t* __restrict__ out1, uint32_t* __restrict__ out2, KeychkVecs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = a.n, nt = n + 2, ti = 3, tz = ti + nt, lt = tz + (n - 1), p1 = lt + a.n_mid, p2 = 2 + nt;
    if (i >= p1) return;
    const uint32_t* rho = a.rnd;
    const uint32_t* sigma = rho + 8 * nt;
    const uint32_t* mu = sigma + 8 * (n - 1);
    const Fr zero = fe_zero<FrParams>();
    Fr x[KEYCHK_G1_VECS];
#pragma unroll
    for (int q = 0; q < KEYCHK_G1_VECS; q++) x[q] = zero;
    if (i >= ti && i < tz) {
        const uint64_t k = i - ti;          // the power of tau, k <= n + 1
        const Fr rk = fe_load<FrParams>(rho + 8 * k);
        if (k >= 1) x[0] = fe_load<FrParams>(rho + 8 * (k - 1));
        if (k <= n) x[1] = rk;
        x[2] = rk;
        if (k + 1 < n) x[4] = fe_load<FrParams>(sigma + 8 * k);
        if (k < n) {
            x[6] = fe_from_mont(fe_load<FrParams>(a.vco + 8 * k));
            x[7] = fe_from_mont(fe_load<FrParams>(a.yco + 8 * k));
        }
    } else if (i >= tz && i < lt) x[3] = fe_load<FrParams>(sigma + 8 * (i - tz));
    else if (i >= lt) x[5] = fe_load<FrParams>(mu + 8 * (uint64_t)a.mid_idx[i - lt]);
#pragma unroll
    for (int q = 0; q < KEYCHK_G1_VECS; q++) fe_store<FrParams>(out1 + 8 * (q * p1 + i), x[q]);
    if (i < p2) {
        Fr y[KEYCHK_G2_VECS] = {zero, zero, zero};
        if (i >= 2) {
            const uint64_t k = i - 2;
            y[0] = fe_load<FrParams>(rho + 8 * k);
            if (k <= n) y[1] = fe_from_mont(fe_load<FrParams>(a.z + 8 * k));
            if (k < n) y[2] = fe_from_mont(fe_load<FrParams>(a.wco + 8 * k));
        }
#pragma unroll
        for (int q = 0; q < KEYCHK_G2_VECS; q++) fe_store<FrParams>(out2 + 8 * (q * p2 + i), y[q]);
    }
}
// out[j] = mu[io_idx[j]]: the coefficients of the verification key's ltgm_io, in its order
__global__ void k_keychk_gather(uint32_t* __restrict__ out, const uint32_t* __restrict__ mu, const uint32_t* __restrict__ io_idx, uint64_t n_io) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_io) return;
    fe_store<FrParams>(out + 8 * j, fe_load<FrParams>(mu + 8 * (uint64_t)io_idx[j]));
}

static inline bool is_identity_bytes(const uint8_t* p) { return (p[0] & 0x40) != 0; }

// Product q = the pairs lens[0] + .. + lens[q-1] onwards, lens[q] of them, of P (96 B each) and Q (192 B each) -> gt: 576 B per product; waits.
// The products of zk_pairing_product_many without its point checks: every point here is a key point the upload checked (in_subgroup), a point of the
// verification key the caller checked, or a sum of such points -- [r] P = O on sixteen pairs would cost more than all the Miller loops.
int keychk_pairing_products(const std::vector<uint8_t>& P, const std::vector<uint8_t>& Q, const std::vector<uint64_t>& lens, std::vector<uint8_t>& gt, hipStream_t s) {
    const uint32_t count = (uint32_t)lens.size();
    gt.resize(576 * (size_t)count);
    std::vector<uint32_t> off(count + 1, 0);
    for (uint32_t j = 0; j < count; j++) off[j + 1] = off[j] + (uint32_t)lens[j];
    const uint64_t npairs = off[count];
    DevBuf pb, qb, pa, qa, dm, doff, dgt, flag;
    ZKCHK(pb.alloc(96 * npairs));
    ZKCHK(qb.alloc(192 * npairs));
    ZKCHK(pa.alloc(96 * npairs));
    ZKCHK(qa.alloc(192 * npairs));
    ZKCHK(dm.alloc(pairing_miller_bytes(npairs)));
    ZKCHK(doff.alloc(4 * (size_t)(count + 1)));
    ZKCHK(dgt.alloc(576 * (size_t)count));
    ZKCHK(flag.alloc(4));
    HIPCHK(hipMemsetAsync(flag.p, 0, 4, s));
    HIPCHK(hipMemcpyAsync(pb.p, P.data(), P.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(qb.p, Q.data(), Q.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(doff.p, off.data(), 4 * (size_t)(count + 1), hipMemcpyHostToDevice, s));
    ZKCHK(points_bytes_to_affine(CURVE_G1, pa.p, pb.p, npairs, flag.as<int>(), s));
    ZKCHK(points_bytes_to_affine(CURVE_G2, qa.p, qb.p, npairs, flag.as<int>(), s));
    ZKCHK(pairing_products_device(pa.as<uint8_t>(), qa.as<uint8_t>(), npairs, doff.as<uint32_t>(), count, dm.as<uint32_t>(), dgt.as<uint8_t>(), s));
    int hf = 0;
    HIPCHK(hipMemcpyAsync(&hf, flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(gt.data(), dgt.p, gt.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (hf) ZK_FAIL(ZK_ERR_HIP, "a point of the check's own making does not decode");
    return ZK_OK;
}

int groth16_key_check(Groth16Key& k, const uint8_t* vk_g1, size_t n_io, const uint8_t* vk_g2, const uint8_t* seed, uint32_t* failed) {
    const bool have_vk = vk_g1 && vk_g2;
    const uint32_t n = k.n, m = k.m, n_mid = k.n_mid;
    const uint64_t p1 = k.p1, p2 = k.p2, nt = (uint64_t)n + 2;
    DeviceScope ds(k.vdev);
    Ctx& c = ctx();
    hipStream_t s = c.stream;
    HIPCHK(hipGetLastError());
    const KeychkSeed sd = seed_take(seed);
    // which variable has its point where: mids in the key's ltd_mid (mid_idx), the others in the verification key's ltgm_io, both in variable order
    std::vector<uint32_t> mids(n_mid ? n_mid : 1), io_idx;
    if (n_mid) HIPCHK(hipMemcpy(mids.data(), k.mid_idx.p, 4 * (size_t)n_mid, hipMemcpyDeviceToHost));
    std::vector<uint8_t> is_mid(m, 0);
    for (uint32_t j = 0; j < n_mid; j++) is_mid[mids[j]] = 1;
    for (uint32_t v = 0; v < m; v++)
        if (!is_mid[v]) io_idx.push_back(v);
    // the verification key's points, decoded and checked like those of zk_groth16_vk_upload (endomorphism subgroup test, its codes): G2 list, then G1 list
    DevBuf vk1, vk2;
    if (have_vk) {
        std::vector<uint8_t> v1, v2;
        ZKCHK(points_decode_two_lists(vk_g1, 1 + n_io, vk_g2, 3, "key_check", SUBGROUP_ENDO, vk1, vk2, v1, v2, s));
        for (uint8_t v : v2)
            if (v) ZK_FAIL(verdict_code(v), "zk_groth16_key_check: bad G2 point in the verification key (one2 | gm | d: encoding, curve or subgroup)");
        for (uint8_t v : v1)
            if (v) ZK_FAIL(verdict_code(v), "zk_groth16_key_check: bad G1 point in the verification key (one1 | ltgm_io: encoding, curve or subgroup)");
    }
    const uint64_t nrnd = nt + (n - 1) + m;
    const size_t g1x = xyzz_bytes(CURVE_G1), g2x = xyzz_bytes(CURVE_G2);
    FrScratch fs;
    MsmWorkspace w1, w2;
    DevBuf rnd, vw, scal1, scal2, res1, res2, d_is_mid, d_io_idx;
    ZKCHK(frstage_scratch_alloc(k.fr, fs));
    ZKCHK(msm_workspace_alloc(w1, k.g1));
    ZKCHK(msm_workspace_alloc(w2, k.g2));
    ZKCHK(rnd.alloc(32 * nrnd));
    ZKCHK(vw.alloc(32 * (size_t)2 * k.fr.n2));
    ZKCHK(scal1.alloc(32 * KEYCHK_G1_VECS * p1));
    ZKCHK(scal2.alloc(32 * KEYCHK_G2_VECS * p2));
    ZKCHK(res1.alloc(g1x * (KEYCHK_G1_VECS + 1)));          // + the product over ltgm_io
    ZKCHK(res2.alloc(g2x * KEYCHK_G2_VECS));
    ZKCHK(d_is_mid.alloc(m));
    ZKCHK(d_io_idx.alloc(4 * (io_idx.size() ? io_idx.size() : 1)));
    HIPCHK(hipMemcpyAsync(d_is_mid.p, is_mid.data(), m, hipMemcpyHostToDevice, s));
    if (!io_idx.empty()) HIPCHK(hipMemcpyAsync(d_io_idx.p, io_idx.data(), 4 * io_idx.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(res1.p, 0, res1.bytes, s));          // zz = 0: the identity, for the sums that have no term
    HIPCHK(hipMemsetAsync(res2.p, 0, res2.bytes, s));
    uint32_t* mu = rnd.as<uint32_t>() + 8 * (nt + (n - 1));
    {
        ScopedTimer t("key_check", s);
        hipLaunchKernelGGL(k_keychk_expand, g1d(nrnd), dim3(256), 0, s, rnd.as<uint32_t>(), nrnd, nt + (n - 1), (const uint8_t*)d_is_mid.as<uint8_t>(), have_vk ? 0 : 1, sd);
        HIPCHK(hipGetLastError());
    }
    // v_mu = sum_k mu_k v_k and w_mu as coefficient vectors (mu satisfies no gate: flags and h are not read), then y_mu: the interpolant of O mu
    ZKCHK(frstage_eval(k.fr, fs, mu, s));
    HIPCHK(hipMemcpyAsync(vw.p, fs.d.p, 32 * (size_t)2 * k.fr.n2, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(fs.abc.p, fs.abc.as<uint8_t>() + 32 * (size_t)2 * n, 32 * (size_t)n, hipMemcpyDeviceToDevice, s));
    ZKCHK(frstage_interpolate(k.fr, fs, s));
    {
        ScopedTimer t("key_check", s);
        KeychkVecs a{rnd.as<uint32_t>(), vw.as<uint32_t>(), vw.as<uint32_t>() + 8 * (uint64_t)k.fr.n2, fs.d.as<uint32_t>(), k.fr.z.as<uint32_t>(), k.mid_idx.as<uint32_t>(), n, n_mid};
        hipLaunchKernelGGL(k_keychk_scalars, g1d(p1), dim3(256), 0, s, scal1.as<uint32_t>(), scal2.as<uint32_t>(), a);
        HIPCHK(hipGetLastError());
    }
    // which sums have a term at all (a product over all-zero scalars is skipped: its result stays the identity)
    const bool l_live = have_vk || n_mid > 0;
    const bool run1[KEYCHK_G1_VECS] = {true, true, true, n > 1, n > 1, n_mid > 0, l_live, l_live};
    const bool run2[KEYCHK_G2_VECS] = {true, true, l_live};
    for (int q = 0; q < KEYCHK_G1_VECS; q++)
        if (run1[q]) ZKCHK(msm_run(k.g1, w1, scal1.as<uint8_t>() + 32 * q * p1, res1.as<uint8_t>() + g1x * q, s));
    for (int q = 0; q < KEYCHK_G2_VECS; q++)
        if (run2[q]) ZKCHK(msm_run(k.g2, w2, scal2.as<uint8_t>() + 32 * q * p2, res2.as<uint8_t>() + g2x * q, s));
    // sum_k mu_k ltgm_io[k] over the verification key's own points: a base set that lives for this product
    MsmBases io;
    MsmWorkspace wio;
    DevBuf mu_io;
    if (have_vk && n_io) {
        ZKCHK(msm_bases_from_device_affine(io, CURVE_G1, vk1.as<uint8_t>() + 96, n_io, 0, false, s, true));
        ZKCHK(msm_workspace_alloc(wio, io));
        ZKCHK(mu_io.alloc(32 * n_io));
        {
            ScopedTimer t("key_check", s);
            hipLaunchKernelGGL(k_keychk_gather, g1d(n_io), dim3(256), 0, s, mu_io.as<uint32_t>(), (const uint32_t*)mu, (const uint32_t*)d_io_idx.as<uint32_t>(), (uint64_t)n_io);
            HIPCHK(hipGetLastError());
        }
        ZKCHK(msm_run(io, wio, mu_io.p, res1.as<uint8_t>() + g1x * KEYCHK_G1_VECS, s));
    }
    // the key's single points and the generators, as bytes: a | d1 | b1 | ti1[0], b2 | d2 | ti2[0] | ti2[1], [1]_1, [1]_2
    DevBuf dn1, dn2, one;
    ZKCHK(dn1.alloc(96 * 5 * 2));
    ZKCHK(dn2.alloc(192 * 5 * 2));
    ZKCHK(one.alloc(32));
    const uint8_t one_le[32] = {1};
    HIPCHK(hipMemcpyAsync(one.p, one_le, 32, hipMemcpyHostToDevice, s));
    ZKCHK(msm_bases_dense(k.g1, 0, 4, dn1.p, s));
    ZKCHK(msm_bases_dense(k.g2, 0, 4, dn2.p, s));
    ZKCHK(fixed_base_mul(CURVE_G1, dn1.as<uint8_t>() + 96 * 4, one.p, 1, s));
    ZKCHK(fixed_base_mul(CURVE_G2, dn2.as<uint8_t>() + 192 * 4, one.p, 1, s));
    ZKCHK(points_affine_to_bytes(CURVE_G1, dn1.as<uint8_t>() + 96 * 5, dn1.p, 5, s));
    ZKCHK(points_affine_to_bytes(CURVE_G2, dn2.as<uint8_t>() + 192 * 5, dn2.p, 5, s));
    uint8_t kp1[5][96], kp2[5][192], s1[KEYCHK_G1_VECS + 1][96], s2[KEYCHK_G2_VECS][192];
    HIPCHK(hipMemcpyAsync(kp1, dn1.as<uint8_t>() + 96 * 5, sizeof kp1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(kp2, dn2.as<uint8_t>() + 192 * 5, sizeof kp2, hipMemcpyDeviceToHost, s));
    ZKCHK(points_xyzz_to_bytes(CURVE_G1, res1.p, KEYCHK_G1_VECS + 1, &s1[0][0], s));          // synchronises
    ZKCHK(points_xyzz_to_bytes(CURVE_G2, res2.p, KEYCHK_G2_VECS, &s2[0][0], s));
    const uint8_t *al = kp1[0], *d1 = kp1[1], *b1 = kp1[2], *g1 = kp1[3], *gen1 = kp1[4];
    const uint8_t *b2 = kp2[0], *d2 = kp2[1], *g2 = kp2[2], *tau2 = kp2[3], *gen2 = kp2[4];
    const uint8_t *gm = have_vk ? vk_g2 + 192 : nullptr, *vkd = have_vk ? vk_g2 + 384 : nullptr;

    // ---- the twelve pairing products: relation j holds iff product 2j equals product 2j + 1
    std::vector<uint8_t> P, Q;
    std::vector<uint64_t> lens;
    auto product = [&](std::initializer_list<std::pair<const uint8_t*, const uint8_t*>> pairs) {
        for (const auto& pq : pairs) {
            P.insert(P.end(), pq.first, pq.first + 96);
            Q.insert(Q.end(), pq.second, pq.second + 192);
        }
        lens.push_back(pairs.size());
    };
    product({{s1[0], g2}});                 product({{s1[1], tau2}});                                // tau powers in G1
    product({{s1[2], g2}});                 product({{g1, s2[0]}});                                  // tau powers in G2
    product({{b1, g2}});                    product({{g1, b2}});                                     // beta
    product({{d1, g2}});                    product({{g1, d2}});                                     // delta
    product({{s1[3], d2}});                 product({{s1[4], s2[1]}});                               // h bases
    if (have_vk) product({{s1[5], d2}, {s1[8], gm}});
    else product({{s1[5], d2}});
    product({{s1[6], b2}, {al, s2[2]}, {s1[7], g2}});                                                  // L_k
    std::vector<uint8_t> gt;
    ZKCHK(keychk_pairing_products(P, Q, lens, gt, s));
    auto differ = [&](int j) { return memcmp(gt.data() + 576 * (2 * j), gt.data() + 576 * (2 * j + 1), 576) != 0; };
    uint32_t f = 0;
    if (memcmp(g1, gen1, 96) || memcmp(g2, gen2, 192) || (have_vk && (memcmp(vk_g1, gen1, 96) || memcmp(vk_g2, gen2, 192)))) f |= ZK_KEYCHK_GENERATORS;
    if (differ(0)) f |= ZK_KEYCHK_TAU_G1;
    if (differ(1)) f |= ZK_KEYCHK_TAU_G2;
    if (differ(2)) f |= ZK_KEYCHK_BETA;
    if (differ(3) || is_identity_bytes(d1) || is_identity_bytes(d2) || (have_vk && memcmp(vkd, d2, 192))) f |= ZK_KEYCHK_DELTA;
    if (differ(4)) f |= ZK_KEYCHK_H_BASES;
    if (differ(5)) f |= ZK_KEYCHK_L;
    if (have_vk && is_identity_bytes(gm)) f |= ZK_KEYCHK_GAMMA;
    *failed = f;
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}

// ---------------------------------------------------------------- zk_groth16_key_check_lagrange (include/zkmi355x.h)
// A Lagrange-form key holds no tau power, not even [tau]_2: its relations are stated on VALUES.  With w_i the barycentric weights of 0..n-1,
// g1 := sum l1, g2 := sum l2 and T2 := sum i l2[i] (honestly [1]_1, [1]_2, [tau]_2), one equation per index:
//   TAU_G2   l1[i] g2 = g1 l2[i]                                           rho (n)
//   TAU_G1   l1[i] (i g2 - T2) proportional to w_i                         pi (n) with sum w_i pi_i = 0: the values on 0..n-1 of a polynomial q of degree <= n-2
//   H_BASES  w_0 hl[t] d2 = l2[0] sum_i i lambda_t(i) l1[i]                sigma_t = q(n + t): pi = sum_t sigma_t lambda_t on 0..n-1, so the right sides add up to
//                                                                          S = sum_i i pi_i l1[i], the sum TAU_G1 has made already
//   L        ltd_mid[k] d2 (or ltgm_io[k] gm) = (L^T l1)_k b2 + a (R^T l2)_k + (O^T l1)_k g2          mu (m): the sums over k are L mu, R mu, O mu over l1 / l2
// pi comes from a raw vector r without a division (pi_i = r_i / (n-1)!, i < n-1; pi_(n-1) = - sum_{i<n-1} w_i r_i: the dot product with w is
// frstage_leading_coeffs), sigma from pi by the stage's own extrapolation (frstage_extrapolate), L mu | R mu | O mu from the stage with mu in the witness's
// place.  No basis conversion anywhere.  Twelve products over the handle's window tables, twelve pairing products.
// abc[i] = r_i in Montgomery form for i < n - 1, 0 for n - 1 <= i < 2n: what frstage_leading_coeffs reads, with the last term left out
__global__ void k_keychk_lag_raw(uint32_t* __restrict__ abc, const uint32_t* __restrict__ r, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * (uint64_t)n) return;
    Fr x = fe_zero<FrParams>();
    if (i + 1 < n) x = fe_to_mont(fe_load<FrParams>(r + 8 * i));
    fe_store<FrParams>(abc + 8 * i, x);
}
// pi (Montgomery): pi_i = raw_i / (n-1)! for i < n - 1, pi_(n-1) = -kappa
__global__ void k_keychk_lag_pi(uint32_t* __restrict__ pi, const uint32_t* __restrict__ raw, const uint32_t* __restrict__ kappa, const uint32_t* __restrict__ invfact, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fr x = i + 1 < n ? fe_mul(fe_load<FrParams>(raw + 8 * i), fe_load<FrParams>(invfact + 8 * (uint64_t)(n - 1))) : fe_neg(fe_load<FrParams>(kappa));
    fe_store<FrParams>(pi + 8 * i, x);
}
// All scalar vectors of the check over the pool layouts g1 = a | d1 | b1 | l1[n] | hl[n-1] | ltd_mid, g2 = b2 | d2 | l2[n], in one pass (canonical).
//   G1, vector q at out1 + 8 q p1:  0: 1 on l1     1: rho on l1     2: pi on l1     3: i pi_i on l1     4: w_0 sigma on hl     5: mu on ltd_mid
//                                    6: L mu on l1     7: O mu on l1
//   G2, vector q at out2 + 8 q p2:  0: 1 on l2     1: rho on l2     2: i on l2     3: R mu on l2
// rnd = rho | r | mu (canonical); pi, ext (the sums of frstage_extrapolate: sigma_t = zt[t] ext[n + t]), zt, invfact and abc = L mu | R mu | O mu in
// Montgomery form.  n = 1: pi, ext, zt and invfact are not read (vectors 2, 3, 4 have no term).
static constexpr int KEYCHK_LAG_G1_VECS = 8, KEYCHK_LAG_G2_VECS = 4;
struct KeychkLagVecs {
    const uint32_t *rnd, *pi, *ext, *zt, *invfact, *abc, *mid_idx;
    uint32_t n, n_mid;
};
__global__ void k_keychk_lag_scalars(uint32_t* __restrict__ out1, uint32_t* __restrict__ out2, KeychkLagVecs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = a.n, l1 = 3, hl = l1 + n, lt = hl + (n - 1), p1 = lt + a.n_mid, p2 = 2 + n;
    if (i >= p1) return;          // p2 < p1
    const uint32_t* rho = a.rnd;
    const uint32_t* mu = rho + 8 * 2 * n;
    const Fr zero = fe_zero<FrParams>();
    Fr one = zero;
    one.v[0] = 1;
    Fr x[KEYCHK_LAG_G1_VECS];
#pragma unroll
    for (int q = 0; q < KEYCHK_LAG_G1_VECS; q++) x[q] = zero;
    if (i >= l1 && i < hl) {
        const uint64_t k = i - l1;
        x[0] = one;
        x[1] = fe_load<FrParams>(rho + 8 * k);
        if (n > 1) {
            const Fr pk = fe_load<FrParams>(a.pi + 8 * k);
            x[2] = fe_from_mont(pk);
            x[3] = fe_from_mont(fe_mul(pk, fe_from_u32<FrParams>((uint32_t)k)));
        }
        x[6] = fe_from_mont(fe_load<FrParams>(a.abc + 8 * k));
        x[7] = fe_from_mont(fe_load<FrParams>(a.abc + 8 * (2 * n + k)));
    } else if (i >= hl && i < lt) {
        const uint64_t t = i - hl;
        Fr w0 = fe_load<FrParams>(a.invfact + 8 * (n - 1));
        if ((n - 1) & 1) w0 = fe_neg(w0);
        x[4] = fe_from_mont(fe_mul(w0, fe_mul(fe_load<FrParams>(a.zt + 8 * t), fe_load<FrParams>(a.ext + 8 * (n + t)))));
    } else if (i >= lt) x[5] = fe_load<FrParams>(mu + 8 * (uint64_t)a.mid_idx[i - lt]);
#pragma unroll
    for (int q = 0; q < KEYCHK_LAG_G1_VECS; q++) fe_store<FrParams>(out1 + 8 * (q * p1 + i), x[q]);
    if (i < p2) {
        Fr y[KEYCHK_LAG_G2_VECS] = {zero, zero, zero, zero};
        if (i >= 2) {
            const uint64_t k = i - 2;
            y[0] = one;
            y[1] = fe_load<FrParams>(rho + 8 * k);
            y[2].v[0] = (uint32_t)k;
            y[3] = fe_from_mont(fe_load<FrParams>(a.abc + 8 * (n + k)));
        }
#pragma unroll
        for (int q = 0; q < KEYCHK_LAG_G2_VECS; q++) fe_store<FrParams>(out2 + 8 * (q * p2 + i), y[q]);
    }
}

int groth16_key_check_lagrange(Groth16Key& k, const uint8_t* vk_g1, size_t n_io, const uint8_t* vk_g2, const uint8_t* seed, uint32_t* failed) {
    const bool have_vk = vk_g1 && vk_g2;
    const uint32_t n = k.n, m = k.m, n_mid = k.n_mid;
    const uint64_t p1 = k.p1, p2 = k.p2;
    if (p1 != 2 + 2 * (uint64_t)n + n_mid || p2 != 2 + (uint64_t)n) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_key_check_lagrange: the handle's pools are not a | d1 | b1 | l1 | hl | ltd_mid and b2 | d2 | l2");
    DeviceScope ds(k.vdev);
    Ctx& c = ctx();
    hipStream_t s = c.stream;
    HIPCHK(hipGetLastError());
    const KeychkSeed sd = seed_take(seed);
    // which variable has its point where: mids in the key's ltd_mid (mid_idx), the others in the verification key's ltgm_io, both in variable order
    std::vector<uint32_t> mids(n_mid ? n_mid : 1), io_idx;
    if (n_mid) HIPCHK(hipMemcpy(mids.data(), k.mid_idx.p, 4 * (size_t)n_mid, hipMemcpyDeviceToHost));
    std::vector<uint8_t> is_mid(m, 0);
    for (uint32_t j = 0; j < n_mid; j++) is_mid[mids[j]] = 1;
    for (uint32_t v = 0; v < m; v++)
        if (!is_mid[v]) io_idx.push_back(v);
    // the verification key's points, decoded and checked like those of zk_groth16_vk_upload (endomorphism subgroup test, its codes): G2 list, then G1 list
    DevBuf vk1, vk2;
    if (have_vk) {
        std::vector<uint8_t> v1, v2;
        ZKCHK(points_decode_two_lists(vk_g1, 1 + n_io, vk_g2, 3, "key_check", SUBGROUP_ENDO, vk1, vk2, v1, v2, s));
        for (uint8_t v : v2)
            if (v) ZK_FAIL(verdict_code(v), "zk_groth16_key_check_lagrange: bad G2 point in the verification key (one2 | gm | d: encoding, curve or subgroup)");
        for (uint8_t v : v1)
            if (v) ZK_FAIL(verdict_code(v), "zk_groth16_key_check_lagrange: bad G1 point in the verification key (one1 | ltgm_io: encoding, curve or subgroup)");
    }
    const uint64_t nrnd = 2 * (uint64_t)n + m;          // rho | r | mu
    const size_t g1x = xyzz_bytes(CURVE_G1), g2x = xyzz_bytes(CURVE_G2);
    FrScratch fs;
    MsmWorkspace w1, w2;
    DevBuf rnd, pi, ext, kappa, partials, scal1, scal2, res1, res2, d_is_mid, d_io_idx;
    ZKCHK(frstage_scratch_alloc(k.fr, fs));
    ZKCHK(msm_workspace_alloc(w1, k.g1));
    ZKCHK(msm_workspace_alloc(w2, k.g2));
    ZKCHK(rnd.alloc(32 * nrnd));
    ZKCHK(pi.alloc(32 * (size_t)n));
    ZKCHK(ext.alloc(32 * (size_t)k.fr.S));
    ZKCHK(kappa.alloc(64));
    ZKCHK(partials.alloc(32 * (size_t)2 * LEAD_BLOCKS));
    ZKCHK(scal1.alloc(32 * KEYCHK_LAG_G1_VECS * p1));
    ZKCHK(scal2.alloc(32 * KEYCHK_LAG_G2_VECS * p2));
    ZKCHK(res1.alloc(g1x * (KEYCHK_LAG_G1_VECS + 1)));          // + the product over ltgm_io
    ZKCHK(res2.alloc(g2x * KEYCHK_LAG_G2_VECS));
    ZKCHK(d_is_mid.alloc(m));
    ZKCHK(d_io_idx.alloc(4 * (io_idx.size() ? io_idx.size() : 1)));
    HIPCHK(hipMemcpyAsync(d_is_mid.p, is_mid.data(), m, hipMemcpyHostToDevice, s));
    if (!io_idx.empty()) HIPCHK(hipMemcpyAsync(d_io_idx.p, io_idx.data(), 4 * io_idx.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(res1.p, 0, res1.bytes, s));          // zz = 0: the identity, for the sums that have no term
    HIPCHK(hipMemsetAsync(res2.p, 0, res2.bytes, s));
    uint32_t* raw = rnd.as<uint32_t>() + 8 * (uint64_t)n;
    uint32_t* mu = rnd.as<uint32_t>() + 8 * 2 * (uint64_t)n;
    {
        ScopedTimer t("key_check", s);
        hipLaunchKernelGGL(k_keychk_expand, g1d(nrnd), dim3(256), 0, s, rnd.as<uint32_t>(), nrnd, 2 * (uint64_t)n, (const uint8_t*)d_is_mid.as<uint8_t>(), have_vk ? 0 : 1, sd);
        if (n > 1) hipLaunchKernelGGL(k_keychk_lag_raw, g1d(2 * (uint64_t)n), dim3(256), 0, s, fs.abc.as<uint32_t>(), (const uint32_t*)raw, n);
        HIPCHK(hipGetLastError());
    }
    if (n > 1) {
        // pi: the projection of r on the hyperplane sum w_i pi_i = 0, then the sums sigma is made of
        ZKCHK(frstage_leading_coeffs(k.fr, fs, kappa.p, partials.p, s));
        ScopedTimer t("key_check", s);
        hipLaunchKernelGGL(k_keychk_lag_pi, g1d(n), dim3(256), 0, s, pi.as<uint32_t>(), (const uint32_t*)fs.abc.as<uint32_t>(), (const uint32_t*)kappa.as<uint32_t>(),
                           (const uint32_t*)k.fr.invfact.as<uint32_t>(), n);
        HIPCHK(hipGetLastError());
        ZKCHK(frstage_extrapolate(k.fr, fs, pi.p, ext.p, s));
    }
    // L mu, R mu, O mu in fs.abc (mu satisfies no gate: the flag and h are not read)
    ZKCHK(frstage_eval_lagrange(k.fr, fs, mu, s));
    {
        ScopedTimer t("key_check", s);
        KeychkLagVecs a{rnd.as<uint32_t>(), pi.as<uint32_t>(), ext.as<uint32_t>(), k.fr.zt.as<uint32_t>(), k.fr.invfact.as<uint32_t>(), fs.abc.as<uint32_t>(), k.mid_idx.as<uint32_t>(), n, n_mid};
        hipLaunchKernelGGL(k_keychk_lag_scalars, g1d(p1), dim3(256), 0, s, scal1.as<uint32_t>(), scal2.as<uint32_t>(), a);
        HIPCHK(hipGetLastError());
    }
    // which sums have a term at all (a product over all-zero scalars is skipped: its result stays the identity)
    const bool l_live = have_vk || n_mid > 0;
    const bool run1[KEYCHK_LAG_G1_VECS] = {true, true, n > 1, n > 1, n > 1, n_mid > 0, l_live, l_live};
    const bool run2[KEYCHK_LAG_G2_VECS] = {true, true, n > 1, l_live};
    for (int q = 0; q < KEYCHK_LAG_G1_VECS; q++)
        if (run1[q]) ZKCHK(msm_run(k.g1, w1, scal1.as<uint8_t>() + 32 * q * p1, res1.as<uint8_t>() + g1x * q, s));
    for (int q = 0; q < KEYCHK_LAG_G2_VECS; q++)
        if (run2[q]) ZKCHK(msm_run(k.g2, w2, scal2.as<uint8_t>() + 32 * q * p2, res2.as<uint8_t>() + g2x * q, s));
    // sum_k mu_k ltgm_io[k] over the verification key's own points: a base set that lives for this product
    MsmBases io;
    MsmWorkspace wio;
    DevBuf mu_io;
    if (have_vk && n_io) {
        ZKCHK(msm_bases_from_device_affine(io, CURVE_G1, vk1.as<uint8_t>() + 96, n_io, 0, false, s, true));
        ZKCHK(msm_workspace_alloc(wio, io));
        ZKCHK(mu_io.alloc(32 * n_io));
        {
            ScopedTimer t("key_check", s);
            hipLaunchKernelGGL(k_keychk_gather, g1d(n_io), dim3(256), 0, s, mu_io.as<uint32_t>(), (const uint32_t*)mu, (const uint32_t*)d_io_idx.as<uint32_t>(), (uint64_t)n_io);
            HIPCHK(hipGetLastError());
        }
        ZKCHK(msm_run(io, wio, mu_io.p, res1.as<uint8_t>() + g1x * KEYCHK_LAG_G1_VECS, s));
    }
    // the key's single points and the generators, as bytes: a | d1 | b1, b2 | d2 | l2[0], [1]_1, [1]_2
    DevBuf dn1, dn2, one;
    ZKCHK(dn1.alloc(96 * 4 * 2));
    ZKCHK(dn2.alloc(192 * 4 * 2));
    ZKCHK(one.alloc(32));
    const uint8_t one_le[32] = {1};
    HIPCHK(hipMemcpyAsync(one.p, one_le, 32, hipMemcpyHostToDevice, s));
    ZKCHK(msm_bases_dense(k.g1, 0, 3, dn1.p, s));
    ZKCHK(msm_bases_dense(k.g2, 0, 3, dn2.p, s));
    ZKCHK(fixed_base_mul(CURVE_G1, dn1.as<uint8_t>() + 96 * 3, one.p, 1, s));
    ZKCHK(fixed_base_mul(CURVE_G2, dn2.as<uint8_t>() + 192 * 3, one.p, 1, s));
    ZKCHK(points_affine_to_bytes(CURVE_G1, dn1.as<uint8_t>() + 96 * 4, dn1.p, 4, s));
    ZKCHK(points_affine_to_bytes(CURVE_G2, dn2.as<uint8_t>() + 192 * 4, dn2.p, 4, s));
    uint8_t kp1[4][96], kp2[4][192], s1[KEYCHK_LAG_G1_VECS + 1][96], s2[KEYCHK_LAG_G2_VECS][192];
    HIPCHK(hipMemcpyAsync(kp1, dn1.as<uint8_t>() + 96 * 4, sizeof kp1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(kp2, dn2.as<uint8_t>() + 192 * 4, sizeof kp2, hipMemcpyDeviceToHost, s));
    ZKCHK(points_xyzz_to_bytes(CURVE_G1, res1.p, KEYCHK_LAG_G1_VECS + 1, &s1[0][0], s));          // synchronises
    ZKCHK(points_xyzz_to_bytes(CURVE_G2, res2.p, KEYCHK_LAG_G2_VECS, &s2[0][0], s));
    const uint8_t *al = kp1[0], *d1 = kp1[1], *b1 = kp1[2], *gen1 = kp1[3];
    const uint8_t *b2 = kp2[0], *d2 = kp2[1], *l20 = kp2[2], *gen2 = kp2[3];
    const uint8_t *g1 = s1[0], *g2 = s2[0], *tau2 = s2[2], *S = s1[3];          // sum l1, sum l2, sum i l2[i], sum i pi_i l1[i]
    const uint8_t *gm = have_vk ? vk_g2 + 192 : nullptr, *vkd = have_vk ? vk_g2 + 384 : nullptr;

    // ---- the pairing products, two per relation: it holds iff they are equal.  TAU_G1 and H_BASES have no term at n = 1 and no product.
    std::vector<uint8_t> P, Q;
    std::vector<uint64_t> lens;
    std::vector<uint32_t> bit;          // of the relation that products 2j and 2j + 1 belong to
    auto product = [&](std::initializer_list<std::pair<const uint8_t*, const uint8_t*>> pairs) {
        for (const auto& pq : pairs) {
            P.insert(P.end(), pq.first, pq.first + 96);
            Q.insert(Q.end(), pq.second, pq.second + 192);
        }
        lens.push_back(pairs.size());
    };
    bit.push_back(ZK_KEYCHK_TAU_G2);        product({{s1[1], g2}});         product({{g1, s2[1]}});
    if (n > 1) {
        bit.push_back(ZK_KEYCHK_TAU_G1);    product({{S, g2}});             product({{s1[2], tau2}});
        bit.push_back(ZK_KEYCHK_H_BASES);   product({{s1[4], d2}});         product({{S, l20}});
    }
    bit.push_back(ZK_KEYCHK_BETA);          product({{b1, g2}});            product({{g1, b2}});
    bit.push_back(ZK_KEYCHK_DELTA);         product({{d1, g2}});            product({{g1, d2}});
    bit.push_back(ZK_KEYCHK_L);
    if (have_vk) product({{s1[5], d2}, {s1[8], gm}});
    else product({{s1[5], d2}});
    product({{s1[6], b2}, {al, s2[3]}, {s1[7], g2}});
    std::vector<uint8_t> gt;
    ZKCHK(keychk_pairing_products(P, Q, lens, gt, s));
    uint32_t f = 0;
    for (size_t j = 0; j < bit.size(); j++)
        if (memcmp(gt.data() + 576 * (2 * j), gt.data() + 576 * (2 * j + 1), 576) != 0) f |= bit[j];
    if (memcmp(g1, gen1, 96) || memcmp(g2, gen2, 192) || (have_vk && (memcmp(vk_g1, gen1, 96) || memcmp(vk_g2, gen2, 192)))) f |= ZK_KEYCHK_GENERATORS;
    if (is_identity_bytes(d1) || is_identity_bytes(d2) || (have_vk && memcmp(vkd, d2, 192))) f |= ZK_KEYCHK_DELTA;
    if (have_vk && is_identity_bytes(gm)) f |= ZK_KEYCHK_GAMMA;
    *failed = f;
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}

}  // namespace zk
