// Key generation on gfx950: Groth16 setup (src/groth16/groth16.ml:45-108) and Pinocchio KeyGen.generate (src/pinocchio/pinocchio.ml:77-189) in one
// call each, with every exponent computed on the device and every point taken from the fixed-base kernel where the exponents lie.
//
// A host that generates its own keys knows the trapdoor, so every key element is a known multiple of a generator:
//   1 lagrange   l_i(x), i < n, over the QAP's integer points first .. first+n-1 (QAP.ml:84,92) and Z(x) = prod (x - j), WITHOUT a division in x:
//                l_i(x) = (prod_{j<i} (x - j)) (prod_{j>i} (x - j)) w_i,   w_i = (-1)^(n-1-i) / (i! (n-1-i)!)
//                -- exact for every x in Fr, the points of the domain included (there one value is 1 and the others 0, as Poly.apply gives them).
//                Two multiplicative scans, a prefix and a suffix, in the plain three-phase shape: chunk products, a scan of the chunk totals in one
//                workgroup, the apply pass.  Three launches; no workgroup ever waits for another.
//   2 powers     x^i (times a constant): square-and-multiply to the start of a chunk, a serial run inside it
//   3 columns    u_k(x) = sum_g M[g][k] l_g(x) for M = L, R, O and every variable k (what `Poly.apply u_k x` computes per variable, groth16.ml:59-68,
//                pinocchio.ml:104-109): three sparse products with the TRANSPOSED matrices (the transposition is a counting pass on the host)
//   4 assemble   one kernel per protocol writes the whole exponent vector in key order (the layouts of include/zkmi355x.h)
//   5 points     fixed_base_mul on the exponent buffers; the key bytes are one encoding launch and one D2H copy per pool, the handle is built from the
//                very same affine points in device memory (no host round trip, no decoding, no subgroup test: groth16.hip / pinocchio.hip say why)
#include "ec.cuh"
#include "groth16_key.cuh"

#include <string.h>
#include <vector>

namespace zk {

int pin_key_from_device(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t* d_g1, const uint8_t* d_g2,
                        const uint8_t* d_hl, uint64_t* handle);          // pinocchio.hip

static inline dim3 g1d(uint64_t n, unsigned t = 256) { return dim3((unsigned)((n + t - 1) / t)); }

static constexpr uint32_t KCH = 32;          // elements one lane walks serially in the scans and the power runs
static constexpr uint32_t KSCAN_T = 256;     // lanes of the ONE workgroup that scans the chunk totals

// ------------------------------------------------------------------ 1 Lagrange basis at a point
// phase 1: tot[c] = prod_{j in chunk c} (x - first - j)
__global__ void k_lag_chunk_prod(uint32_t* __restrict__ tot, const uint32_t* __restrict__ x, uint32_t n, uint32_t first) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, lo = c * KCH;
    if (lo >= n) return;
    const uint64_t hi = lo + KCH < n ? lo + KCH : n;
    const Fr one = fe_one<FrParams>();
    Fr d = fe_sub(fe_load<FrParams>(x), fe_from_u32<FrParams>(first + (uint32_t)lo)), acc = one;
    for (uint64_t i = lo; i < hi; i++) {
        acc = fe_mul(acc, d);
        d = fe_sub(d, one);
    }
    fe_store<FrParams>(tot + 8 * c, acc);
}
// phase 2, one workgroup: pre[c] = prod_{c' < c} tot[c'], suf[c] = prod_{c' > c} tot[c'], *z (unless null) = the product of all of them = Z(x).
// Every lane folds a contiguous segment of the totals, the 256 segment products are scanned in LDS (both directions), every lane walks its segment again.
__global__ __launch_bounds__(KSCAN_T) void k_lag_scan_totals(uint32_t* __restrict__ pre, uint32_t* __restrict__ suf, uint32_t* __restrict__ z,
                                                             const uint32_t* __restrict__ tot, uint32_t nch) {
    __shared__ uint4 lp[2 * KSCAN_T], ls[2 * KSCAN_T];          // one Fr = two uint4
    const uint32_t t = threadIdx.x, seg = (nch + KSCAN_T - 1) / KSCAN_T;
    const uint32_t lo = t * seg < nch ? t * seg : nch, hi = lo + seg < nch ? lo + seg : nch;
    const Fr one = fe_one<FrParams>();
    Fr acc = one;
    for (uint32_t c = lo; c < hi; c++) acc = fe_mul(acc, fe_load<FrParams>(tot + 8 * (uint64_t)c));
    fe_store<FrParams>(lp + 2 * t, acc);
    fe_store<FrParams>(ls + 2 * t, acc);
    __syncthreads();
    for (uint32_t off = 1; off < KSCAN_T; off <<= 1) {          // inclusive scans: lp forward, ls backward
        Fr a = fe_load<FrParams>(lp + 2 * t), b = fe_load<FrParams>(ls + 2 * t);
        if (t >= off) a = fe_mul(fe_load<FrParams>(lp + 2 * (t - off)), a);
        if (t + off < KSCAN_T) b = fe_mul(b, fe_load<FrParams>(ls + 2 * (t + off)));
        __syncthreads();
        fe_store<FrParams>(lp + 2 * t, a);
        fe_store<FrParams>(ls + 2 * t, b);
        __syncthreads();
    }
    Fr run = t ? fe_load<FrParams>(lp + 2 * (t - 1)) : one;
    for (uint32_t c = lo; c < hi; c++) {
        fe_store<FrParams>(pre + 8 * (uint64_t)c, run);
        run = fe_mul(run, fe_load<FrParams>(tot + 8 * (uint64_t)c));
    }
    if (z && t == KSCAN_T - 1) fe_store<FrParams>(z, fe_load<FrParams>(lp + 2 * t));
    Fr back = t + 1 < KSCAN_T ? fe_load<FrParams>(ls + 2 * (t + 1)) : one;
    for (uint32_t c = hi; c-- > lo;) {
        fe_store<FrParams>(suf + 8 * (uint64_t)c, back);
        back = fe_mul(back, fe_load<FrParams>(tot + 8 * (uint64_t)c));
    }
}
// phase 3: out[i] = prefix_i * w_i on the way up the chunk, times suffix_i on the way down
__global__ void k_lag_apply(uint32_t* out, const uint32_t* __restrict__ x, const uint32_t* __restrict__ pre, const uint32_t* __restrict__ suf,
                            const uint32_t* __restrict__ invfact, uint32_t n, uint32_t first) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, lo = c * KCH;
    if (lo >= n) return;
    const uint64_t hi = lo + KCH < n ? lo + KCH : n;
    const Fr one = fe_one<FrParams>();
    Fr d = fe_sub(fe_load<FrParams>(x), fe_from_u32<FrParams>(first + (uint32_t)lo)), run = fe_load<FrParams>(pre + 8 * c);
    for (uint64_t i = lo; i < hi; i++) {
        Fr w = fe_mul(fe_load<FrParams>(invfact + 8 * i), fe_load<FrParams>(invfact + 8 * (n - 1 - i)));
        if ((n - 1 - i) & 1) w = fe_neg(w);
        fe_store<FrParams>(out + 8 * i, fe_mul(run, w));
        run = fe_mul(run, d);
        d = fe_sub(d, one);
    }
    Fr back = fe_load<FrParams>(suf + 8 * c);
    for (uint64_t i = hi; i-- > lo;) {
        d = fe_add(d, one);                                              // x - first - i
        fe_store<FrParams>(out + 8 * i, fe_mul(fe_load<FrParams>(out + 8 * i), back));
        back = fe_mul(back, d);
    }
}
// d_out: n values l_i(x), d_z: Z(x) (all Montgomery, device); d_x: x in Montgomery form; d_invfact: 1/i!, i < n.  `scratch` must outlive the launches.
static int lagrange_at_dev(void* d_out, void* d_z, uint32_t n, uint32_t first, const void* d_x, const void* d_invfact, DevBuf& scratch, hipStream_t s) {
    const uint32_t nch = (n + KCH - 1) / KCH;
    ZKCHK(scratch.alloc(32 * 3 * (size_t)nch));
    uint32_t *tot = scratch.as<uint32_t>(), *pre = tot + 8 * (size_t)nch, *suf = pre + 8 * (size_t)nch;
    ScopedTimer t("keygen_lagrange", s);
    hipLaunchKernelGGL(k_lag_chunk_prod, g1d(nch, 64), dim3(64), 0, s, tot, (const uint32_t*)d_x, n, first);
    hipLaunchKernelGGL(k_lag_scan_totals, dim3(1), dim3(KSCAN_T), 0, s, pre, suf, (uint32_t*)d_z, (const uint32_t*)tot, nch);
    hipLaunchKernelGGL(k_lag_apply, g1d(nch, 64), dim3(64), 0, s, (uint32_t*)d_out, (const uint32_t*)d_x, (const uint32_t*)pre, (const uint32_t*)suf,
                       (const uint32_t*)d_invfact, n, first);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

// ------------------------------------------------------------------ 2 power sequence: out[i] = scale * x^i, i < cnt (scale == nullptr: 1)
__global__ void k_power_run(uint32_t* __restrict__ out, const uint32_t* __restrict__ x, const uint32_t* __restrict__ scale, uint64_t cnt) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, lo = c * KCH;
    if (lo >= cnt) return;
    const uint64_t hi = lo + KCH < cnt ? lo + KCH : cnt;
    const Fr xs = fe_load<FrParams>(x);
    Fr acc = scale ? fe_load<FrParams>(scale) : fe_one<FrParams>(), base = xs;
    for (uint64_t e = lo; e; e >>= 1) {
        if (e & 1) acc = fe_mul(acc, base);
        base = fe_sqr(base);
    }
    for (uint64_t i = lo; i < hi; i++) {
        fe_store<FrParams>(out + 8 * i, acc);
        acc = fe_mul(acc, xs);
    }
}
int power_run(void* d_out, const void* d_x, const void* d_scale, uint64_t cnt, hipStream_t s, const char* family) {
    if (!cnt) return ZK_OK;
    ScopedTimer t(family, s);
    hipLaunchKernelGGL(k_power_run, g1d((cnt + KCH - 1) / KCH, 64), dim3(64), 0, s, (uint32_t*)d_out, (const uint32_t*)d_x, (const uint32_t*)d_scale, cnt);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

// ------------------------------------------------------------------ 3 columns: u_k(x) through the transposed matrices
// M (n rows, m columns) -> its transpose as CSR over m rows; validates M as the uploads do (the counting pass indexes by its columns)
int transpose_csr(const zk_csr* M, uint32_t n, uint32_t m, std::vector<uint32_t>& ptr, std::vector<uint32_t>& col, std::vector<uint8_t>& val) {
    if (!M->row_ptr) ZK_FAIL(ZK_ERR_ARG, "R1CS matrix: null row_ptr");
    for (uint32_t g = 0; g < n; g++)
        if (M->row_ptr[g] > M->row_ptr[g + 1]) ZK_FAIL(ZK_ERR_ARG, "R1CS matrix: row_ptr not monotone");
    const uint64_t e0 = M->row_ptr[0], e1 = M->row_ptr[n];
    if (e1 > e0 && (!M->col || !M->val)) ZK_FAIL(ZK_ERR_ARG, "R1CS matrix: null col/val");
    ptr.assign((size_t)m + 1, 0);
    for (uint64_t e = e0; e < e1; e++) {
        if (M->col[e] >= m) ZK_FAIL(ZK_ERR_ARG, "R1CS matrix: column index out of range");
        ptr[M->col[e] + 1]++;
    }
    for (uint32_t k = 0; k < m; k++) ptr[k + 1] += ptr[k];
    std::vector<uint32_t> cur(ptr.begin(), ptr.end() - 1);
    col.resize(e1 - e0 ? e1 - e0 : 1);
    val.resize(32 * (e1 - e0 ? e1 - e0 : 1));
    for (uint32_t g = 0; g < n; g++)
        for (uint64_t e = M->row_ptr[g]; e < M->row_ptr[g + 1]; e++) {
            const uint32_t pos = cur[M->col[e]]++;
            col[pos] = g;
            memcpy(val.data() + 32 * (size_t)pos, M->val + 32 * e, 32);
        }
    return ZK_OK;
}
// d_uks: v_k(x) | w_k(x) | y_k(x), m each (Montgomery), from d_lag = the n values l_g(x)
static int columns_at_dev(void* d_uks, uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const void* d_lag, hipStream_t s) {
    const zk_csr* Ms[3] = {L, R, O};
    std::vector<uint32_t> ptr, col;
    std::vector<uint8_t> val;
    for (int q = 0; q < 3; q++) {
        ZKCHK(transpose_csr(Ms[q], n, m, ptr, col, val));
        const zk_csr T = {ptr.data(), col.data(), val.data()};
        CsrDev d;
        ZKCHK(frstage_upload_csr(d, &T, m, n, s));          // ZK_ERR_SCALAR_RANGE for a coefficient >= r
        ScopedTimer t("keygen_columns", s);
        ZKCHK(frstage_spmv(d, m, d_lag, (uint8_t*)d_uks + 32 * (size_t)m * q, s));
        HIPCHK(hipStreamSynchronize(s));                    // the host vectors and `d` are reused / released
    }
    return ZK_OK;
}

// ------------------------------------------------------------------ trapdoor scalars
// k[0 .. cnt) = the trapdoor in Montgomery form, then the derived constants: Groth16 (cnt = 5: alpha beta gamma delta tau) -> 1/delta | 1/gamma -- the
// two inversions of a whole setup; Pinocchio (cnt = 8: rv rw s av aw ay b gm) -> ry = rv rw (pinocchio.ml:93)
__global__ void k_keygen_consts(uint32_t* __restrict__ k, const uint32_t* __restrict__ toxic, uint32_t cnt) {
    if (blockIdx.x || threadIdx.x) return;
    for (uint32_t i = 0; i < cnt; i++) fe_store<FrParams>(k + 8 * i, fe_to_mont(fe_load<FrParams>(toxic + 8 * i)));
    if (cnt == 5) {
        fe_store<FrParams>(k + 8 * 5, fe_inv(fe_load<FrParams>(k + 8 * 3)));
        fe_store<FrParams>(k + 8 * 6, fe_inv(fe_load<FrParams>(k + 8 * 2)));
    } else {
        fe_store<FrParams>(k + 8 * 8, fe_mul(fe_load<FrParams>(k), fe_load<FrParams>(k + 8)));
    }
}
__global__ void k_fr_mul1(uint32_t* out, const uint32_t* a, const uint32_t* b) {
    if (blockIdx.x || threadIdx.x) return;
    fe_store<FrParams>(out, fe_mul(fe_load<FrParams>(a), fe_load<FrParams>(b)));
}
__global__ void k_fr_to_mont1(uint32_t* out, const uint32_t* a) {
    if (blockIdx.x || threadIdx.x) return;
    fe_store<FrParams>(out, fe_to_mont(fe_load<FrParams>(a)));
}

// ------------------------------------------------------------------ 4a Groth16: the exponent vectors in key order (oracle/zk_oracle.c: orc_groth16_setup_exponents)
//   e1 = a | d | b | [tau^i (n+2) | tau^i Z/delta (n-1)] | L_k/delta (mids) | 1 | L_k/gamma (io) | [l_i (n) | lambda_t Z/delta (n-1)]
//   e2 = b | d | [tau^i (n+2)] | 1 | gamma | delta | [l_i (n)]
// The first bracket is the key in the reference's format (has_pow), the last the Lagrange-form pools (has_lag); in between the verification key.
struct G16Asm {
    uint32_t *e1, *e2;
    const uint32_t *k;                 // alpha beta gamma delta tau 1/delta 1/gamma | Z/delta
    const uint32_t *pw;                // tau^i (n+2) | tau^i Z/delta (n-1)
    const uint32_t *lag, *lam;         // l_i(tau), lambda_t(tau)
    const uint32_t *uks;               // v_k | w_k | y_k
    const uint32_t *mid_idx, *io_idx;
    uint32_t n, m, n_mid, n_io, has_pow, has_lag;
};
static inline uint64_t g16_npow(uint32_t n, bool has_pow) { return has_pow ? (uint64_t)n + 2 : 0; }
__global__ void k_groth16_assemble(G16Asm p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t np = p.has_pow ? (uint64_t)p.n + 2 : 0, nz = p.has_pow ? (uint64_t)p.n - 1 : 0, nl = p.has_lag ? (uint64_t)p.n : 0, nh = p.has_lag ? (uint64_t)p.n - 1 : 0;
    const uint64_t o_z = 3 + np, o_mid = o_z + nz, o_vk = o_mid + p.n_mid, o_lag = o_vk + 1 + p.n_io, o_lam = o_lag + nl, total1 = o_lam + nh;
    const uint64_t q_vk = 2 + np, q_lag = q_vk + 3, total2 = q_lag + nl;
    auto K = [&](int j) { return fe_load<FrParams>(p.k + 8 * j); };
    auto Lk = [&](uint32_t k) {          // L_k(tau) = beta v_k + alpha w_k + y_k, groth16.ml:59-68
        const Fr v = fe_load<FrParams>(p.uks + 8 * (uint64_t)k), w = fe_load<FrParams>(p.uks + 8 * ((uint64_t)p.m + k)), y = fe_load<FrParams>(p.uks + 8 * (2 * (uint64_t)p.m + k));
        return fe_add(fe_add(fe_mul(K(1), v), fe_mul(K(0), w)), y);
    };
    if (i < total1) {
        Fr x;
        if (i == 0) x = K(0);
        else if (i == 1) x = K(3);
        else if (i == 2) x = K(1);
        else if (i < o_mid) x = fe_load<FrParams>(p.pw + 8 * (i - 3));
        else if (i < o_vk) x = fe_mul(Lk(p.mid_idx[i - o_mid]), K(5));
        else if (i == o_vk) x = fe_one<FrParams>();
        else if (i < o_lag) x = fe_mul(Lk(p.io_idx[i - o_vk - 1]), K(6));
        else if (i < o_lam) x = fe_load<FrParams>(p.lag + 8 * (i - o_lag));
        else x = fe_mul(fe_load<FrParams>(p.lam + 8 * (i - o_lam)), K(7));
        fe_store<FrParams>(p.e1 + 8 * i, fe_from_mont(x));
    }
    if (i < total2) {
        Fr x;
        if (i == 0) x = K(1);
        else if (i == 1) x = K(3);
        else if (i < q_vk) x = fe_load<FrParams>(p.pw + 8 * (i - 2));
        else if (i == q_vk) x = fe_one<FrParams>();
        else if (i == q_vk + 1) x = K(2);
        else if (i == q_vk + 2) x = K(3);
        else x = fe_load<FrParams>(p.lag + 8 * (i - q_lag));
        fe_store<FrParams>(p.e2 + 8 * i, fe_from_mont(x));
    }
}

// ------------------------------------------------------------------ 4b Pinocchio: the exponent vectors in key order (orc_pinocchio_keygen_exponents)
//   e1 = vv | yy | vav | yay | bvwy (n_mid each) | si (n+1) | v_all (m) | w_all (m) | vt yt vavt yayt vbt wbt ybt || one aw bgm | vv_io | yy_io || [lambda_t(s) (n-1) | Z(s)]
//   e2 = ww | waw (n_mid each) | si2 (n+1) | wt wawt || one2 av ay gm2 bgm2 yt | ww_io
struct PinAsm {
    uint32_t *e1, *e2;
    const uint32_t *k;                 // rv rw s av aw ay b gm ry | t = Z(s)
    const uint32_t *pw;                // s^i, i <= n
    const uint32_t *lam;               // lambda_t(s), t < n - 1
    const uint32_t *uks, *mid_idx, *io_idx;
    uint32_t n, m, n_mid, n_io, has_lag;
};
__global__ void k_pinocchio_assemble(PinAsm p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nm = p.n_mid, n1 = (uint64_t)p.n + 1, m = p.m, ni = p.n_io;
    const uint64_t o_si = 5 * nm, o_v = o_si + n1, o_w = o_v + m, o_one = o_w + m, o_vk = o_one + 7, o_hl = o_vk + 3 + 2 * ni, total1 = o_hl + (p.has_lag ? p.n : 0);
    const uint64_t q_si = 2 * nm, q_one = q_si + n1, q_vk = q_one + 2, total2 = q_vk + 6 + ni;
    enum { RV, RW, S, AV, AW, AY, B, GM, RY, T };
    auto K = [&](int j) { return fe_load<FrParams>(p.k + 8 * j); };
    auto V = [&](uint64_t k) { return fe_load<FrParams>(p.uks + 8 * k); };
    auto W = [&](uint64_t k) { return fe_load<FrParams>(p.uks + 8 * (m + k)); };
    auto Y = [&](uint64_t k) { return fe_load<FrParams>(p.uks + 8 * (2 * m + k)); };
    const Fr one = fe_one<FrParams>();
    if (i < total1) {
        Fr x;
        if (i < o_si) {
            const uint64_t q = i / nm, k = p.mid_idx[i % nm];
            const Fr rvv = fe_mul(K(RV), V(k)), ryy = fe_mul(K(RY), Y(k));
            if (q == 0) x = rvv;                                                                  // vv   :113
            else if (q == 1) x = ryy;                                                             // yy   :118
            else if (q == 2) x = fe_mul(rvv, K(AV));                                              // vav  :126
            else if (q == 3) x = fe_mul(ryy, K(AY));                                              // yay  :130
            else x = fe_mul(fe_add(fe_add(rvv, fe_mul(K(RW), W(k))), ryy), K(B));                 // bvwy :137-140
        } else if (i < o_v) x = fe_load<FrParams>(p.pw + 8 * (i - o_si));                         // si   :133
        else if (i < o_w) x = V(i - o_v);                                                         // v_all :153
        else if (i < o_one) x = W(i - o_w);                                                       // w_all :156
        else if (i < o_vk) {
            const uint64_t j = i - o_one;
            const Fr vt = fe_mul(K(RV), K(T)), wt = fe_mul(K(RW), K(T)), yt = fe_mul(K(RY), K(T));
            x = j == 0 ? vt : j == 1 ? yt : j == 2 ? fe_mul(vt, K(AV)) : j == 3 ? fe_mul(yt, K(AY)) : j == 4 ? fe_mul(vt, K(B)) : j == 5 ? fe_mul(wt, K(B)) : fe_mul(yt, K(B));
        } else if (i < o_hl) {
            const uint64_t j = i - o_vk;
            if (j == 0) x = one;
            else if (j == 1) x = K(AW);
            else if (j == 2) x = fe_mul(K(GM), K(B));
            else if (j < 3 + ni) x = fe_mul(K(RV), V(p.io_idx[j - 3]));                           // vv_io :172
            else x = fe_mul(K(RY), Y(p.io_idx[j - 3 - ni]));                                      // yy_io :174
        } else {
            const uint64_t j = i - o_hl;
            x = j + 1 < p.n ? fe_load<FrParams>(p.lam + 8 * j) : K(T);
        }
        fe_store<FrParams>(p.e1 + 8 * i, fe_from_mont(x));
    }
    if (i < total2) {
        Fr x;
        if (i < q_si) {
            const uint64_t q = i / nm, k = p.mid_idx[i % nm];
            x = fe_mul(K(RW), W(k));                                                              // ww   :116
            if (q == 1) x = fe_mul(x, K(AW));                                                     // waw  :128
        } else if (i < q_one) x = fe_load<FrParams>(p.pw + 8 * (i - q_si));                       // si2  :134
        else if (i < q_vk) {
            x = fe_mul(K(RW), K(T));                                                              // wt   :143
            if (i - q_one == 1) x = fe_mul(x, K(AW));                                             // wawt :146
        } else {
            const uint64_t j = i - q_vk;
            x = j == 0 ? one : j == 1 ? K(AV) : j == 2 ? K(AY) : j == 3 ? K(GM) : j == 4 ? fe_mul(K(GM), K(B)) : j == 5 ? fe_mul(K(RY), K(T)) : fe_mul(K(RW), W(p.io_idx[j - 6]));
        }
        fe_store<FrParams>(p.e2 + 8 * i, fe_from_mont(x));
    }
}

// ------------------------------------------------------------------ host side
static const uint64_t FR_MOD64[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
static bool fr_canonical(const uint8_t* b) {          // 32 B little-endian < r
    for (int i = 3; i >= 0; i--) {
        uint64_t w;
        memcpy(&w, b + 8 * i, 8);          // the library runs on little-endian hosts only (every Fr buffer is copied to the device as it is)
        if (w != FR_MOD64[i]) return w < FR_MOD64[i];
    }
    return false;
}
static bool fr_is_zero(const uint8_t* b) {
    uint8_t o = 0;
    for (int i = 0; i < 32; i++) o |= b[i];
    return o == 0;
}
// the argument checks both keygen entries share, in the order the header promises: null / form, sizes, point counts, the trapdoor -- all before the device
static int keygen_precheck(const char* who, uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t* toxic,
                           uint32_t form, std::vector<uint32_t>& mids, std::vector<uint32_t>& ios) {
    if (!L || !R || !O || !mid || !toxic) return set_error(ZK_ERR_ARG, who, __FILE__, __LINE__);
    if (form != ZK_KEY_FORM_TAU_POWERS && form != ZK_KEY_FORM_LAGRANGE) ZK_FAIL(ZK_ERR_ARG, "keygen: form must be ZK_KEY_FORM_TAU_POWERS or ZK_KEY_FORM_LAGRANGE");
    if (n < 1 || n > (1u << 24) || m == 0) ZK_FAIL(ZK_ERR_ARG, "keygen: constraint count must be in [1, 2^24] and there must be a variable");
    for (uint32_t k = 0; k < m; k++) (mid[k] ? mids : ios).push_back(k);
    return ZK_OK;
}
static int toxic_check(const uint8_t* toxic, uint32_t ntoxic) {
    for (uint32_t i = 0; i < ntoxic; i++)
        if (!fr_canonical(toxic + 32 * i)) ZK_FAIL(ZK_ERR_SCALAR_RANGE, "keygen: a trapdoor scalar is >= r");
    return ZK_OK;
}
// points [lo, lo + cnt) of a dense affine buffer, encoded, to host memory (enqueue only; `bytes` must outlive the stream's work)
static int emit_points(Curve cv, uint8_t* host_out, const DevBuf& aff, uint64_t lo, uint64_t cnt, DevBuf& bytes, hipStream_t s) {
    if (!host_out || !cnt) return ZK_OK;
    const size_t pb = aff_bytes(cv);
    ZKCHK(bytes.alloc(pb * cnt));
    ZKCHK(points_affine_to_bytes(cv, bytes.p, aff.as<uint8_t>() + pb * lo, cnt, s));
    HIPCHK(hipMemcpyAsync(host_out, bytes.p, pb * cnt, hipMemcpyDeviceToHost, s));
    return ZK_OK;
}
static int upload_indices(DevBuf& d, const std::vector<uint32_t>& v, hipStream_t s) {
    ZKCHK(d.alloc(4 * (v.size() ? v.size() : 1)));
    if (!v.empty()) HIPCHK(hipMemcpyAsync(d.p, v.data(), 4 * v.size(), hipMemcpyHostToDevice, s));
    return ZK_OK;
}

}  // namespace zk

using namespace zk;
extern "C" {

int zk_fr_lagrange_at(uint32_t n, uint32_t first, const uint8_t x[32], uint8_t* out, uint8_t z_out[32]) {
    if (!x || !out || n == 0) ZK_FAIL(ZK_ERR_ARG, "zk_fr_lagrange_at: null argument or an empty domain");
    if (n > (1u << 24) || (uint64_t)first + n > ((uint64_t)1 << 32)) ZK_FAIL(ZK_ERR_ARG, "zk_fr_lagrange_at: at most 2^24 points, all below 2^32");
    if (!fr_canonical(x)) ZK_FAIL(ZK_ERR_SCALAR_RANGE, "zk_fr_lagrange_at: x >= r");
    ZKCHK(ensure_init());
    Ctx& c = ctx();
    DevBuf dx, dz, dout, invf, scratch;
    ZKCHK(dx.alloc(32));
    ZKCHK(dz.alloc(32));
    ZKCHK(dout.alloc(32 * (size_t)n));
    ZKCHK(invf.alloc(32 * (size_t)n));
    HIPCHK(hipMemcpyAsync(dx.p, x, 32, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(k_fr_to_mont1, dim3(1), dim3(64), 0, c.stream, dx.as<uint32_t>(), (const uint32_t*)dx.as<uint32_t>());
    ZKCHK(frstage_invfact(invf.p, n, c.stream));
    ZKCHK(lagrange_at_dev(dout.p, dz.p, n, first, dx.p, invf.p, scratch, c.stream));
    ZKCHK(fr_from_mont(dout.p, dout.p, n, c.stream));
    ZKCHK(fr_from_mont(dz.p, dz.p, 1, c.stream));
    HIPCHK(hipMemcpyAsync(out, dout.p, 32 * (size_t)n, hipMemcpyDeviceToHost, c.stream));
    if (z_out) HIPCHK(hipMemcpyAsync(z_out, dz.p, 32, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    return ZK_OK;
}

int zk_groth16_keygen(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t toxic[160], uint32_t form,
                      uint8_t* pk_g1, size_t pk_g1_points, uint8_t* pk_g2, size_t pk_g2_points, uint8_t* vk_g1, uint8_t* vk_g2, uint64_t* handle) {
    std::vector<uint32_t> mids, ios;
    ZKCHK(keygen_precheck("zk_groth16_keygen: null argument", n, m, L, R, O, mid, toxic, form, mids, ios));
    const uint32_t n_mid = (uint32_t)mids.size(), n_io = (uint32_t)ios.size();
    const uint64_t key1 = 3 + ((uint64_t)n + 2) + (n - 1) + n_mid, key2 = 2 + ((uint64_t)n + 2);
    if (pk_g1 && pk_g1_points != key1) ZK_FAIL(ZK_ERR_DOMAIN, "zk_groth16_keygen: G1 key length != 3 + (n+2) + (n-1) + |mids|");
    if (pk_g2 && pk_g2_points != key2) ZK_FAIL(ZK_ERR_DOMAIN, "zk_groth16_keygen: G2 key length != 2 + (n+2)");
    ZKCHK(toxic_check(toxic, 5));
    // groth16.ml:70-90 divides by delta and by gamma (Fr.( / ) raises on zero)
    if (fr_is_zero(toxic + 64) || fr_is_zero(toxic + 96)) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_keygen: gamma = 0 or delta = 0 (the reference divides by them)");
    ZKCHK(ensure_init());
    if (handle && ctx_count() > 1) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_keygen: a handle needs a device list of one entry (the key bytes can be had on any list)");
    Ctx& c = ctx();
    hipStream_t s = c.stream;
    const bool want_tau_handle = handle && form == ZK_KEY_FORM_TAU_POWERS;
    const bool has_lag = handle && form == ZK_KEY_FORM_LAGRANGE, has_pow = pk_g1 || pk_g2 || want_tau_handle;
    // ---- Fr: trapdoor, Lagrange values, powers, columns
    DevBuf tox, k, invf, lag, lam, pw, uks, d_mid, d_io, scr1, scr2;
    ZKCHK(tox.alloc(160));
    ZKCHK(k.alloc(32 * 8));
    ZKCHK(invf.alloc(32 * (size_t)n));
    ZKCHK(lag.alloc(32 * (size_t)n));
    ZKCHK(lam.alloc(32 * (size_t)n));
    ZKCHK(pw.alloc(32 * (2 * (size_t)n + 1)));
    ZKCHK(uks.alloc(32 * 3 * (size_t)m));
    HIPCHK(hipMemcpyAsync(tox.p, toxic, 160, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_keygen_consts, dim3(1), dim3(64), 0, s, k.as<uint32_t>(), (const uint32_t*)tox.as<uint32_t>(), 5u);
    uint32_t* K = k.as<uint32_t>();
    const uint32_t *tau = K + 8 * 4, *dinv = K + 8 * 5;
    uint32_t* ztd = K + 8 * 7;
    ZKCHK(frstage_invfact(invf.p, n, s));
    ZKCHK(lagrange_at_dev(lag.p, ztd, n, 0, tau, invf.p, scr1, s));                            // ztd = Z(tau) for now
    hipLaunchKernelGGL(k_fr_mul1, dim3(1), dim3(64), 0, s, ztd, (const uint32_t*)ztd, dinv);   // Z(tau) / delta
    if (has_pow) {
        ZKCHK(power_run(pw.p, tau, nullptr, (uint64_t)n + 2, s));
        ZKCHK(power_run(pw.as<uint32_t>() + 8 * ((size_t)n + 2), tau, ztd, (uint64_t)n - 1, s));
    }
    if (has_lag && n > 1) ZKCHK(lagrange_at_dev(lam.p, nullptr, n - 1, n, tau, invf.p, scr2, s));   // lambda_t: the basis of the points n .. 2n-2
    ZKCHK(columns_at_dev(uks.p, n, m, L, R, O, lag.p, s));
    ZKCHK(upload_indices(d_mid, mids, s));
    ZKCHK(upload_indices(d_io, ios, s));
    // ---- exponents in key order
    const uint64_t np = g16_npow(n, has_pow), nz = has_pow ? (uint64_t)n - 1 : 0, nl = has_lag ? n : 0, nh = has_lag ? (uint64_t)n - 1 : 0;
    const uint64_t o_mid = 3 + np + nz, o_vk = o_mid + n_mid, o_lag = o_vk + 1 + n_io, total1 = o_lag + nl + nh;
    const uint64_t q_vk = 2 + np, q_lag = q_vk + 3, total2 = q_lag + nl;
    DevBuf e1, e2, a1, a2;
    ZKCHK(e1.alloc(32 * total1));
    ZKCHK(e2.alloc(32 * total2));
    ZKCHK(a1.alloc(96 * total1));
    ZKCHK(a2.alloc(192 * total2));
    {
        G16Asm p = {e1.as<uint32_t>(), e2.as<uint32_t>(), K, pw.as<uint32_t>(), lag.as<uint32_t>(), lam.as<uint32_t>(), uks.as<uint32_t>(),
                    d_mid.as<uint32_t>(), d_io.as<uint32_t>(), n, m, n_mid, n_io, has_pow ? 1u : 0u, has_lag ? 1u : 0u};
        ScopedTimer t("keygen_assemble", s);
        hipLaunchKernelGGL(k_groth16_assemble, g1d(total1), dim3(256), 0, s, p);
        HIPCHK(hipGetLastError());
    }
    // ---- points: ONE pass over the exponents serves the key bytes, the verification key and the handle
    ZKCHK(fixed_base_mul(CURVE_G1, a1.p, e1.p, total1, s));
    ZKCHK(fixed_base_mul(CURVE_G2, a2.p, e2.p, total2, s));
    DevBuf b1, b2, b3, b4;
    if (has_pow) {
        ZKCHK(emit_points(CURVE_G1, pk_g1, a1, 0, key1, b1, s));
        ZKCHK(emit_points(CURVE_G2, pk_g2, a2, 0, key2, b2, s));
    }
    ZKCHK(emit_points(CURVE_G1, vk_g1, a1, o_vk, 1 + (uint64_t)n_io, b3, s));
    ZKCHK(emit_points(CURVE_G2, vk_g2, a2, q_vk, 3, b4, s));
    // the caller's buffers are complete BEFORE a handle exists: a failure below returns with nothing in flight into them, and a handle is never
    // registered ahead of an error (the key builders end synchronised themselves)
    HIPCHK(hipStreamSynchronize(s));
    if (handle) {
        if (!has_lag) {
            ZKCHK(groth16_key_from_device(n, m, L, R, O, mid, a1.p, key1, a2.p, key2, false, handle));          // the key's prefix of a1 / a2 IS the pool
        } else {
            // a | d1 | b1 | [l_i] (n) | [lambda_t Z/delta] (n-1) | ltd_mid      b2 | d2 | [l_i] (n)
            const uint64_t p1 = 3 + (uint64_t)n + (n - 1) + n_mid, p2 = 2 + (uint64_t)n;
            DevBuf g1, g2;
            ZKCHK(g1.alloc(96 * p1));
            ZKCHK(g2.alloc(192 * p2));
            HIPCHK(hipMemcpyAsync(g1.p, a1.p, 96 * 3, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(g1.as<uint8_t>() + 96 * 3, a1.as<uint8_t>() + 96 * o_lag, 96 * (nl + nh), hipMemcpyDeviceToDevice, s));
            if (n_mid) HIPCHK(hipMemcpyAsync(g1.as<uint8_t>() + 96 * (3 + nl + nh), a1.as<uint8_t>() + 96 * o_mid, 96 * (uint64_t)n_mid, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(g2.p, a2.p, 192 * 2, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(g2.as<uint8_t>() + 192 * 2, a2.as<uint8_t>() + 192 * q_lag, 192 * nl, hipMemcpyDeviceToDevice, s));
            ZKCHK(groth16_key_from_device(n, m, L, R, O, mid, g1.p, p1, g2.p, p2, true, handle));
        }
    }
    return ZK_OK;
}

int zk_pinocchio_keygen(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t toxic[256], uint32_t form,
                        uint8_t* pk_g1, size_t pk_g1_points, uint8_t* pk_g2, size_t pk_g2_points, uint8_t* vk_g1, uint8_t* vk_g2, uint64_t* handle) {
    std::vector<uint32_t> mids, ios;
    ZKCHK(keygen_precheck("zk_pinocchio_keygen: null argument", n, m, L, R, O, mid, toxic, form, mids, ios));
    const uint32_t n_mid = (uint32_t)mids.size(), n_io = (uint32_t)ios.size();
    const uint64_t key1 = 5 * (uint64_t)n_mid + ((uint64_t)n + 1) + 2 * (uint64_t)m + 7, key2 = 2 * (uint64_t)n_mid + ((uint64_t)n + 1) + 2;
    if (pk_g1 && pk_g1_points != key1) ZK_FAIL(ZK_ERR_DOMAIN, "zk_pinocchio_keygen: G1 key length");
    if (pk_g2 && pk_g2_points != key2) ZK_FAIL(ZK_ERR_DOMAIN, "zk_pinocchio_keygen: G2 key length");
    ZKCHK(toxic_check(toxic, 8));          // KeyGen.generate divides by nothing: every trapdoor value below r is served
    ZKCHK(ensure_init());
    if (handle && ctx_count() > 1) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_keygen: a handle needs a device list of one entry (the key bytes can be had on any list)");
    Ctx& c = ctx();
    hipStream_t s = c.stream;
    const bool has_lag = handle && form == ZK_KEY_FORM_LAGRANGE;
    DevBuf tox, k, invf, lag, lam, pw, uks, d_mid, d_io, scr1, scr2;
    ZKCHK(tox.alloc(256));
    ZKCHK(k.alloc(32 * 10));
    ZKCHK(invf.alloc(32 * (size_t)n));
    ZKCHK(lag.alloc(32 * (size_t)n));
    ZKCHK(lam.alloc(32 * (size_t)n));
    ZKCHK(pw.alloc(32 * ((size_t)n + 1)));
    ZKCHK(uks.alloc(32 * 3 * (size_t)m));
    HIPCHK(hipMemcpyAsync(tox.p, toxic, 256, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_keygen_consts, dim3(1), dim3(64), 0, s, k.as<uint32_t>(), (const uint32_t*)tox.as<uint32_t>(), 8u);
    uint32_t* K = k.as<uint32_t>();
    const uint32_t* sp = K + 8 * 2;
    ZKCHK(frstage_invfact(invf.p, n, s));
    ZKCHK(lagrange_at_dev(lag.p, K + 8 * 9, n, 0, sp, invf.p, scr1, s));          // t = Z(s)
    ZKCHK(power_run(pw.p, sp, nullptr, (uint64_t)n + 1, s));
    if (has_lag && n > 1) ZKCHK(lagrange_at_dev(lam.p, nullptr, n - 1, n, sp, invf.p, scr2, s));
    ZKCHK(columns_at_dev(uks.p, n, m, L, R, O, lag.p, s));
    ZKCHK(upload_indices(d_mid, mids, s));
    ZKCHK(upload_indices(d_io, ios, s));
    const uint64_t o_vk = key1, o_hl = o_vk + 3 + 2 * (uint64_t)n_io, total1 = o_hl + (has_lag ? n : 0);
    const uint64_t q_si = 2 * (uint64_t)n_mid, q_one = q_si + n + 1, q_vk = key2, total2 = q_vk + 6 + n_io;
    DevBuf e1, e2, a1, a2;
    ZKCHK(e1.alloc(32 * total1));
    ZKCHK(e2.alloc(32 * total2));
    ZKCHK(a1.alloc(96 * total1));
    ZKCHK(a2.alloc(192 * total2));
    {
        PinAsm p = {e1.as<uint32_t>(), e2.as<uint32_t>(), K, pw.as<uint32_t>(), lam.as<uint32_t>(), uks.as<uint32_t>(), d_mid.as<uint32_t>(), d_io.as<uint32_t>(),
                    n, m, n_mid, n_io, has_lag ? 1u : 0u};
        ScopedTimer t("keygen_assemble", s);
        hipLaunchKernelGGL(k_pinocchio_assemble, g1d(total1 > total2 ? total1 : total2), dim3(256), 0, s, p);
        HIPCHK(hipGetLastError());
    }
    ZKCHK(fixed_base_mul(CURVE_G1, a1.p, e1.p, total1, s));
    if (pk_g2) {
        ZKCHK(fixed_base_mul(CURVE_G2, a2.p, e2.p, total2, s));
    } else {
        // si2 is part of the key's bytes only (no product of a proof reads it, pinocchio.ml:37-60): a call that asks for no G2 bytes skips its n + 1 points
        ZKCHK(fixed_base_mul(CURVE_G2, a2.p, e2.p, q_si, s));
        ZKCHK(fixed_base_mul(CURVE_G2, a2.as<uint8_t>() + 192 * q_one, e2.as<uint8_t>() + 32 * q_one, total2 - q_one, s));
    }
    DevBuf b1, b2, b3, b4;
    ZKCHK(emit_points(CURVE_G1, pk_g1, a1, 0, key1, b1, s));
    ZKCHK(emit_points(CURVE_G2, pk_g2, a2, 0, key2, b2, s));
    ZKCHK(emit_points(CURVE_G1, vk_g1, a1, o_vk, 3 + 2 * (uint64_t)n_io, b3, s));
    ZKCHK(emit_points(CURVE_G2, vk_g2, a2, q_vk, 6 + (uint64_t)n_io, b4, s));
    HIPCHK(hipStreamSynchronize(s));          // as in zk_groth16_keygen: the bytes are complete before a handle exists
    if (handle) ZKCHK(pin_key_from_device(n, m, L, R, O, mid, a1.as<uint8_t>(), a2.as<uint8_t>(), has_lag ? a1.as<uint8_t>() + 96 * o_hl : nullptr, handle));
    return ZK_OK;
}

}  // extern "C"
