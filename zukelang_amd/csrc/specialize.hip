// A phase-1 string specialised to a circuit: zk_groth16_pk_specialize (include/zkmi355x.h).
//
// Given [tau^i]_1, [alpha tau^i]_1, [beta tau^i]_1, [beta]_2, [tau^i]_2 and the circuit, the key of groth16.ml:45-108 for the trapdoor
// (alpha, beta, 1, 1, tau) is a LINEAR image of those points -- no secret is needed, none exists on this host:
//   [l_i]_1, [alpha l_i]_1, [beta l_i]_1   three derivations over the same tables        lagrange_derive.hip: specialize_g1_bases
//   tiztd[i] = sum_j z_j [tau^(i+j)]_1      one correlation in the exponent               the same function
//   ltd_mid / ltgm_io [k] = sum_i (L[i,k] [beta l_i] + R[i,k] [alpha l_i] + O[i,k] [l_i])   (groth16.ml:59-68: beta goes with L, alpha with R)
// The last line is the new work of this unit: a TRANSPOSED sparse product whose vector entries are group elements.  One output per variable, the
// matrices by column (transpose_csr, a counting pass on the host), and per entry a scalar multiplication -- 256 registers, a 16-point scratch table
// and ~1 600 field products (xyzz_mul_scalar_endo) -- unless the coefficient is 1 or r - 1, which R1CS matrices are mostly made of.  A branch that
// skips the multiplication saves nothing unless whole waves take it (see k_gntt_stage's j-major order), so the entries are split BY CLASS on the host:
//   (a) unit entries (c = 1, c = r - 1) name their base point, general entries are compacted into a list of their own; c = 0 is dropped;
//   (b) ONE chain of launches multiplies the compacted general entries: k_colsum_gather copies their base points into a raw XYZZ array, k_g_tabmul
//       (lagrange_derive.hip: g1_raw_tabmul, slabs of DERIVE_SLAB) multiplies it in place -- every lane of every wave multiplies;
//   (c) k_colsum walks each column's run of operands in chunks of COLSUM_C, one lane per chunk: an operand is the base point (y negated for r - 1) or
//       a product, every addition the general xyzz_add_impl (P + P, P + (-P), identity operands, an accumulator back at the identity in mid-run);
//   (d) a column of more than COLSUM_C operands leaves one partial per chunk, and the same kernel runs again over the partials until one point per
//       column remains (the variable `one` meets up to n rows).  An empty column is one chunk of no operands: the identity.
// No atomics; a lane's work is its own chunk, whatever the other columns hold.  All working arrays live for the call.
#include "ec.cuh"
#include "groth16_key.cuh"

#include <string.h>
#include <vector>

// 0: every kept entry is multiplied, the unit ones too (the measurement of DESIGN 2s; never the default)
#ifndef ZK_SPECIALIZE_SPLIT
#define ZK_SPECIALIZE_SPLIT 1
#endif

namespace zk {

static inline dim3 g1d(uint64_t n, unsigned t = 256) { return dim3((unsigned)((n + t - 1) / t)); }

static constexpr uint32_t COLSUM_C = 16;                       // operands one lane adds up
static constexpr uint32_t OP_GENERAL = 1u << 31;               // the operand is entry `index` of the product (or partial) array
static constexpr uint32_t OP_NEG = 1u << 30;                   // unit entry with c = r - 1: the base point negated
static constexpr uint32_t OP_INDEX = OP_NEG - 1;
static constexpr uint64_t COLSUM_MAX = OP_INDEX;               // operands, chunks and base points are 30-bit indices

// dst[i] = base[src[i]] in the raw XYZZ layout: the multiplicands of the general entries
__global__ void k_colsum_gather(uint8_t* __restrict__ dst, const uint8_t* __restrict__ base, const uint32_t* __restrict__ src, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    xyzz_store_raw<Fp>(dst + (uint64_t)RawLayout<Fp>::XYZZ * i, xyzz_from_aff(aff_load<Fp>(base + (uint64_t)96 * src[i])));
}
// out[j] = the sum of the operands cstart[j] .. cstart[j+1] - 1 (at most COLSUM_C of them; none: the identity).  ops == nullptr: operand e is pts[e]
// (the levels over the partials); else ops[e] names a base point, possibly negated, or an entry of pts (the products).
__global__ __launch_bounds__(128) void k_colsum(uint8_t* __restrict__ out, const uint32_t* __restrict__ cstart, uint32_t nchunks, const uint32_t* __restrict__ ops,
                                                const uint8_t* __restrict__ base, const uint8_t* __restrict__ pts) {
    constexpr uint64_t XB = RawLayout<Fp>::XYZZ;
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nchunks) return;
    const uint32_t lo = cstart[j], hi = cstart[j + 1];
    Xyzz<Fp> acc = xyzz_inf<Fp>();
#pragma unroll 1
    for (uint32_t e = lo; e < hi; e++) {
        const uint32_t op = ops ? ops[e] : (OP_GENERAL | e);
        Xyzz<Fp> q;
        if (op & OP_GENERAL) {
            q = xyzz_load_raw<Fp>(pts + XB * (op & OP_INDEX));
        } else {
            q = xyzz_from_aff(aff_load<Fp>(base + (uint64_t)96 * (op & OP_INDEX)));
            if (op & OP_NEG) q.y = Fp(fp_canon(fe_neg(q.y)));
        }
        xyzz_add_impl(acc, q);
    }
    xyzz_store_raw<Fp>(out + XB * j, acc);
}
// dst[i] = src[idx[i]], dense affine G1 points: the sums of the mid / io variables into key order
__global__ void k_pick_points_g1(uint4* __restrict__ dst, const uint4* __restrict__ src, const uint32_t* __restrict__ idx, uint64_t total_vec) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total_vec) return;
    dst[g] = src[(uint64_t)6 * idx[g / 6] + g % 6];
}

// ---- (a) the host's counting pass: the operands of every column, in column order
struct ColsumPlan {
    std::vector<uint32_t> ops;           // one per kept entry
    std::vector<uint32_t> col_end;       // col_end[k]: operands of the columns < k (m + 1 values)
    std::vector<uint32_t> gsrc;          // base index of every general entry
    std::vector<uint8_t> gk;             // its coefficient, 32 B
    uint64_t n_unit = 0, n_zero = 0;
    void begin() { col_end.assign(1, 0); }
    int add(uint64_t base_index, const uint8_t* coef) {
        uint64_t c[4], neg[4];
        cs_load(c, coef);
        if (!cs_canonical(c)) ZK_FAIL(ZK_ERR_SCALAR_RANGE, "a matrix coefficient is >= r");
        if (cs_is_zero(c)) { n_zero++; return ZK_OK; }
        if (base_index > COLSUM_MAX || ops.size() >= COLSUM_MAX) ZK_FAIL(ZK_ERR_ARG, "column sums: more than 2^30 - 1 entries or base points");
        (void)cs_sub(neg, CS_R, c);
        const bool unit = ZK_SPECIALIZE_SPLIT && (cs_is_one(c) || cs_is_one(neg));
        if (unit) {
            ops.push_back((uint32_t)base_index | (cs_is_one(c) ? 0u : OP_NEG));
            n_unit++;
        } else {
            ops.push_back(OP_GENERAL | (uint32_t)gsrc.size());
            gsrc.push_back((uint32_t)base_index);
            gk.insert(gk.end(), coef, coef + 32);
        }
        return ZK_OK;
    }
    void end_column() { col_end.push_back((uint32_t)ops.size()); }
};
template <class V> static int upload_vec(DevBuf& d, const V& v, hipStream_t s) {
    const size_t bytes = v.size() * sizeof(v[0]);
    ZKCHK(d.alloc(bytes ? bytes : 16));
    if (bytes) HIPCHK(hipMemcpyAsync(d.p, v.data(), bytes, hipMemcpyHostToDevice, s));
    return ZK_OK;
}
// (b) - (d) on the device: d_base = the dense affine points the plan's indices name -> d_out = m dense affine points, one per column.  Waits.
static int colsum_run(const ColsumPlan& p, uint32_t m, const uint8_t* d_base, uint8_t* d_out, hipStream_t s) {
    constexpr size_t XB = RawLayout<Fp>::XYZZ;
    const uint32_t ng = (uint32_t)p.gsrc.size();
    if ((uint64_t)p.ops.size() + m > COLSUM_MAX) ZK_FAIL(ZK_ERR_ARG, "column sums: more than 2^30 - 1 entries and columns");
    DevBuf d_ops, d_gsrc, d_gk, prod;
    ZKCHK(upload_vec(d_ops, p.ops, s));
    if (ng) {
        ZKCHK(upload_vec(d_gsrc, p.gsrc, s));
        ZKCHK(upload_vec(d_gk, p.gk, s));
        ZKCHK(prod.alloc(XB * ng));
        ScopedTimer t("specialize_mul", s);
        hipLaunchKernelGGL(k_colsum_gather, g1d(ng), dim3(256), 0, s, prod.as<uint8_t>(), d_base, (const uint32_t*)d_gsrc.as<uint32_t>(), ng);
        HIPCHK(hipGetLastError());
        ZKCHK(g1_raw_tabmul(prod.p, d_gk.p, ng, s));
    }
    // the levels: `len[k]` operands per column, chunks of COLSUM_C; an empty column is one empty chunk
    std::vector<uint32_t> len(m), cstart;
    for (uint32_t k = 0; k < m; k++) len[k] = p.col_end[k + 1] - p.col_end[k];
    DevBuf part[2], d_cstart[2];          // the stream runs behind the host: a level's arrays stay until the next but one
    const uint8_t* in = prod.as<uint8_t>();
    const uint32_t* ops = d_ops.as<uint32_t>();
    ScopedTimer t("specialize_sum", s);
    for (uint32_t level = 0;; level++) {
        cstart.clear();
        uint32_t at = 0;
        bool more = false;
        for (uint32_t k = 0; k < m; k++) {
            uint32_t left = len[k], chunks = 0;
            do {
                cstart.push_back(at);
                const uint32_t take = left < COLSUM_C ? left : COLSUM_C;
                at += take;
                left -= take;
                chunks++;
            } while (left);
            len[k] = chunks;
            more |= chunks > 1;
        }
        cstart.push_back(at);
        const uint32_t nchunks = (uint32_t)cstart.size() - 1;
        DevBuf &out = part[level & 1], &cs = d_cstart[level & 1];
        HIPCHK(hipStreamSynchronize(s));          // the buffers of level - 2 are reused, `cstart` of level - 1 has been read
        ZKCHK(out.alloc(XB * nchunks));
        ZKCHK(upload_vec(cs, cstart, s));
        hipLaunchKernelGGL(k_colsum, g1d(nchunks, 128), dim3(128), 0, s, out.as<uint8_t>(), (const uint32_t*)cs.as<uint32_t>(), nchunks, ops, d_base, in);
        HIPCHK(hipGetLastError());
        in = out.as<uint8_t>();
        ops = nullptr;
        if (!more) break;
    }
    ZKCHK(g1_raw_to_affine(d_out, in, m, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}

static int emit_points(Curve cv, uint8_t* host_out, const void* d_aff, uint64_t cnt, DevBuf& bytes, hipStream_t s) {
    if (!host_out || !cnt) return ZK_OK;
    const size_t pb = aff_bytes(cv);
    ZKCHK(bytes.alloc(pb * cnt));
    ZKCHK(points_affine_to_bytes(cv, bytes.p, d_aff, cnt, s));
    HIPCHK(hipMemcpyAsync(host_out, bytes.p, pb * cnt, hipMemcpyDeviceToHost, s));
    return ZK_OK;
}
static inline uint64_t srs_tau_g1(uint32_t n) { return (uint64_t)n + 2 > 2 * (uint64_t)n - 1 ? (uint64_t)n + 2 : 2 * (uint64_t)n - 1; }

}  // namespace zk

using namespace zk;
extern "C" {

int zk_groth16_srs_sizes(uint32_t n, uint64_t* tau_g1, uint64_t* ab_g1, uint64_t* tau_g2) {
    if (n < 1 || n > (1u << 24)) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_srs_sizes: constraint count must be in [1, 2^24]");
    if (tau_g1) *tau_g1 = srs_tau_g1(n);
    if (ab_g1) *ab_g1 = n;
    if (tau_g2) *tau_g2 = (uint64_t)n + 2;
    return ZK_OK;
}

int zk_groth16_pk_specialize(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t* srs_g1, size_t srs_g1_points,
                             const uint8_t* srs_g2, size_t srs_g2_points, uint32_t form, uint8_t* pk_g1, size_t pk_g1_points, uint8_t* pk_g2, size_t pk_g2_points,
                             uint8_t* vk_g1, uint8_t* vk_g2, uint64_t* handle) {
    if (!L || !R || !O || !mid || !srs_g1 || !srs_g2) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_pk_specialize: null argument");
    if (form != ZK_KEY_FORM_TAU_POWERS && form != ZK_KEY_FORM_LAGRANGE) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_pk_specialize: form must be ZK_KEY_FORM_TAU_POWERS or ZK_KEY_FORM_LAGRANGE");
    if (n < 1 || n > (1u << 24) || m == 0) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_pk_specialize: constraint count must be in [1, 2^24] and there must be a variable");
    std::vector<uint32_t> mids, ios;
    for (uint32_t k = 0; k < m; k++) (mid[k] ? mids : ios).push_back(k);
    const uint32_t n_mid = (uint32_t)mids.size(), n_io = (uint32_t)ios.size();
    const uint64_t T = srs_tau_g1(n), key1 = 3 + ((uint64_t)n + 2) + (n - 1) + n_mid, key2 = 2 + ((uint64_t)n + 2);
    if (srs_g1_points != T + 2 * (uint64_t)n) ZK_FAIL(ZK_ERR_DOMAIN, "zk_groth16_pk_specialize: G1 string length != max(n+2, 2n-1) + n + n");
    if (srs_g2_points != 1 + ((uint64_t)n + 2)) ZK_FAIL(ZK_ERR_DOMAIN, "zk_groth16_pk_specialize: G2 string length != 1 + (n+2)");
    if (pk_g1 && pk_g1_points != key1) ZK_FAIL(ZK_ERR_DOMAIN, "zk_groth16_pk_specialize: G1 key length != 3 + (n+2) + (n-1) + |mids|");
    if (pk_g2 && pk_g2_points != key2) ZK_FAIL(ZK_ERR_DOMAIN, "zk_groth16_pk_specialize: G2 key length != 2 + (n+2)");
    // ---- the matrices by column, one operand list: column k = its entries of L (on [beta l_i]), of R (on [alpha l_i]), of O (on [l_i])
    ColsumPlan plan;
    {
        const zk_csr* Ms[3] = {L, R, O};
        std::vector<uint32_t> ptr[3], row[3];
        std::vector<uint8_t> val[3];
        for (int q = 0; q < 3; q++) ZKCHK(transpose_csr(Ms[q], n, m, ptr[q], row[q], val[q]));
        plan.begin();
        for (uint32_t k = 0; k < m; k++) {
            for (int q = 0; q < 3; q++)
                for (uint32_t e = ptr[q][k]; e < ptr[q][k + 1]; e++) ZKCHK(plan.add((uint64_t)q * n + row[q][e], val[q].data() + 32 * (size_t)e));
            plan.end_column();
        }
    }
    ZKCHK(ensure_init());
    if (handle && ctx_count() > 1) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_pk_specialize: a handle needs a device list of one entry (the key bytes can be had on any list)");
    Ctx& c = ctx();
    hipStream_t s = c.stream;
    // ---- the string: five lists from outside, checked like the points of an uploaded key, the first bad list deciding
    const bool chk = key_subgroup_check();
    DevBuf s1, s2;
    ZKCHK(s1.alloc(96 * (T + 2 * (uint64_t)n)));
    ZKCHK(s2.alloc(192 * ((uint64_t)n + 3)));
    uint8_t *d_tau1 = s1.as<uint8_t>(), *d_at1 = d_tau1 + 96 * T, *d_bt1 = d_at1 + 96 * (uint64_t)n, *d_b2 = s2.as<uint8_t>(), *d_tau2 = d_b2 + 192;
    ZKCHK(points_from_bytes_checked(CURVE_G1, srs_g1, T, d_tau1, chk, s));
    ZKCHK(points_from_bytes_checked(CURVE_G1, srs_g1 + 96 * T, n, d_at1, chk, s));
    ZKCHK(points_from_bytes_checked(CURVE_G1, srs_g1 + 96 * (T + n), n, d_bt1, chk, s));
    ZKCHK(points_from_bytes_checked(CURVE_G2, srs_g2, 1, d_b2, chk, s));
    ZKCHK(points_from_bytes_checked(CURVE_G2, srs_g2 + 192, (uint64_t)n + 2, d_tau2, chk, s));
    // ---- the Lagrange-form lists and tiztd
    FrStage f;
    ZKCHK(frstage_init(f, n, m, L, R, O, s));
    DevBuf lab, sums, a1, a2, v1, v2, one, d_mid, d_io;
    ZKCHK(lab.alloc(96 * 3 * (uint64_t)n));          // [beta l_i] | [alpha l_i] | [l_i]: the plan's base indices
    ZKCHK(a1.alloc(96 * key1));
    ZKCHK(a2.alloc(192 * key2));
    uint8_t *d_bl = lab.as<uint8_t>(), *d_al = d_bl + 96 * (uint64_t)n, *d_l = d_al + 96 * (uint64_t)n;
    uint8_t *g1 = a1.as<uint8_t>(), *g2 = a2.as<uint8_t>();
    const uint64_t o_tz = 3 + ((uint64_t)n + 2), o_mid = o_tz + (n - 1);
    {
        const uint8_t* src[3] = {d_tau1, d_at1, d_bt1};
        uint8_t* dst[3] = {d_l, d_al, d_bl};
        ZKCHK(specialize_g1_bases(f, src, dst, d_tau1, g1 + 96 * o_tz, s));
    }
    // ---- the column sums of every variable, then into key order
    ZKCHK(sums.alloc(96 * (uint64_t)m));
    ZKCHK(colsum_run(plan, m, lab.as<uint8_t>(), sums.as<uint8_t>(), s));
    ZKCHK(upload_vec(d_mid, mids, s));
    ZKCHK(upload_vec(d_io, ios, s));
    ZKCHK(v1.alloc(96 * (1 + (uint64_t)n_io)));
    ZKCHK(v2.alloc(192 * 3));
    ZKCHK(one.alloc(32));
    {
        const uint8_t e_one[32] = {1};
        HIPCHK(hipMemcpyAsync(one.p, e_one, 32, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));          // e_one leaves with this block
    }
    ZKCHK(fixed_base_mul(CURVE_G1, v1.p, one.p, 1, s));                         // one1
    ZKCHK(fixed_base_mul(CURVE_G2, v2.p, one.p, 1, s));                         // one2 = gm = d: gamma = delta = 1
    HIPCHK(hipMemcpyAsync(v2.as<uint8_t>() + 192, v2.p, 192, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(v2.as<uint8_t>() + 384, v2.p, 192, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(g1, d_at1, 96, hipMemcpyDeviceToDevice, s));                                      // a
    HIPCHK(hipMemcpyAsync(g1 + 96, v1.p, 96, hipMemcpyDeviceToDevice, s));                                  // d1
    HIPCHK(hipMemcpyAsync(g1 + 192, d_bt1, 96, hipMemcpyDeviceToDevice, s));                                // b1
    HIPCHK(hipMemcpyAsync(g1 + 288, d_tau1, 96 * ((uint64_t)n + 2), hipMemcpyDeviceToDevice, s));           // ti1
    HIPCHK(hipMemcpyAsync(g2, d_b2, 192, hipMemcpyDeviceToDevice, s));                                      // b2
    HIPCHK(hipMemcpyAsync(g2 + 192, v2.p, 192, hipMemcpyDeviceToDevice, s));                                // d2
    HIPCHK(hipMemcpyAsync(g2 + 384, d_tau2, 192 * ((uint64_t)n + 2), hipMemcpyDeviceToDevice, s));          // ti2
    if (n_mid) hipLaunchKernelGGL(k_pick_points_g1, g1d(6 * (uint64_t)n_mid), dim3(256), 0, s, (uint4*)(g1 + 96 * o_mid), (const uint4*)sums.as<uint4>(), (const uint32_t*)d_mid.as<uint32_t>(), 6 * (uint64_t)n_mid);
    if (n_io) hipLaunchKernelGGL(k_pick_points_g1, g1d(6 * (uint64_t)n_io), dim3(256), 0, s, (uint4*)(v1.as<uint8_t>() + 96), (const uint4*)sums.as<uint4>(), (const uint32_t*)d_io.as<uint32_t>(), 6 * (uint64_t)n_io);
    HIPCHK(hipGetLastError());
    DevBuf b1, b2, b3, b4;
    ZKCHK(emit_points(CURVE_G1, pk_g1, g1, key1, b1, s));
    ZKCHK(emit_points(CURVE_G2, pk_g2, g2, key2, b2, s));
    ZKCHK(emit_points(CURVE_G1, vk_g1, v1.p, 1 + (uint64_t)n_io, b3, s));
    ZKCHK(emit_points(CURVE_G2, vk_g2, v2.p, 3, b4, s));
    HIPCHK(hipStreamSynchronize(s));          // as in zk_groth16_keygen: the bytes are complete before a handle exists
    if (!handle) return ZK_OK;
    if (form == ZK_KEY_FORM_TAU_POWERS) return groth16_key_from_device(n, m, L, R, O, mid, g1, key1, g2, key2, false, handle, chk);
    // Lagrange form: [l_i]_2 and the h bases are derived, [l_i]_1 is the list the column sums were taken over
    const uint64_t p1 = 3 + (uint64_t)n + (n - 1) + n_mid, p2 = 2 + (uint64_t)n;
    DevBuf l1, l2;
    ZKCHK(l1.alloc(96 * p1));
    ZKCHK(l2.alloc(192 * p2));
    ZKCHK(groth16_derive_lagrange_pools(f, g1, n_mid, g2, l1.as<uint8_t>(), l2.as<uint8_t>(), 2u | 4u, s));
    HIPCHK(hipMemcpyAsync(l1.as<uint8_t>() + 96 * 3, d_l, 96 * (uint64_t)n, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return groth16_key_from_device(n, m, L, R, O, mid, l1.p, p1, l2.p, p2, true, handle, chk);
}

// (a) - (d) on a caller's list (include/zkmi355x.h; tests/test_gpu_colsum.py).  Everything that can be refused is refused before the device is touched.
int zk_selftest_g1_colsum(const uint8_t* pts, size_t n_pts, const uint32_t* col_ptr, const uint32_t* row, const uint8_t* coef, uint32_t m, uint8_t* out) {
    if (!pts || !col_ptr || !out || n_pts == 0 || m == 0) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_g1_colsum: null argument, an empty list or no column");
    for (uint32_t k = 0; k < m; k++)
        if (col_ptr[k] > col_ptr[k + 1]) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_g1_colsum: col_ptr not monotone");
    if (col_ptr[m] > col_ptr[0] && (!row || !coef)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_g1_colsum: null row / coef");
    ColsumPlan plan;
    plan.begin();
    for (uint32_t k = 0; k < m; k++) {
        for (uint32_t e = col_ptr[k]; e < col_ptr[k + 1]; e++) {
            if (row[e] >= n_pts) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_g1_colsum: row index out of range");
            ZKCHK(plan.add(row[e], coef + 32 * (size_t)e));
        }
        plan.end_column();
    }
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    DevBuf dense, sums, bytes;
    ZKCHK(dense.alloc(96 * n_pts));
    ZKCHK(sums.alloc(96 * (uint64_t)m));
    ZKCHK(points_from_bytes_checked(CURVE_G1, pts, n_pts, dense.p, false, s));
    ZKCHK(colsum_run(plan, m, dense.as<uint8_t>(), sums.as<uint8_t>(), s));
    ZKCHK(emit_points(CURVE_G1, out, sums.p, m, bytes, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}

}  // extern "C"
