// Verification of many proofs under one key, on the device (include/zkmi355x.h: zk_groth16_vk_upload, zk_pinocchio_vk_upload, zk_vk_info, zk_vk_free,
// zk_groth16_verify_resident, zk_pinocchio_verify_resident, zk_groth16_verify_folded, and zk_groth16_verify_many, zk_pinocchio_verify_many): the
// verification-side twin of the resident MSM bases.  A verifier checks a stream of proofs under ONE key (Groth16.verify of groth16.ml:163-173, Verify.f of
// pinocchio.ml:254-420, the points through of_bytes_exn, curve.ml:199-212).  The key is decoded and checked ONCE, and a call moves only what belongs to
// its proofs.  ONE pipeline serves both kinds of call: a *_verify_many call builds the same key with the same code, keeps it out of the handle table,
// runs the same slabs and drops it when it returns -- a resident key that lives for one call.  Two fields of the key (VkChecks) tell the two apart and
// nothing else does: the subgroup test of every point (an uploaded key SUBGROUP_ENDO, a one-call key SUBGROUP_ORDER) and the timer family of the point
// checks (verify_point_checks / pairing_point_checks).
//
//   build    key bytes -> dense affine points on the device, every one checked (encoding, curve, subgroup: msm_points.hip); the IO points also as
//            narrow tables for the short products of msm_resident.hip, one per SHORT_BASES_MAX consecutive points of a list (an uploaded key holds at
//            most that many public inputs: one table per list; a one-call key has no such limit); `ab` kept as its 576 bytes.
//   verify   per slab of up to VK_SLAB proofs, on workspaces the key keeps and grows on demand:
//              1 one H2D copy: proofs | public inputs
//              2 k_vk_gather + k_bytes_to_affine_verdict + k_subgroup_verdict: every proof point decoded once, one verdict byte each
//              3 k_vk_scalar_range, k_vk_status: a public input >= r, then the proof's first failure in the host's order (verdict_order.h) -> one code byte per proof
//              4 one short product per IO sum, table and proof (k_msm_short; a rejected proof's product has no scalars), results stay on the device;
//                where a list has several tables, one xyzz_sum_columns launch adds their sums
//              5 k_vk_pairs_*: the pair lists assembled on the device -- G1 points negated as points (y -> p - y), Pinocchio's vio + vv, yio + yy,
//                wio + ww added here; a rejected proof gets identity pairs
//              6 k_miller, k_final_exp (pairing_dev.hip, unchanged), k_vk_compare against the 576 bytes of `ab` / of 1
//              7 one D2H copy: ok | code
//            The *_compressed calls bring the proofs as the reference's proof record holds them (192 / 480 B: 48 B per G1 point, 96 B per G2 point).
//            Steps 1-2 become: one H2D copy at that stride; one decompression launch per group, straight out of the slab buffer into the dense lists
//            and the verdict bytes (k_decompress_verdict, timer family verify_point_decompress); k_subgroup_verdict.  The rest is the same code.
// The verdicts are those of the host verifiers (pairing_host.hip), and the same under both subgroup tests: one predicate
// (tests/test_subgroup_criterion.py, tests/test_gpu_subgroup_endo.py).  Nothing here reads an option.
//
// zk_groth16_verify_folded answers ONE question about a batch -- are all of these proofs good? -- with one pairing equation instead of one per proof:
// with a secret random rho_i per proof,
//     prod_i e([rho_i] A_i, B_i) . e(-sum_k t_k ltgm_io_k, gm) . e(-sum_i [rho_i] C_i, d) = ab^S,    t_k = sum_i rho_i w_ik (mod r),  S = sum_i rho_i
// Steps 1-3 above are shared (vk_slab_front: the statuses are those of the per-proof call); then, per slab, on proofs that are still live:
//   k_fold_scale   [rho_i] A_i -> dense affine, [rho_i] C_i -> XYZZ: 128-bit double-and-add on the complete group law, one lane per point
//   k_fold_sum     the [rho_i] C_i and the running sum -> one point, by trees of complete additions in LDS, level after level
//   k_fold_fr      t_k += sum_i rho_i w_ik, S += sum_i rho_i, and the count of rejected proofs: one workgroup per k
//   k_miller over the pairs ([rho_i] A_i, B_i), pairing_tree_product_device over their values and the running product
// and once, after the last slab: one short product sum_k t_k ltgm_io_k, k_fold_key_pairs, k_miller on the two key pairs, k_final_exp on the product of
// the three values, pairing_gt_pow_device for ab^S, k_fold_verdict, and one D2H copy (codes | all_ok).  The kernels know nothing of Groth16: they scale
// and sum points, fold scalars and multiply Miller values; which points and which key pairs is decided in vk_fold.
#include "ec.cuh"
#include "handle_table.h"
#include "msm.cuh"
#include "verdict_order.h"

#include <memory>
#include <string.h>

namespace zk {

static constexpr uint32_t VK_MAX_PROOFS = 1u << 24;
static constexpr uint32_t VK_SLAB = 8192;          // proofs per pass: bounds the workspaces (Pinocchio: 20 KiB per proof) whatever the call's count
// ... and whatever the key's n_io: a slab's input buffer, stride + 32 n_io bytes per proof on the device and as many in its pinned twin, stays under this
// budget.  A slab holds VK_SLAB proofs whenever that fits (keys of up to some 2000 public inputs), and at least one.
static constexpr uint64_t VK_SLAB_BYTES = (uint64_t)1 << 30;

// 16-byte units of every proof's points -> the dense lists the decoder reads: G1 point q of proof i at g1[(n1 i + q) 96], G2 at g2[(n2 i + q) 192]
__global__ void k_vk_gather(const uint8_t* __restrict__ proofs, uint32_t count, VkPlan p, uint8_t* __restrict__ g1, uint8_t* __restrict__ g2) {
    const uint32_t per = 6 * p.n1 + 12 * p.n2;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)count * per) return;
    const uint32_t i = (uint32_t)(t / per), u = (uint32_t)(t - (uint64_t)i * per);
    const uint8_t* src = proofs + (size_t)p.stride * i;
    if (u < 6 * p.n1) {
        const uint32_t q = u / 6, w = u % 6;
        reinterpret_cast<uint4*>(g1 + 96 * ((size_t)p.n1 * i + q))[w] = reinterpret_cast<const uint4*>(src + p.off1[q])[w];
    } else {
        const uint32_t v = u - 6 * p.n1, q = v / 12, w = v % 12;
        reinterpret_cast<uint4*>(g2 + 192 * ((size_t)p.n2 * i + q))[w] = reinterpret_cast<const uint4*>(src + p.off2[q])[w];
    }
}
// bad[i] = 1 when one of proof i's n_io public inputs is >= r (bad is zeroed beforehand; every writer stores the same byte)
__global__ void k_vk_scalar_range(const uint32_t* __restrict__ scalars, uint64_t total, uint32_t n_io, uint8_t* __restrict__ bad) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    if (!fe_is_canonical(fe_load<FrParams>(scalars + 8 * t))) bad[t / n_io] = 1;
}
// code[i] = proof_code of verdict_order.h; live[i] = 1 iff code[i] == 0
__global__ void k_vk_status(const uint8_t* __restrict__ v1, const uint8_t* __restrict__ v2, const uint8_t* __restrict__ bad, uint32_t count, VkPlan p,
                            uint8_t* __restrict__ code, uint8_t* __restrict__ live) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint8_t c = proof_code(p, v1, v2, bad, i);
    code[i] = c;
    live[i] = c == 0 ? 1 : 0;
}

FF_INLINE Aff<Fp> g1_negated(const Aff<Fp>& p) {          // the identity stays (0, 0); no point of the curve has y = 0
    if (aff_is_inf(p)) return p;
    Aff<Fp> r;
    r.x = p.x;
    r.y = fe_neg(fp_assume<1>(p.y));
    return r;
}
template <int BYTES> FF_INLINE void copy_point(uint8_t* dst, const uint8_t* src) {
#pragma unroll
    for (int k = 0; k < BYTES / 16; k++) reinterpret_cast<uint4*>(dst)[k] = reinterpret_cast<const uint4*>(src)[k];
}
template <int BYTES> FF_INLINE void zero_point(uint8_t* dst) {
#pragma unroll
    for (int k = 0; k < BYTES / 16; k++) reinterpret_cast<uint4*>(dst)[k] = make_uint4(0, 0, 0, 0);
}
// Groth16, proof i: e(A, B) e(-acc, gm) e(-C, d), acc = sum_k w_k ltgm_io_k as dense XYZZ.  a1 = A | C per proof, a2 = B, key2 = gm | d.
__global__ __launch_bounds__(64) void k_vk_pairs_groth16(const uint8_t* __restrict__ a1, const uint8_t* __restrict__ a2, const uint8_t* __restrict__ key2,
                                                         const uint8_t* __restrict__ acc, const uint8_t* __restrict__ live, uint32_t count,
                                                         uint8_t* __restrict__ q1, uint8_t* __restrict__ q2, uint32_t* __restrict__ off) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    off[i] = 3 * i;
    if (i == count - 1) off[count] = 3 * count;
    uint8_t* o1 = q1 + 96 * 3 * (size_t)i;
    uint8_t* o2 = q2 + 192 * 3 * (size_t)i;
    if (!live[i]) {          // three pairs that contribute 1
        for (int k = 0; k < 3; k++) { zero_point<96>(o1 + 96 * k); zero_point<192>(o2 + 192 * k); }
        return;
    }
    copy_point<96>(o1, a1 + 96 * 2 * (size_t)i);
    aff_store<Fp>(o1 + 96, g1_negated(xyzz_to_aff(xyzz_load<Fp>(acc + 192 * (size_t)i))));
    aff_store<Fp>(o1 + 192, g1_negated(aff_load<Fp>(a1 + 96 * (2 * (size_t)i + 1))));
    copy_point<192>(o2, a2 + 192 * (size_t)i);
    copy_point<192>(o2 + 192, key2);
    copy_point<192>(o2 + 384, key2 + 192);
}
// Pinocchio, proof i: the thirteen pairs of the five equations (pinocchio.ml:285, 298, 311, 361-366, 418-420) in the order of zk_pinocchio_verify_many.
//   key1 = one | aw | bgm | ...    key2 = one2 | av | ay | gm2 | bgm2 | yt | ...    a1 = vv yy h vavv yayy bvwy per proof, a2 = ww waww
//   vio, yio (G1), wio (G2): the sums over the public inputs as dense XYZZ; vio + vv, yio + yy, wio + ww are added here (every case of the group law)
__global__ __launch_bounds__(64) void k_vk_pairs_pinocchio(const uint8_t* __restrict__ a1, const uint8_t* __restrict__ a2, const uint8_t* __restrict__ key1,
                                                           const uint8_t* __restrict__ key2, const uint8_t* __restrict__ vio, const uint8_t* __restrict__ yio,
                                                           const uint8_t* __restrict__ wio, const uint8_t* __restrict__ live, uint32_t count,
                                                           uint8_t* __restrict__ q1, uint8_t* __restrict__ q2, uint32_t* __restrict__ off) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    off[5 * i] = 13 * i; off[5 * i + 1] = 13 * i + 2; off[5 * i + 2] = 13 * i + 4; off[5 * i + 3] = 13 * i + 6; off[5 * i + 4] = 13 * i + 10;
    if (i == count - 1) off[5 * count] = 13 * count;
    uint8_t* o1 = q1 + 96 * 13 * (size_t)i;
    uint8_t* o2 = q2 + 192 * 13 * (size_t)i;
    if (!live[i]) {
        for (int k = 0; k < 13; k++) { zero_point<96>(o1 + 96 * k); zero_point<192>(o2 + 192 * k); }
        return;
    }
    const uint8_t* p1 = a1 + 96 * 6 * (size_t)i;
    const uint8_t* p2 = a2 + 192 * 2 * (size_t)i;
    const uint8_t *vv = p1, *yy = p1 + 96, *h = p1 + 192, *vavv = p1 + 288, *yayy = p1 + 384, *bvwy = p1 + 480, *ww = p2, *waww = p2 + 192;
    const uint8_t *one = key1, *aw = key1 + 96, *bgm = key1 + 192;
    const uint8_t *one2 = key2, *av = key2 + 192, *ay = key2 + 384, *gm2 = key2 + 576, *bgm2 = key2 + 768, *yt = key2 + 960;
    int k = 0;
    auto pair = [&](const uint8_t* g1p, bool neg, const uint8_t* g2p) {
        if (neg) aff_store<Fp>(o1 + 96 * k, g1_negated(aff_load<Fp>(g1p)));
        else copy_point<96>(o1 + 96 * k, g1p);
        copy_point<192>(o2 + 192 * k, g2p);
        k++;
    };
    pair(vv, false, av); pair(vavv, true, one2);
    pair(aw, false, ww); pair(one, true, waww);
    pair(yy, false, ay); pair(yayy, true, one2);
    pair(bvwy, false, gm2); pair(vv, true, bgm2); pair(bgm, true, ww); pair(yy, true, bgm2);
    {
        Xyzz<Fp> s = xyzz_load<Fp>(vio + 192 * (size_t)i);
        xyzz_madd(s, aff_load<Fp>(vv));
        aff_store<Fp>(o1 + 96 * 10, xyzz_to_aff(s));
        Xyzz<Fp2> w = xyzz_load<Fp2>(wio + 384 * (size_t)i);
        xyzz_madd(w, aff_load<Fp2>(ww));
        aff_store<Fp2>(o2 + 192 * 10, xyzz_to_aff(w));
        s = xyzz_load<Fp>(yio + 192 * (size_t)i);
        xyzz_madd(s, aff_load<Fp>(yy));
        aff_store<Fp>(o1 + 96 * 11, g1_negated(xyzz_to_aff(s)));
        copy_point<192>(o2 + 192 * 11, one2);
    }
    k = 12;
    pair(h, true, yt);
}
// ok[i] = 1 iff proof i is live and each of its `products` GT encodings equals the 576 bytes of `want`
__global__ void k_vk_compare(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ want, const uint8_t* __restrict__ live, uint32_t count, uint32_t products,
                             uint8_t* __restrict__ ok) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t diff = live[i] ? 0u : 1u;
    const uint4* w = reinterpret_cast<const uint4*>(want);
    for (uint32_t q = 0; q < products && !diff; q++) {
        const uint4* g = reinterpret_cast<const uint4*>(gt + 576 * ((size_t)products * i + q));
        for (int k = 0; k < 36; k++) {
            const uint4 a = g[k], b = w[k];
            diff |= (a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w);
        }
    }
    ok[i] = diff ? 0 : 1;
}

// ------------------------------------------------------------------ the folded verifier's kernels
// The scaling stage of both folds, one lane per (item, job).  A job takes a base point of item i -- point `pt` of its per_item dense affine points,
// plus point `add` of the same item (FOLD_ADD_IO: plus io[i], a sum over the public inputs as dense XYZZ; FOLD_NONE: nothing) -- multiplies it by
// coefficient `rho` of the item's rho_per_item (16 B little-endian each; FOLD_NONE: by 1) and writes the result to out_aff[i] as dense affine (dst
// FOLD_NONE) or to segment dst of out_xyzz as dense XYZZ.  Segment d holds count + 1 points: the items' and, behind them, the running sum carry[d] of
// the earlier slabs, which the lanes past the jobs copy there, so that one tree of k_fold_sum adds everything.  Lanes are job-major: the lanes of a
// wave share their job.  Items that are not live give the identity (zero bytes) and their points are not read.  xyzz_dbl / xyzz_madd are the complete
// ones: a base may be the identity (vio + vv = O, vv + yy = O), and nothing is assumed of rho.
enum : uint8_t { FOLD_NONE = 0xff, FOLD_ADD_IO = 0xfe };
struct FoldJob { uint8_t pt, add, rho, dst; };
struct FoldPlan {
    uint32_t njobs, per_item, rho_per_item, nseg;
    FoldJob job[9];
};
// Groth16 (a1 = A | C): [rho] A -> affine, [rho] C -> segment 0
static const FoldPlan FOLD_GROTH16 = {2, 2, 1, 1, {{0, FOLD_NONE, 0, FOLD_NONE}, {1, FOLD_NONE, 0, 0}}};
// Pinocchio, G1 (a1 = vv yy h vavv yayy bvwy): the eight segments are S_av | S_one2 in its three parts | S_ay | S_gm2 | S_bgm2 | S_yt, then the Miller
// loop's [rho_4](vio + vv)
static const FoldPlan FOLD_PINOCCHIO_G1 = {9, 6, 5, 8, {{0, FOLD_NONE, 0, 0}, {3, FOLD_NONE, 0, 1}, {4, FOLD_NONE, 2, 2}, {1, FOLD_NONE, 4, 3}, {1, FOLD_NONE, 2, 4},
                                                        {5, FOLD_NONE, 3, 5}, {0, 1, 3, 6}, {2, FOLD_NONE, 4, 7}, {0, FOLD_ADD_IO, 4, FOLD_NONE}}};
// Pinocchio, G2 (a2 = ww waww): T_aw | T_one | T_bgm, then the Miller loop's wio + ww
static const FoldPlan FOLD_PINOCCHIO_G2 = {4, 2, 5, 3, {{0, FOLD_NONE, 1, 0}, {1, FOLD_NONE, 1, 1}, {0, FOLD_NONE, 3, 2}, {0, FOLD_ADD_IO, FOLD_NONE, FOLD_NONE}}};
template <class F>
__global__ __launch_bounds__(64) void k_fold_scale(const uint8_t* __restrict__ pts, FoldPlan p, const uint8_t* __restrict__ io, const uint32_t* __restrict__ rho,
                                                   const uint8_t* __restrict__ live, uint32_t count, const uint8_t* __restrict__ carry, uint8_t* __restrict__ out_aff,
                                                   uint8_t* __restrict__ out_xyzz) {
    constexpr size_t AB = FieldOps<F>::WORDS * 8, XB = FieldOps<F>::WORDS * 16;          // a dense affine point, a dense XYZZ point
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, jobs = (uint64_t)p.njobs * count;
    if (j >= jobs + p.nseg) return;
    if (j >= jobs) {
        const uint32_t d = (uint32_t)(j - jobs);
        xyzz_store<F>(out_xyzz + XB * ((size_t)(count + 1) * d + count), xyzz_load<F>(carry + XB * d));
        return;
    }
    const FoldJob job = p.job[j / count];
    const uint32_t i = (uint32_t)(j % count);
    Xyzz<F> acc = xyzz_inf<F>();
    if (live[i]) {
        Aff<F> P = aff_load<F>(pts + AB * ((size_t)p.per_item * i + job.pt));
        if (job.add != FOLD_NONE) {
            acc = job.add == FOLD_ADD_IO ? xyzz_load<F>(io + XB * (size_t)i) : xyzz_from_aff(aff_load<F>(pts + AB * ((size_t)p.per_item * i + job.add)));
            xyzz_madd(acc, P);
            if (job.rho != FOLD_NONE) {
                P = xyzz_to_aff(acc);
                acc = xyzz_inf<F>();
            }
        } else if (job.rho == FOLD_NONE) acc = xyzz_from_aff(P);
        if (job.rho != FOLD_NONE) {
            const uint4 e = reinterpret_cast<const uint4*>(rho)[(size_t)p.rho_per_item * i + job.rho];
            const uint32_t w[4] = {e.x, e.y, e.z, e.w};
            for (int b = 127; b >= 0; b--) {
                acc = xyzz_dbl(acc);
                if ((w[b >> 5] >> (b & 31)) & 1) xyzz_madd(acc, P);
            }
        }
    }
    if (job.dst == FOLD_NONE) aff_store<F>(out_aff + AB * (size_t)i, xyzz_to_aff(acc));
    else xyzz_store<F>(out_xyzz + XB * ((size_t)(count + 1) * job.dst + i), acc);
}
// Segment blockIdx.y: out[out_stride y + blockIdx.x] = the sum of in[in_stride y + 64 blockIdx.x ...] (dense XYZZ, at most 64 of the segment's n; the
// strides count points): every lane takes one point (the identity past the end), then the wave halves them in LDS -- 16 KiB of raw points in G1,
// 32 KiB in G2, both under the 64 KiB a kernel may declare.  The additions are the complete xyzz_add: equal summands (a proof repeated with the same
// rho) and opposite ones occur.
static constexpr uint32_t FOLD_SUM_THREADS = 64;
template <class F>
__global__ __launch_bounds__(FOLD_SUM_THREADS) void k_fold_sum(const uint8_t* __restrict__ in, uint32_t n, uint32_t in_stride, uint8_t* __restrict__ out, uint32_t out_stride) {
    constexpr int RB = RawLayout<F>::XYZZ;
    constexpr size_t XB = FieldOps<F>::WORDS * 16;
    static_assert(FOLD_SUM_THREADS * RB <= 65536, "k_fold_sum: the raw points of one workgroup must fit the static LDS limit");
    __shared__ __attribute__((aligned(16))) uint8_t lds[FOLD_SUM_THREADS * RB];
    const uint32_t t = threadIdx.x, i = blockIdx.x * FOLD_SUM_THREADS + t;
    Xyzz<F> acc = xyzz_inf<F>();
    if (i < n) acc = xyzz_load<F>(in + XB * ((size_t)in_stride * blockIdx.y + i));
    xyzz_store_raw(lds + RB * t, acc);
    __syncthreads();
    for (uint32_t h = FOLD_SUM_THREADS / 2; h > 0; h >>= 1) {          // the bound is the workgroup's: every lane meets every barrier
        if (t < h) {
            const Xyzz<F> q = xyzz_load_raw<F>(lds + RB * (t + h));
            xyzz_add(acc, q);
            xyzz_store_raw(lds + RB * t, acc);
        }
        __syncthreads();
    }
    if (t == 0) xyzz_store<F>(out + XB * ((size_t)out_stride * blockIdx.y + blockIdx.x), acc);
}
// Workgroup k < n: t[k] += sum over the live items i of rho_i w[i n + k] (mod r); workgroup n: S += sum of the live rho_i (mod r; as an integer the sum
// stays below 2^152 < r; skipped when S is null) and *dead += the items that are not live.  rho_i = coefficient rho_at of the item's rho_per_item.
// w: canonical scalars (a live item's are: the range test ran), t and S canonical too.
static constexpr uint32_t FOLD_FR_THREADS = 256;
__global__ __launch_bounds__(FOLD_FR_THREADS) void k_fold_fr(const uint32_t* __restrict__ w, uint32_t n, const uint32_t* __restrict__ rho, uint32_t rho_per_item,
                                                             uint32_t rho_at, const uint8_t* __restrict__ live, uint32_t count, uint32_t* __restrict__ t,
                                                             uint32_t* __restrict__ S, uint32_t* __restrict__ dead) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[FOLD_FR_THREADS * 8];
    __shared__ uint32_t ndead;
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (lane == 0) ndead = 0;
    __syncthreads();
    Fr acc = fe_zero<FrParams>();
    uint32_t mine = 0;
    for (uint32_t i = lane; i < count; i += FOLD_FR_THREADS) {
        if (!live[i]) { mine++; continue; }
        const uint4 e = reinterpret_cast<const uint4*>(rho)[(size_t)rho_per_item * i + rho_at];
        Fr r = fe_zero<FrParams>();
        r.v[0] = e.x; r.v[1] = e.y; r.v[2] = e.z; r.v[3] = e.w;
        if (k < n) r = fe_mul(fe_to_mont(r), fe_load<FrParams>(w + 8 * ((size_t)n * i + k)));          // (rho R) w R^-1 = rho w
        acc = fe_add(acc, r);
    }
    if (k == n && mine) atomicAdd(&ndead, mine);
    fe_store(lds + 8 * lane, acc);
    __syncthreads();
    for (uint32_t h = FOLD_FR_THREADS / 2; h > 0; h >>= 1) {
        if (lane < h) {
            acc = fe_add(acc, fe_load<FrParams>(lds + 8 * (lane + h)));
            fe_store(lds + 8 * lane, acc);
        }
        __syncthreads();
    }
    if (lane == 0) {
        uint32_t* dst = k < n ? t + 8 * (size_t)k : S;
        if (dst) fe_store(dst, fe_add(acc, fe_load<FrParams>(dst)));
        if (k == n) *dead += ndead;
    }
}
// The two pairs of the key's side, (-p[0], key2[0]) and (-p[1], key2[1]), for two dense XYZZ points p -> q1 (2 x 96 B), q2 (2 x 192 B), and the offsets
// of ONE product over the three Miller values that lie together (the running product, then these two).
__global__ __launch_bounds__(64) void k_fold_key_pairs(const uint8_t* __restrict__ p, const uint8_t* __restrict__ key2, uint8_t* __restrict__ q1, uint8_t* __restrict__ q2,
                                                       uint32_t* __restrict__ off) {
    const uint32_t i = threadIdx.x;
    if (i >= 2) return;
    aff_store<Fp>(q1 + 96 * i, g1_negated(xyzz_to_aff(xyzz_load<Fp>(p + 192 * i))));
    copy_point<192>(q2 + 192 * i, key2 + 192 * i);
    off[i] = 3 * i;
}
// Pinocchio's nine pairs of the key's side, one lane each, in the order of the folded equation (include/zkmi355x.h):
//   (S_av, av) (-(S_one2 + S_yio), one2) (S_ay, ay) (S_gm2, gm2) (-S_bgm2, bgm2) (-S_yt, yt) | (aw, T_aw) (-one, T_one) (-bgm, T_bgm)
// s1: the eight running sums of FOLD_PINOCCHIO_G1's segments, s2: the three of FOLD_PINOCCHIO_G2's (dense XYZZ).  sums: seven dense XYZZ points
// S_av | S_one2 | S_ay | S_gm2 | S_bgm2 | S_yt | S_yio; the last is there already (the short product's), the first six are written here, un-negated, S_one2
// as the proofs' part alone -- its three parts and S_yio are added by the complete addition.  Negations are done as points.  off: the offsets of ONE
// product over the ten Miller values that lie together (the running product, then these nine).
__global__ __launch_bounds__(64) void k_fold_key_pairs_pinocchio(const uint8_t* __restrict__ s1, const uint8_t* __restrict__ s2, const uint8_t* __restrict__ key1,
                                                                 const uint8_t* __restrict__ key2, uint8_t* __restrict__ sums, uint8_t* __restrict__ q1,
                                                                 uint8_t* __restrict__ q2, uint32_t* __restrict__ off) {
    const uint32_t i = threadIdx.x;
    if (i >= 9) return;
    if (i < 2) off[i] = 10 * i;
    if (i < 6) {
        const uint32_t seg = i == 0 ? 0 : i + 2;                 // S_one2 takes segments 1, 2, 3
        const uint32_t k2 = i == 0 ? 1 : i == 1 ? 0 : i;         // key2 = one2 | av | ay | gm2 | bgm2 | yt
        Xyzz<Fp> s = xyzz_load<Fp>(s1 + 192 * (i == 1 ? 1 : seg));
        if (i == 1) {
            xyzz_add(s, xyzz_load<Fp>(s1 + 192 * 2));
            xyzz_add(s, xyzz_load<Fp>(s1 + 192 * 3));
        }
        xyzz_store<Fp>(sums + 192 * i, s);
        if (i == 1) xyzz_add(s, xyzz_load<Fp>(sums + 192 * 6));
        const Aff<Fp> a = xyzz_to_aff(s);
        aff_store<Fp>(q1 + 96 * i, i == 1 || i >= 4 ? g1_negated(a) : a);
        copy_point<192>(q2 + 192 * i, key2 + 192 * k2);
    } else {
        const uint32_t k1 = i == 6 ? 1 : i == 7 ? 0 : 2;         // key1 = one | aw | bgm
        const Aff<Fp> a = aff_load<Fp>(key1 + 96 * k1);
        aff_store<Fp>(q1 + 96 * i, i == 6 ? a : g1_negated(a));
        aff_store<Fp2>(q2 + 192 * i, xyzz_to_aff(xyzz_load<Fp2>(s2 + 384 * (i - 6))));
    }
}
// *all_ok = 1 iff no item was rejected, `want` was an element of Fp12 and the 576 bytes of both sides agree
__global__ void k_fold_verdict(const uint8_t* __restrict__ lhs, const uint8_t* __restrict__ rhs, const uint32_t* __restrict__ dead, const uint32_t* __restrict__ bad,
                               uint8_t* __restrict__ all_ok) {
    if (threadIdx.x) return;
    uint32_t diff = *dead | *bad;
    const uint4 *a = reinterpret_cast<const uint4*>(lhs), *b = reinterpret_cast<const uint4*>(rhs);
    for (int k = 0; k < 36; k++) diff |= (a[k].x ^ b[k].x) | (a[k].y ^ b[k].y) | (a[k].z ^ b[k].z) | (a[k].w ^ b[k].w);
    *all_ok = diff ? 0 : 1;
}

// ================================================================== host side
// what an uploaded key and the key of one *_verify_many call differ in
struct VkChecks {
    SubgroupTest test;                        // of every point of the key and of its proofs
    const char* family;                       // the timer family of those checks
};
static constexpr VkChecks CHECKS_UPLOADED = {SUBGROUP_ENDO, "verify_point_checks"}, CHECKS_ONE_CALL = {SUBGROUP_ORDER, "pairing_point_checks"};

struct ResidentVk {
    int protocol = 0;                         // 0 Groth16, 1 Pinocchio
    uint64_t n_io = 0;
    VkChecks checks = CHECKS_UPLOADED;
    uint32_t slab = VK_SLAB;                  // proofs per pass (VK_SLAB_BYTES)
    DevBuf key1, key2;                        // the key's points, dense affine.  Groth16: ltgm_io[n_io] / gm | d.  Pinocchio: the layouts of zk_pinocchio_verify
    DevBuf want;                              // 576 B: ab (Groth16) / the encoding of 1 (Pinocchio)
    std::vector<ShortBases*> io[3];           // Groth16: ltgm_io.  Pinocchio: vv_io, yy_io, ww_io.  One table per SHORT_BASES_MAX points of the list; none when n_io = 0
    DevBuf parts;                             // the tables' sums of one list for `cap` proofs, before they are added (lists of several tables only)
    // workspaces for `cap` proofs
    uint32_t cap = 0;
    DevBuf in, b1, b2, a1, a2, verdict, flags, sums, q1, q2, off, miller, gt;
    uint8_t* host = nullptr;                  // pinned: [proofs | scalars | rho] in, [ok | code | all_ok] out
    size_t host_bytes = 0;
    // the folded verifier: workspaces for `fold_cap` proofs, and the state a call carries from slab to slab
    uint32_t fold_cap = 0;
    DevBuf fa, fc, fsum, fm, fm2, fold;       // the Miller loops' G1 points, dense affine | the G1 multiples and the running sums, XYZZ segments | partial sums | Miller values | tree levels | the state
    DevBuf fa2, fc2;                          // Pinocchio: the Miller loops' G2 points | the G2 multiples and the running sums
    ~ResidentVk() {
        for (const std::vector<ShortBases*>& list : io)
            for (ShortBases* b : list) short_bases_free(b);
        if (host) (void)hipHostFree(host);
    }
};
// Where the folded call's state lies in ResidentVk::fold (offsets in bytes; everything from F_SUMS on is zeroed when a call begins)
enum : size_t {
    F_MILLER = 0,                             // three raw Miller values: the running product, then the two key pairs'
    F_SUMS = 3 * PAIRING_RAW_BYTES,                            // two XYZZ points in the order of key2 = gm | d: sum t_k ltgm_io_k | sum [rho_i] C_i
    F_SUM_C = F_SUMS + 192,
    F_S = F_SUMS + 384,                       // S, 32 B
    F_OFF = F_S + 32,                         // the offsets of the one product: 0, 3
    F_DEAD = F_OFF + 8,                       // rejected proofs so far
    F_BAD = F_DEAD + 4,                       // 1: `want` is no element of Fp12
    F_ONE = F_BAD + 4,                        // a `live` byte for the one short product (16 B with its padding)
    F_GT = F_ONE + 16,                        // lhs | rhs, 576 B each
    F_BYTES = F_GT + 1152,                    // the two sums in the ABI's encoding, 96 B each
    F_T = F_BYTES + 192,                      // t: n_io x 32 B
};
static_assert(F_SUMS % 16 == 0 && F_T % 16 == 0, "the state's points and scalars are read 16 bytes at a time");
// The same for a Pinocchio key (everything from PF_SUMS1 on is zeroed when a call begins)
enum : size_t {
    PF_MILLER = 0,                            // ten raw Miller values: the running product, then the nine key pairs'
    PF_SUMS1 = 10 * PAIRING_RAW_BYTES,        // the running sums of FOLD_PINOCCHIO_G1's eight segments, XYZZ
    PF_SUMS2 = PF_SUMS1 + 8 * 192,            // ... of FOLD_PINOCCHIO_G2's three
    PF_OUT1 = PF_SUMS2 + 3 * 384,             // S_av | S_one2 | S_ay | S_gm2 | S_bgm2 | S_yt | S_yio, XYZZ (k_fold_key_pairs_pinocchio)
    PF_OFF = PF_OUT1 + 7 * 192,               // the offsets of the one product: 0, 10
    PF_DEAD = PF_OFF + 8,                     // rejected proofs so far
    PF_BAD = PF_DEAD + 4,                     // stays 0: `want` is the encoding of 1
    PF_ONE = PF_BAD + 4,                      // a `live` byte for the one short product (16 B with its padding)
    PF_GT = PF_ONE + 16,                      // lhs, 576 B
    PF_BYTES = PF_GT + 576,                   // the ten sums in the ABI's encoding: 7 x 96 B, then 3 x 192 B
    PF_T = PF_BYTES + 7 * 96 + 3 * 192,       // t: n_io x 32 B
};
static_assert(PF_SUMS1 % 16 == 0 && PF_OFF % 16 == 0 && PF_T % 16 == 0, "the state's points and scalars are read 16 bytes at a time");
static constexpr size_t FOLD_RHO_BYTES[2] = {16, 80};          // per proof, by protocol: one coefficient / five
static const VkPlan& plan_of(const ResidentVk& k) { return k.protocol == 0 ? PLAN_GROTH16 : PLAN_PINOCCHIO; }
// a call's proofs lie `stride` bytes apart: the plan's, or the wire form's when the call brings compressed proofs (wire != null)
static size_t proof_stride(const ResidentVk& k, const VkWire* wire) { return wire ? wire->stride : plan_of(k).stride; }

// a range of its own (handle_table.h); like resident bases, a live verification key pins the device list
static HandleTable<ResidentVk>& g_vk = *new HandleTable<ResidentVk>(HANDLES_VERIFICATION_KEY, "unknown verification key handle");
static void vk_release() {
    if (!g_vk.size()) return;
    DeviceScope ds(0);
    g_vk.release_all();
}
static CleanupRegistrar g_vk_cleanup(vk_release);

static int vk_lookup(uint64_t handle, int protocol, ResidentVk** out) {
    if (!(*out = g_vk.find(handle))) ZK_FAIL(ZK_ERR_HANDLE, g_vk.unknown());
    if (protocol >= 0 && (*out)->protocol != protocol) ZK_FAIL(ZK_ERR_HANDLE, "the verification key handle belongs to the other protocol");
    return ZK_OK;
}
// ---- the builders: a key of either kind, not yet in the table.  vk_new touches no device; *_vk_fill decodes, checks and tabulates the key's points on
// stream s and waits for it.  A defect of the key is the caller's error, in the host verifier's order (verdict_order.h)
static std::unique_ptr<ResidentVk> vk_new(int protocol, uint64_t n_io, VkChecks checks) {
    auto k = std::make_unique<ResidentVk>();
    k->protocol = protocol;
    k->n_io = n_io;
    k->checks = checks;
    const uint64_t fit = VK_SLAB_BYTES / (2 * (plan_of(*k).stride + 32 * n_io));
    k->slab = fit >= VK_SLAB ? VK_SLAB : fit ? (uint32_t)fit : 1;
    return k;
}
// IO list q = the n_io dense affine points at d_affine (checked, in the subgroup) as narrow tables
static int vk_io_tables(ResidentVk& k, int q, Curve curve, const uint8_t* d_affine, hipStream_t s) {
    for (uint64_t lo = 0; lo < k.n_io; lo += SHORT_BASES_MAX) {
        ShortBases* b = nullptr;
        ZKCHK(short_bases_create(&b, curve, d_affine + aff_bytes(curve) * lo, k.n_io - lo < SHORT_BASES_MAX ? k.n_io - lo : SHORT_BASES_MAX, s));
        k.io[q].push_back(b);
    }
    return ZK_OK;
}
static int vk_finish(ResidentVk& k, const uint8_t want[576], hipStream_t s) {
    ZKCHK(k.want.alloc(576));
    HIPCHK(hipMemcpyAsync(k.want.p, want, 576, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));          // the tables are built, the caller's bytes are read
    return ZK_OK;
}
static int groth16_vk_fill(ResidentVk& k, const uint8_t ab[576], const uint8_t* ltgm_io, const uint8_t gm[192], const uint8_t d[192], hipStream_t s) {
    const size_t n_io = k.n_io;
    uint8_t g2[384];
    memcpy(g2, gm, 192);
    memcpy(g2 + 192, d, 192);
    std::vector<uint8_t> v1, v2;
    ZKCHK(points_decode_two_lists(ltgm_io, n_io, g2, 2, k.checks.family, k.checks.test, k.key1, k.key2, v1, v2, s));
    const KeyDefect bad = groth16_key_defect(v1.data(), v2.data(), n_io);
    if (bad.verdict) ZK_FAIL(verdict_code(bad.verdict), bad.what);
    ZKCHK(vk_io_tables(k, 0, CURVE_G1, k.key1.as<uint8_t>(), s));
    return vk_finish(k, ab, s);
}
static int pinocchio_vk_fill(ResidentVk& k, const uint8_t* vk_g1, const uint8_t* vk_g2, hipStream_t s) {
    const size_t n_io = k.n_io;
    std::vector<uint8_t> v1, v2;
    ZKCHK(points_decode_two_lists(vk_g1, 3 + 2 * n_io, vk_g2, 6 + n_io, k.checks.family, k.checks.test, k.key1, k.key2, v1, v2, s));
    const KeyDefect bad = pinocchio_key_defect(v1.data(), v2.data(), n_io);
    if (bad.verdict) ZK_FAIL(verdict_code(bad.verdict), bad.what);
    ZKCHK(vk_io_tables(k, 0, CURVE_G1, k.key1.as<uint8_t>() + 96 * 3, s));
    ZKCHK(vk_io_tables(k, 1, CURVE_G1, k.key1.as<uint8_t>() + 96 * (3 + n_io), s));
    ZKCHK(vk_io_tables(k, 2, CURVE_G2, k.key2.as<uint8_t>() + 192 * 6, s));
    uint8_t gt_one[576];
    gt_one_bytes(gt_one);
    return vk_finish(k, gt_one, s);
}

static int vk_reserve(ResidentVk& k, uint32_t c, hipStream_t s) {
    if (c <= k.cap) return ZK_OK;
    HIPCHK(hipStreamSynchronize(s));
    const VkPlan& p = plan_of(k);
    // what the folded call adds: rho behind the public inputs (16 B per proof under a Groth16 key, 80 B under a Pinocchio key), all_ok behind the codes
    const size_t fold = 1;
    const size_t n = c, in_bytes = ((size_t)p.stride + 32 * k.n_io + FOLD_RHO_BYTES[k.protocol]) * n, out_bytes = 2 * n + 16 * fold;
    const uint32_t nsum1 = k.protocol == 0 ? 1 : 2, nsum2 = k.protocol == 0 ? 0 : 1;
    k.cap = 0;
    ZKCHK(k.in.alloc(in_bytes));
    ZKCHK(k.b1.alloc(96 * p.n1 * n));
    ZKCHK(k.b2.alloc(192 * p.n2 * n));
    ZKCHK(k.a1.alloc(96 * p.n1 * n));
    ZKCHK(k.a2.alloc(192 * p.n2 * n));
    ZKCHK(k.verdict.alloc((p.n1 + p.n2) * n));
    ZKCHK(k.flags.alloc(4 * n + 16 * fold));  // scalar-range byte | live | ok | code (| all_ok)
    ZKCHK(k.sums.alloc((192 * nsum1 + 384 * nsum2) * n));
    const uint64_t tables = (k.n_io + SHORT_BASES_MAX - 1) / SHORT_BASES_MAX;          // per IO list
    if (tables > 1) ZKCHK(k.parts.alloc(xyzz_bytes(k.protocol == 0 ? CURVE_G1 : CURVE_G2) * tables * n));
    ZKCHK(k.q1.alloc(96 * p.pairs * n));
    ZKCHK(k.q2.alloc(192 * p.pairs * n));
    ZKCHK(k.off.alloc(4 * (p.products * n + 1)));
    ZKCHK(k.miller.alloc(pairing_miller_bytes(p.pairs * n)));
    ZKCHK(k.gt.alloc(576 * p.products * n));
    if (k.host) (void)hipHostFree(k.host);
    k.host = nullptr;
    k.host_bytes = in_bytes + out_bytes;
    HIPCHK(hipHostMalloc((void**)&k.host, k.host_bytes, hipHostMallocDefault));
    k.cap = c;
    return ZK_OK;
}

// The workspaces of the folded call on top of vk_reserve's
static int vk_reserve_fold(ResidentVk& k, uint32_t c, hipStream_t s) {
    ZKCHK(vk_reserve(k, c, s));
    if (!k.fold.p) ZKCHK(k.fold.alloc((k.protocol == 0 ? F_T : PF_T) + 32 * k.n_io));
    if (c <= k.fold_cap) return ZK_OK;
    HIPCHK(hipStreamSynchronize(s));
    const size_t n = c, nsum = (n + FOLD_SUM_THREADS) / FOLD_SUM_THREADS;          // partial sums of n + 1 points, per segment
    const size_t seg1 = k.protocol == 0 ? FOLD_GROTH16.nseg : FOLD_PINOCCHIO_G1.nseg, seg2 = k.protocol == 0 ? 0 : FOLD_PINOCCHIO_G2.nseg;
    k.fold_cap = 0;
    ZKCHK(k.fa.alloc(96 * n));
    ZKCHK(k.fc.alloc(192 * seg1 * (n + 1)));
    if (seg2) {
        ZKCHK(k.fa2.alloc(192 * n));
        ZKCHK(k.fc2.alloc(384 * seg2 * (n + 1)));
    }
    ZKCHK(k.fsum.alloc((192 * seg1 > 384 * seg2 ? 192 * seg1 : 384 * seg2) * (nsum + (nsum + FOLD_SUM_THREADS - 1) / FOLD_SUM_THREADS)));          // G1 and G2 take turns
    ZKCHK(k.fm.alloc(pairing_miller_bytes(n + 1)));
    ZKCHK(k.fm2.alloc(pairing_miller_bytes(pairing_tree_scratch(n + 1))));
    k.fold_cap = c;
    return ZK_OK;
}

// where the front half of a slab leaves its results
struct SlabFront {
    size_t pb, sb, rb;                        // bytes of the proofs, of the public inputs and of rho in k.in and k.host
    const uint32_t *d_sc, *d_rho;             // the public inputs and the folded call's rho on the device
    uint8_t *bad, *live, *d_ok, *code;        // k.flags
};
// proofs [0, c) of a slab, steps 1-3 of the file's header: the H2D copy (rho behind the public inputs when the folded call brings one), the decoder,
// the subgroup and range tests, one code and one live byte per proof.  wire != null: the proofs are compressed.  The copy moves them at their own stride
// (192 / 480 B, less than the workspaces were sized for) and ONE launch per group takes every point from where it lies in the slab buffer to the dense
// affine lists a1 / a2 and its verdict byte (points_decompress_verdicts): no gather, no 96 / 192-byte form in between, and nothing decoded twice.  The
// subgroup test then runs on those lists as it does behind the other decoder, and everything behind it is shared.
static int vk_slab_front(ResidentVk& k, const uint8_t* io_scalars, const uint8_t* proofs, const uint8_t* rho, const VkWire* wire, uint32_t c, SlabFront& f, hipStream_t s) {
    const VkPlan& p = plan_of(k);
    const size_t n = c, pb = proof_stride(k, wire) * n, sb = 32 * k.n_io * n, rb = rho ? FOLD_RHO_BYTES[k.protocol] * n : 0;
    memcpy(k.host, proofs, pb);
    if (sb) memcpy(k.host + pb, io_scalars, sb);
    if (rb) memcpy(k.host + pb + sb, rho, rb);
    HIPCHK(hipMemcpyAsync(k.in.p, k.host, pb + sb + rb, hipMemcpyHostToDevice, s));
    uint8_t *d_in = k.in.as<uint8_t>(), *bad = k.flags.as<uint8_t>(), *live = bad + n, *code = bad + 3 * n;
    uint8_t *v1 = k.verdict.as<uint8_t>(), *v2 = v1 + p.n1 * n;
    const uint32_t* d_sc = reinterpret_cast<const uint32_t*>(d_in + pb);
    f = SlabFront{pb, sb, rb, d_sc, reinterpret_cast<const uint32_t*>(d_in + pb + sb), bad, live, bad + 2 * n, code};
    HIPCHK(hipMemsetAsync(bad, 0, n, s));
    if (wire) {
        {
            ScopedTimer t("verify_point_decompress", s);
            ZKCHK(points_decompress_verdicts(CURVE_G2, k.a2.p, d_in, n, p.n2, wire->stride, wire->off2, v2, s));
            ZKCHK(points_decompress_verdicts(CURVE_G1, k.a1.p, d_in, n, p.n1, wire->stride, wire->off1, v1, s));
        }
        ScopedTimer t(k.checks.family, s);
        ZKCHK(points_subgroup_verdicts(CURVE_G2, k.a2.p, p.n2 * n, v2, k.checks.test, s));
        ZKCHK(points_subgroup_verdicts(CURVE_G1, k.a1.p, p.n1 * n, v1, k.checks.test, s));
    } else {
        hipLaunchKernelGGL(k_vk_gather, grid_for(n * (6 * p.n1 + 12 * p.n2), 256), dim3(256), 0, s, (const uint8_t*)d_in, c, p, k.b1.as<uint8_t>(), k.b2.as<uint8_t>());
        ScopedTimer t(k.checks.family, s);
        ZKCHK(points_decode_verdicts(CURVE_G2, k.a2.p, k.b2.p, p.n2 * n, v2, k.checks.test, s));
        ZKCHK(points_decode_verdicts(CURVE_G1, k.a1.p, k.b1.p, p.n1 * n, v1, k.checks.test, s));
    }
    if (sb) hipLaunchKernelGGL(k_vk_scalar_range, grid_for(k.n_io * n, 256), dim3(256), 0, s, d_sc, k.n_io * n, (uint32_t)k.n_io, bad);
    hipLaunchKernelGGL(k_vk_status, grid_for(n, 256), dim3(256), 0, s, (const uint8_t*)v1, (const uint8_t*)v2, (const uint8_t*)bad, c, p, code, live);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

// out[i] = sum_k scalars[i n_io + k] P_k over IO list q (2: the list in G2) for c proofs, dense XYZZ, the identity where live[i] == 0: one short product per
// table of the list, and where it has several, their sums added by the complete addition of xyzz_sum_columns
static int vk_io_sum(ResidentVk& k, int q, const uint32_t* d_sc, const uint8_t* live, uint32_t c, uint8_t* out, hipStream_t s) {
    const std::vector<ShortBases*>& tables = k.io[q];
    if (tables.size() == 1) return short_bases_run(*tables[0], d_sc, live, c, k.n_io, 0, out, s);
    const Curve curve = q == 2 ? CURVE_G2 : CURVE_G1;
    for (size_t j = 0; j < tables.size(); j++)
        ZKCHK(short_bases_run(*tables[j], d_sc, live, c, k.n_io, SHORT_BASES_MAX * j, k.parts.as<uint8_t>() + xyzz_bytes(curve) * c * j, s));
    ScopedTimer t("msm_short", s);
    return xyzz_sum_columns(curve, out, k.parts.p, (uint32_t)tables.size(), c, s);
}

// proofs [0, c) of a slab: everything of the file's header, steps 1-7 (front: steps 1-3 are already enqueued and left this)
static int vk_slab(ResidentVk& k, const uint8_t* io_scalars, const uint8_t* proofs, const VkWire* wire, uint32_t c, const SlabFront* front, uint8_t* ok, int32_t* status,
                   hipStream_t s) {
    const VkPlan& p = plan_of(k);
    const size_t n = c;
    SlabFront f;
    if (front) f = *front;
    else ZKCHK(vk_slab_front(k, io_scalars, proofs, nullptr, wire, c, f, s));
    const size_t pb = f.pb, sb = f.sb;
    const uint32_t* d_sc = f.d_sc;
    uint8_t *live = f.live, *d_ok = f.d_ok;
    // the sums over the public inputs: dense XYZZ, zero bytes = the identity (n_io = 0)
    uint8_t* sum[3] = {k.sums.as<uint8_t>(), k.sums.as<uint8_t>() + 192 * n, k.sums.as<uint8_t>() + 384 * n};
    const int nsums = k.protocol == 0 ? 1 : 3;
    if (!k.n_io) HIPCHK(hipMemsetAsync(k.sums.p, 0, k.protocol == 0 ? 192 * n : 768 * n, s));
    else
        for (int q = 0; q < nsums; q++) ZKCHK(vk_io_sum(k, q, d_sc, live, c, sum[q], s));
    if (k.protocol == 0)
        hipLaunchKernelGGL(k_vk_pairs_groth16, grid_for(n, 64), dim3(64), 0, s, (const uint8_t*)k.a1.as<uint8_t>(), (const uint8_t*)k.a2.as<uint8_t>(),
                           (const uint8_t*)k.key2.as<uint8_t>(), (const uint8_t*)sum[0], (const uint8_t*)live, c, k.q1.as<uint8_t>(), k.q2.as<uint8_t>(), k.off.as<uint32_t>());
    else
        hipLaunchKernelGGL(k_vk_pairs_pinocchio, grid_for(n, 64), dim3(64), 0, s, (const uint8_t*)k.a1.as<uint8_t>(), (const uint8_t*)k.a2.as<uint8_t>(),
                           (const uint8_t*)k.key1.as<uint8_t>(), (const uint8_t*)k.key2.as<uint8_t>(), (const uint8_t*)sum[0], (const uint8_t*)sum[1], (const uint8_t*)sum[2],
                           (const uint8_t*)live, c, k.q1.as<uint8_t>(), k.q2.as<uint8_t>(), k.off.as<uint32_t>());
    HIPCHK(hipGetLastError());
    ZKCHK(pairing_products_device(k.q1.as<uint8_t>(), k.q2.as<uint8_t>(), p.pairs * n, k.off.as<uint32_t>(), p.products * c, k.miller.as<uint32_t>(), k.gt.as<uint8_t>(), s));
    hipLaunchKernelGGL(k_vk_compare, grid_for(n, 64), dim3(64), 0, s, (const uint8_t*)k.gt.as<uint8_t>(), (const uint8_t*)k.want.as<uint8_t>(), (const uint8_t*)live, c,
                       p.products, d_ok);
    HIPCHK(hipGetLastError());
    uint8_t* h_out = k.host + pb + sb;
    HIPCHK(hipMemcpyAsync(h_out, d_ok, 2 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < c; i++) {
        ok[i] = h_out[i];
        if (status) status[i] = verdict_code(h_out[n + i]);
    }
    return ZK_OK;
}

// count >= 1 proofs under key k, slab after slab (the arguments are checked).  first: the front half of the first slab, where it is already enqueued
static int vk_run(ResidentVk& k, const uint8_t* io_scalars, const uint8_t* proofs, const VkWire* wire, uint32_t count, const SlabFront* first, uint8_t* ok, int32_t* status,
                  hipStream_t s) {
    ZKCHK(vk_reserve(k, count < k.slab ? count : k.slab, s));
    const size_t stride = proof_stride(k, wire);
    for (uint32_t lo = 0; lo < count; lo += k.slab) {
        const uint32_t c = count - lo < k.slab ? count - lo : k.slab;
        ZKCHK(vk_slab(k, k.n_io ? io_scalars + 32 * k.n_io * (size_t)lo : nullptr, proofs + stride * lo, wire, c, lo ? nullptr : first, ok + lo, status ? status + lo : nullptr, s));
    }
    return ZK_OK;
}
static int vk_verify(uint64_t handle, int protocol, const uint8_t* io_scalars, const uint8_t* proofs, const VkWire* wire, uint32_t count, uint8_t* ok, int32_t* status) {
    ResidentVk* kp;
    ZKCHK(vk_lookup(handle, protocol, &kp));
    if (!count) return ZK_OK;
    ResidentVk& k = *kp;
    if (!proofs || !ok || (k.n_io && !io_scalars)) ZK_FAIL(ZK_ERR_ARG, "verify_resident: null argument");
    if (count > VK_MAX_PROOFS) ZK_FAIL(ZK_ERR_ARG, "verify_resident: more than 2^24 proofs in one call");
    DeviceScope ds(0);
    return vk_run(k, io_scalars, proofs, wire, count, nullptr, ok, status, ctx().stream);
}
// A *_verify_many call (the arguments are checked, the device is current): the key of vk_new lives for this call and is in no table -- it draws no handle
// number, does not count among the live handles and does not pin the device list.  `fill` is its protocol's *_vk_fill.  The first slab's proof points are
// checked WHILE the key's are, on the context's two streams: neither needs the other, and [r] P = O is a chain of 254 doublings on one lane per point --
// some 20 ms for two G2 points as for thousands -- so one after the other they would cost a call twice that.  A defective key still fails the call before
// anything is written.  Nothing of the call is in flight when the key goes (as in zk_vk_free), whatever the call returns.
template <class Fill>
static int vk_verify_once(std::unique_ptr<ResidentVk> k, Fill fill, const uint8_t* io_scalars, const uint8_t* proofs, uint32_t count, uint8_t* ok, int32_t* status) {
    hipStream_t s = ctx().stream, s_key = ctx().stream2;
    const uint32_t c = count < k->slab ? count : k->slab;
    SlabFront f;
    int rc = vk_reserve(*k, c, s);
    if (!rc) rc = vk_slab_front(*k, io_scalars, proofs, nullptr, nullptr, c, f, s);
    if (!rc) rc = fill(*k, s_key);
    if (!rc) rc = vk_run(*k, io_scalars, proofs, nullptr, count, &f, ok, status, s);
    (void)hipStreamSynchronize(s_key);
    (void)hipStreamSynchronize(s);
    return rc;
}

// nseg segments of m dense XYZZ points each (m apart) at src -> their nseg sums, next to each other at dst: trees of k_fold_sum, level after level, the
// partial sums alternating between the halves of k.fsum
template <class F> static int vk_fold_sums(ResidentVk& k, const uint8_t* src, uint32_t m, uint32_t nseg, uint8_t* dst, hipStream_t s) {
    constexpr size_t XB = FieldOps<F>::WORDS * 16;
    const uint32_t first = (m + FOLD_SUM_THREADS - 1) / FOLD_SUM_THREADS;
    uint8_t* part[2] = {k.fsum.as<uint8_t>(), k.fsum.as<uint8_t>() + XB * nseg * first};
    uint32_t stride = m;
    for (int lvl = 0;; lvl ^= 1) {
        const uint32_t blocks = (m + FOLD_SUM_THREADS - 1) / FOLD_SUM_THREADS;
        uint8_t* out = blocks == 1 ? dst : part[lvl];
        hipLaunchKernelGGL(k_fold_sum<F>, dim3(blocks, nseg), dim3(FOLD_SUM_THREADS), 0, s, src, m, stride, out, blocks);
        if (blocks == 1) break;
        src = out;
        m = stride = blocks;
    }
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

// One slab of the folded call: the front half, then the slab's share of both sides folded into the state
static int vk_fold_slab(ResidentVk& k, const uint8_t* io_scalars, const uint8_t* proofs, const uint8_t* rho, const VkWire* wire, uint32_t c, bool first, bool last,
                        int32_t* status, uint8_t* all_ok, hipStream_t s) {
    const size_t n = c;
    const bool pin = k.protocol == 1;
    SlabFront f;
    ZKCHK(vk_slab_front(k, io_scalars, proofs, rho, wire, c, f, s));
    uint8_t* st = k.fold.as<uint8_t>();
    uint32_t* run = reinterpret_cast<uint32_t*>(st + (pin ? PF_MILLER : F_MILLER));
    const uint8_t* live = f.live;
    const uint8_t* miller2 = k.a2.as<uint8_t>();          // Groth16: the pairs ([rho_i] A_i, B_i)
    if (pin) {
        // vio and wio per proof, as the per-proof call forms them (zero bytes, the identity, when n_io = 0); yio is folded into t instead
        uint8_t *vio = k.sums.as<uint8_t>(), *wio = vio + 384 * n;
        if (!k.n_io) HIPCHK(hipMemsetAsync(k.sums.p, 0, 768 * n, s));
        else {
            ZKCHK(vk_io_sum(k, 0, f.d_sc, live, c, vio, s));
            ZKCHK(vk_io_sum(k, 2, f.d_sc, live, c, wio, s));
        }
        {
            ScopedTimer t("verify_fold_scale_g2", s);
            hipLaunchKernelGGL(k_fold_scale<Fp2>, grid_for(FOLD_PINOCCHIO_G2.njobs * n + FOLD_PINOCCHIO_G2.nseg, 64), dim3(64), 0, s, (const uint8_t*)k.a2.as<uint8_t>(),
                               FOLD_PINOCCHIO_G2, (const uint8_t*)wio, f.d_rho, live, c, (const uint8_t*)(st + PF_SUMS2), k.fa2.as<uint8_t>(), k.fc2.as<uint8_t>());
            HIPCHK(hipGetLastError());
        }
        ScopedTimer t("verify_fold_scale", s);
        hipLaunchKernelGGL(k_fold_scale<Fp>, grid_for(FOLD_PINOCCHIO_G1.njobs * n + FOLD_PINOCCHIO_G1.nseg, 64), dim3(64), 0, s, (const uint8_t*)k.a1.as<uint8_t>(),
                           FOLD_PINOCCHIO_G1, (const uint8_t*)vio, f.d_rho, live, c, (const uint8_t*)(st + PF_SUMS1), k.fa.as<uint8_t>(), k.fc.as<uint8_t>());
        HIPCHK(hipGetLastError());
        ZKCHK(vk_fold_sums<Fp2>(k, k.fc2.as<uint8_t>(), c + 1, FOLD_PINOCCHIO_G2.nseg, st + PF_SUMS2, s));
        ZKCHK(vk_fold_sums<Fp>(k, k.fc.as<uint8_t>(), c + 1, FOLD_PINOCCHIO_G1.nseg, st + PF_SUMS1, s));
        hipLaunchKernelGGL(k_fold_fr, dim3((unsigned)k.n_io + 1), dim3(FOLD_FR_THREADS), 0, s, f.d_sc, (uint32_t)k.n_io, f.d_rho, 5u, 4u, live, c,
                           reinterpret_cast<uint32_t*>(st + PF_T), (uint32_t*)nullptr, reinterpret_cast<uint32_t*>(st + PF_DEAD));
        HIPCHK(hipGetLastError());
        miller2 = k.fa2.as<uint8_t>();                    // the pairs ([rho_i4](vio_i + vv_i), wio_i + ww_i)
    } else {
        ScopedTimer t("verify_fold_scale", s);
        // a1 = A | C per proof; the running sum rides along behind the [rho_i] C_i
        hipLaunchKernelGGL(k_fold_scale<Fp>, grid_for(FOLD_GROTH16.njobs * n + FOLD_GROTH16.nseg, 64), dim3(64), 0, s, (const uint8_t*)k.a1.as<uint8_t>(), FOLD_GROTH16,
                           (const uint8_t*)nullptr, f.d_rho, live, c, (const uint8_t*)(st + F_SUM_C), k.fa.as<uint8_t>(), k.fc.as<uint8_t>());
        HIPCHK(hipGetLastError());
        ZKCHK(vk_fold_sums<Fp>(k, k.fc.as<uint8_t>(), c + 1, FOLD_GROTH16.nseg, st + F_SUM_C, s));
        hipLaunchKernelGGL(k_fold_fr, dim3((unsigned)k.n_io + 1), dim3(FOLD_FR_THREADS), 0, s, f.d_sc, (uint32_t)k.n_io, f.d_rho, 1u, 0u, live, c,
                           reinterpret_cast<uint32_t*>(st + F_T), reinterpret_cast<uint32_t*>(st + F_S), reinterpret_cast<uint32_t*>(st + F_DEAD));
        HIPCHK(hipGetLastError());
    }
    // A rejected proof's G1 point is the identity here (k_fold_scale), and k_miller writes 1 for a pair with an identity on either side whatever the
    // other holds: its loop has no inversion and no branch on data.  Under a Groth16 key such a proof's B is what the decoder left -- the identity for
    // a bad encoding or a point off the curve, else a point of the curve, possibly outside the subgroup -- never bytes that are no point; under a
    // Pinocchio key its G2 point is the identity too
    ZKCHK(pairing_miller_device(k.fa.as<uint8_t>(), miller2, n, k.fm.as<uint32_t>(), s));
    if (!first) HIPCHK(hipMemcpyAsync(k.fm.as<uint8_t>() + pairing_miller_bytes(n), run, pairing_miller_bytes(1), hipMemcpyDeviceToDevice, s));
    ZKCHK(pairing_tree_product_device(k.fm.as<uint32_t>(), c + (first ? 0 : 1), k.fm2.as<uint32_t>(), run, s));
    size_t out = n;
    if (last && pin) {
        // S_yio = sum_k t_k yy_io_k (zero bytes, the identity, when n_io = 0), the key's nine pairs, the one final exponentiation, the comparison with 1
        if (k.n_io) ZKCHK(vk_io_sum(k, 1, reinterpret_cast<const uint32_t*>(st + PF_T), st + PF_ONE, 1, st + PF_OUT1 + 6 * 192, s));
        hipLaunchKernelGGL(k_fold_key_pairs_pinocchio, dim3(1), dim3(64), 0, s, (const uint8_t*)(st + PF_SUMS1), (const uint8_t*)(st + PF_SUMS2),
                           (const uint8_t*)k.key1.as<uint8_t>(), (const uint8_t*)k.key2.as<uint8_t>(), st + PF_OUT1, k.q1.as<uint8_t>(), k.q2.as<uint8_t>(),
                           reinterpret_cast<uint32_t*>(st + PF_OFF));
        HIPCHK(hipGetLastError());
        ZKCHK(pairing_miller_device(k.q1.as<uint8_t>(), k.q2.as<uint8_t>(), 9, run + pairing_miller_bytes(1) / 4, s));
        ZKCHK(pairing_final_exp_device(run, reinterpret_cast<const uint32_t*>(st + PF_OFF), 1, st + PF_GT, s));
        hipLaunchKernelGGL(k_fold_verdict, dim3(1), dim3(64), 0, s, (const uint8_t*)(st + PF_GT), (const uint8_t*)k.want.as<uint8_t>(),
                           reinterpret_cast<const uint32_t*>(st + PF_DEAD), reinterpret_cast<const uint32_t*>(st + PF_BAD), f.code + n);
        HIPCHK(hipGetLastError());
        out = n + 1;
    } else if (last) {
        // sum_k t_k ltgm_io_k (zero bytes, the identity, when n_io = 0), the key's two pairs, the one final exponentiation, ab^S, the comparison
        if (k.n_io) ZKCHK(vk_io_sum(k, 0, reinterpret_cast<const uint32_t*>(st + F_T), st + F_ONE, 1, st + F_SUMS, s));
        hipLaunchKernelGGL(k_fold_key_pairs, dim3(1), dim3(64), 0, s, (const uint8_t*)(st + F_SUMS), (const uint8_t*)k.key2.as<uint8_t>(), k.q1.as<uint8_t>(),
                           k.q2.as<uint8_t>(), reinterpret_cast<uint32_t*>(st + F_OFF));
        HIPCHK(hipGetLastError());
        ZKCHK(pairing_miller_device(k.q1.as<uint8_t>(), k.q2.as<uint8_t>(), 2, run + pairing_miller_bytes(1) / 4, s));
        ZKCHK(pairing_final_exp_device(run, reinterpret_cast<const uint32_t*>(st + F_OFF), 1, st + F_GT, s));
        ZKCHK(pairing_gt_pow_device(k.want.as<uint8_t>(), reinterpret_cast<const uint32_t*>(st + F_S), 160, st + F_GT + 576, reinterpret_cast<uint32_t*>(st + F_BAD), s));
        hipLaunchKernelGGL(k_fold_verdict, dim3(1), dim3(64), 0, s, (const uint8_t*)(st + F_GT), (const uint8_t*)(st + F_GT + 576), reinterpret_cast<const uint32_t*>(st + F_DEAD),
                           reinterpret_cast<const uint32_t*>(st + F_BAD), f.code + n);
        HIPCHK(hipGetLastError());
        out = n + 1;
    }
    uint8_t* h_out = k.host + f.pb + f.sb + f.rb;
    HIPCHK(hipMemcpyAsync(h_out, f.code, out, hipMemcpyDeviceToHost, s));          // codes | all_ok
    HIPCHK(hipStreamSynchronize(s));
    if (status)
        for (uint32_t i = 0; i < c; i++) status[i] = verdict_code(h_out[i]);
    if (last) *all_ok = h_out[n];
    return ZK_OK;
}

// zk_groth16_verify_folded, zk_pinocchio_verify_folded and their hooks.  `debug`, or null: Groth16 lhs 576 | rhs 576 | sum_io 96 | sum_c 96; Pinocchio
// lhs 576 | the seven G1 sums 7 x 96 | the three G2 sums 3 x 192.  wire != null: the proofs are compressed (vk_slab_front)
static int vk_fold(uint64_t handle, int protocol, const uint8_t* io_scalars, const uint8_t* proofs, const VkWire* wire, const uint8_t* rho, uint32_t count, int* all_ok,
                   int32_t* status, uint8_t* debug) {
    // what needs no handle comes first: these are refused before the table or the device is looked at
    if (!all_ok) ZK_FAIL(ZK_ERR_ARG, "verify_folded: null argument");
    if (count > VK_MAX_PROOFS) ZK_FAIL(ZK_ERR_ARG, "verify_folded: more than 2^24 proofs in one call");
    if (count && (!proofs || !rho)) ZK_FAIL(ZK_ERR_ARG, "verify_folded: null argument");
    const size_t rho_bytes = FOLD_RHO_BYTES[protocol];
    for (size_t i = 0; i < rho_bytes / 16 * count; i++) {
        uint8_t any = 0;
        for (int b = 0; b < 16; b++) any |= rho[16 * i + b];
        if (!any) ZK_FAIL(ZK_ERR_ARG, protocol == 0 ? "verify_folded: a coefficient rho_i is zero" : "verify_folded: one of a proof's five coefficients rho is zero");
    }
    ResidentVk* kp;
    if (handle && !g_vk.find(handle)) ZKCHK(ensure_init());          // without a device no handle exists: say that, not that this one is unknown
    ZKCHK(vk_lookup(handle, protocol, &kp));
    if (!count) {
        *all_ok = 1;
        return ZK_OK;
    }
    ResidentVk& k = *kp;
    if (k.n_io && !io_scalars) ZK_FAIL(ZK_ERR_ARG, "verify_folded: null argument");
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    ZKCHK(vk_reserve_fold(k, count < k.slab ? count : k.slab, s));
    uint8_t* st = k.fold.as<uint8_t>();
    const size_t stride = proof_stride(k, wire);
    if (protocol == 0) HIPCHK(hipMemsetAsync(st + F_SUMS, 0, F_T + 32 * k.n_io - F_SUMS, s));
    else HIPCHK(hipMemsetAsync(st + PF_SUMS1, 0, PF_T + 32 * k.n_io - PF_SUMS1, s));
    HIPCHK(hipMemsetAsync(st + (protocol == 0 ? F_ONE : PF_ONE), 1, 1, s));
    uint8_t verdict = 0;
    for (uint32_t lo = 0; lo < count; lo += k.slab) {
        const uint32_t c = count - lo < k.slab ? count - lo : k.slab;
        ZKCHK(vk_fold_slab(k, k.n_io ? io_scalars + 32 * k.n_io * (size_t)lo : nullptr, proofs + stride * lo, rho + rho_bytes * lo, wire, c, lo == 0, lo + c == count,
                           status ? status + lo : nullptr, &verdict, s));
    }
    *all_ok = verdict;
    if (debug && protocol == 0) {
        ZKCHK(points_xyzz_to_bytes_dev(CURVE_G1, st + F_SUMS, 2, st + F_BYTES, s));
        HIPCHK(hipMemcpyAsync(debug, st + F_GT, 1152 + 192, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    } else if (debug) {
        ZKCHK(points_xyzz_to_bytes_dev(CURVE_G1, st + PF_OUT1, 7, st + PF_BYTES, s));
        ZKCHK(points_xyzz_to_bytes_dev(CURVE_G2, st + PF_SUMS2, 3, st + PF_BYTES + 7 * 96, s));
        HIPCHK(hipMemcpyAsync(debug, st + PF_GT, PF_T - PF_GT, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return ZK_OK;
}

}  // namespace zk

using namespace zk;
extern "C" {

int zk_groth16_vk_upload(const uint8_t ab[576], const uint8_t* ltgm_io, size_t n_io, const uint8_t gm[192], const uint8_t d[192], uint64_t* handle) {
    if (!ab || !gm || !d || !handle || (n_io && !ltgm_io)) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_vk_upload: null argument");
    if (n_io > SHORT_BASES_MAX) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_vk_upload: a resident key holds at most 2^13 public inputs (zk_groth16_verify_many has no such limit)");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    auto k = vk_new(0, n_io, CHECKS_UPLOADED);
    ZKCHK(groth16_vk_fill(*k, ab, ltgm_io, gm, d, ctx().stream));
    *handle = g_vk.add(std::move(k));
    return ZK_OK;
}

int zk_pinocchio_vk_upload(const uint8_t* vk_g1, const uint8_t* vk_g2, size_t n_io, uint64_t* handle) {
    if (!vk_g1 || !vk_g2 || !handle) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_vk_upload: null argument");
    if (n_io > SHORT_BASES_MAX) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_vk_upload: a resident key holds at most 2^13 public inputs (zk_pinocchio_verify_many has no such limit)");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    auto k = vk_new(1, n_io, CHECKS_UPLOADED);
    ZKCHK(pinocchio_vk_fill(*k, vk_g1, vk_g2, ctx().stream));
    *handle = g_vk.add(std::move(k));
    return ZK_OK;
}

// groth16.ml:163-173:  e(A, B) = ab * e(sum_k w_k ltgm_io_k, gm) * e(C, d), as zk_groth16_verify decides it: e(A, B) e(-acc, gm) e(-C, d) == ab on bytes
int zk_groth16_verify_many(const uint8_t ab[576], const uint8_t* ltgm_io, size_t n_io, const uint8_t gm[192], const uint8_t d[192], const uint8_t* io_scalars,
                           const uint8_t* proofs, uint32_t count, uint8_t* ok, int32_t* status) {
    if (!ab || !gm || !d || (n_io && !ltgm_io)) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_verify_many: null argument");
    if (!count) return ZK_OK;
    if (!proofs || !ok || (n_io && !io_scalars)) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_verify_many: null argument");
    if (count > VK_MAX_PROOFS) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_verify_many: more than 2^24 proofs in one call");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    return vk_verify_once(vk_new(0, n_io, CHECKS_ONE_CALL), [&](ResidentVk& k, hipStream_t s) { return groth16_vk_fill(k, ab, ltgm_io, gm, d, s); }, io_scalars, proofs, count,
                          ok, status);
}

// Verify.f, pinocchio.ml:254-420, as zk_pinocchio_verify decides it: five products of pairings, each equal to 1 (k_vk_pairs_pinocchio)
int zk_pinocchio_verify_many(const uint8_t* vk_g1, const uint8_t* vk_g2, size_t n_io, const uint8_t* io_scalars, const uint8_t* proofs, uint32_t count, uint8_t* ok,
                             int32_t* status) {
    if (!vk_g1 || !vk_g2) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_verify_many: null argument");
    if (!count) return ZK_OK;
    if (!proofs || !ok || (n_io && !io_scalars)) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_verify_many: null argument");
    if (count > VK_MAX_PROOFS) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_verify_many: more than 2^24 proofs in one call");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    return vk_verify_once(vk_new(1, n_io, CHECKS_ONE_CALL), [&](ResidentVk& k, hipStream_t s) { return pinocchio_vk_fill(k, vk_g1, vk_g2, s); }, io_scalars, proofs, count, ok,
                          status);
}

int zk_vk_info(uint64_t handle, int* protocol, uint64_t* n_io) {
    ResidentVk* k;
    ZKCHK(vk_lookup(handle, -1, &k));
    if (protocol) *protocol = k->protocol;
    if (n_io) *n_io = k->n_io;
    return ZK_OK;
}

int zk_vk_free(uint64_t handle) {
    if (!g_vk.find(handle)) ZK_FAIL(ZK_ERR_HANDLE, g_vk.unknown());
    DeviceScope ds(0);
    (void)hipStreamSynchronize(ctx().stream);
    g_vk.take(handle);
    return ZK_OK;
}

int zk_groth16_verify_resident(uint64_t handle, const uint8_t* io_scalars, const uint8_t* proofs, uint32_t count, uint8_t* ok, int32_t* status) {
    return vk_verify(handle, 0, io_scalars, proofs, nullptr, count, ok, status);
}
int zk_pinocchio_verify_resident(uint64_t handle, const uint8_t* io_scalars, const uint8_t* proofs, uint32_t count, uint8_t* ok, int32_t* status) {
    return vk_verify(handle, 1, io_scalars, proofs, nullptr, count, ok, status);
}
int zk_groth16_verify_folded(uint64_t vk_handle, const uint8_t* io_scalars, const uint8_t* proofs, const uint8_t* rho, uint32_t count, int* all_ok, int32_t* status) {
    return vk_fold(vk_handle, 0, io_scalars, proofs, nullptr, rho, count, all_ok, status, nullptr);
}
int zk_pinocchio_verify_folded(uint64_t vk_handle, const uint8_t* io_scalars, const uint8_t* proofs, const uint8_t* rho, uint32_t count, int* all_ok, int32_t* status) {
    return vk_fold(vk_handle, 1, io_scalars, proofs, nullptr, rho, count, all_ok, status, nullptr);
}
// the same four calls on proofs in their compressed wire form: one more argument on the way down, and the slab's front half decompresses
int zk_groth16_verify_resident_compressed(uint64_t handle, const uint8_t* io_scalars, const uint8_t* proofs, uint32_t count, uint8_t* ok, int32_t* status) {
    return vk_verify(handle, 0, io_scalars, proofs, &WIRE_GROTH16, count, ok, status);
}
int zk_pinocchio_verify_resident_compressed(uint64_t handle, const uint8_t* io_scalars, const uint8_t* proofs, uint32_t count, uint8_t* ok, int32_t* status) {
    return vk_verify(handle, 1, io_scalars, proofs, &WIRE_PINOCCHIO, count, ok, status);
}
int zk_groth16_verify_folded_compressed(uint64_t vk_handle, const uint8_t* io_scalars, const uint8_t* proofs, const uint8_t* rho, uint32_t count, int* all_ok,
                                        int32_t* status) {
    return vk_fold(vk_handle, 0, io_scalars, proofs, &WIRE_GROTH16, rho, count, all_ok, status, nullptr);
}
int zk_pinocchio_verify_folded_compressed(uint64_t vk_handle, const uint8_t* io_scalars, const uint8_t* proofs, const uint8_t* rho, uint32_t count, int* all_ok,
                                          int32_t* status) {
    return vk_fold(vk_handle, 1, io_scalars, proofs, &WIRE_PINOCCHIO, rho, count, all_ok, status, nullptr);
}
int zk_selftest_groth16_fold(uint64_t vk_handle, const uint8_t* io_scalars, const uint8_t* proofs, const uint8_t* rho, uint32_t count, uint8_t lhs_gt[576],
                             uint8_t rhs_gt[576], uint8_t sum_c[96], uint8_t sum_io[96], int32_t* status) {
    if (!count || !lhs_gt || !rhs_gt || !sum_c || !sum_io) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_groth16_fold: null argument or no proofs");
    uint8_t out[1152 + 192];
    int all_ok = 0;
    ZKCHK(vk_fold(vk_handle, 0, io_scalars, proofs, nullptr, rho, count, &all_ok, status, out));
    memcpy(lhs_gt, out, 576);
    memcpy(rhs_gt, out + 576, 576);
    memcpy(sum_io, out + 1152, 96);
    memcpy(sum_c, out + 1248, 96);
    return ZK_OK;
}
int zk_selftest_pinocchio_fold(uint64_t vk_handle, const uint8_t* io_scalars, const uint8_t* proofs, const uint8_t* rho, uint32_t count, uint8_t lhs_gt[576],
                               uint8_t sums_g1[7 * 96], uint8_t sums_g2[3 * 192], int32_t* status) {
    if (!count || !lhs_gt || !sums_g1 || !sums_g2) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_pinocchio_fold: null argument or no proofs");
    uint8_t out[576 + 7 * 96 + 3 * 192];
    int all_ok = 0;
    ZKCHK(vk_fold(vk_handle, 1, io_scalars, proofs, nullptr, rho, count, &all_ok, status, out));
    memcpy(lhs_gt, out, 576);
    memcpy(sums_g1, out + 576, 7 * 96);
    memcpy(sums_g2, out + 576 + 7 * 96, 3 * 192);
    return ZK_OK;
}
}
