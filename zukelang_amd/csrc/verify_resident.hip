// Verification keys resident on the device (include/zkmi355x.h: zk_groth16_vk_upload, zk_pinocchio_vk_upload, zk_vk_info, zk_vk_free,
// zk_groth16_verify_resident, zk_pinocchio_verify_resident): the verification-side twin of the resident MSM bases.  A verifier checks a stream of proofs
// under ONE key (Groth16.verify of groth16.ml:163-173, Verify.f of pinocchio.ml:254-420, the points through of_bytes_exn, curve.ml:199-212), and the
// batched verifiers of pairing_dev.hip pay for the key again in every call: its points are decoded and subgroup-checked, its IO points go through the
// public zk_bases_upload (a second decode and check, window tables, a pinned arena), and a dozen buffers are allocated and freed.  Here the key is
// decoded and checked ONCE, and a call moves only what belongs to its proofs:
//
//   upload   key bytes -> dense affine points on the device, every one checked (encoding, curve, subgroup by endomorphism: SUBGROUP_ENDO of
//            msm_points.hip); the IO points also as a narrow table for the short products of msm_resident.hip; `ab` kept as its 576 bytes.
//   verify   per slab of up to VK_SLAB proofs, on workspaces the handle keeps and grows on demand:
//              1 one H2D copy: proofs | public inputs
//              2 k_vk_gather + k_bytes_to_affine_verdict + k_subgroup_verdict: every proof point decoded once, one verdict byte each
//              3 k_vk_scalar_range, k_vk_status: a public input >= r, then the proof's first failure in the host's order (verdict_order.h) -> one code byte per proof
//              4 one short product per IO sum and proof (k_msm_short; a rejected proof's product has no scalars), results stay on the device
//              5 k_vk_pairs_*: the pair lists assembled on the device -- G1 points negated as points (y -> p - y), Pinocchio's vio + vv, yio + yy,
//                wio + ww added here; a rejected proof gets identity pairs
//              6 k_miller, k_final_exp (pairing_dev.hip, unchanged), k_vk_compare against the 576 bytes of `ab` / of 1
//              7 one D2H copy: ok | code
// The verdicts are those of zk_*_verify_many byte for byte: the same decoder, the same order of checks, the same pairs into the same two kernels, and
// a subgroup verdict that is the same predicate (tests/test_subgroup_criterion.py, tests/test_gpu_subgroup_endo.py).  Nothing here reads an option.
#include "ec.cuh"
#include "handle_table.h"
#include "msm.cuh"
#include "verdict_order.h"

#include <memory>
#include <string.h>

namespace zk {

static constexpr uint32_t VK_MAX_PROOFS = 1u << 24;
static constexpr uint32_t VK_SLAB = 8192;          // proofs per pass: bounds the workspaces (Pinocchio: 20 KiB per proof) whatever the call's count

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

// ================================================================== host side
struct ResidentVk {
    int protocol = 0;                         // 0 Groth16, 1 Pinocchio
    uint64_t n_io = 0;
    DevBuf key1, key2;                        // the key's points, dense affine.  Groth16: ltgm_io[n_io] / gm | d.  Pinocchio: the layouts of zk_pinocchio_verify
    DevBuf want;                              // 576 B: ab (Groth16) / the encoding of 1 (Pinocchio)
    ShortBases* io[3] = {nullptr, nullptr, nullptr};          // Groth16: ltgm_io.  Pinocchio: vv_io, yy_io, ww_io.  null when n_io = 0
    // workspaces for `cap` proofs
    uint32_t cap = 0;
    DevBuf in, b1, b2, a1, a2, verdict, flags, sums, q1, q2, off, miller, gt;
    uint8_t* host = nullptr;                  // pinned: [proofs | scalars] in, [ok | code] out
    size_t host_bytes = 0;
    ~ResidentVk() {
        for (ShortBases* b : io) short_bases_free(b);
        if (host) (void)hipHostFree(host);
    }
};
static const VkPlan& plan_of(const ResidentVk& k) { return k.protocol == 0 ? PLAN_GROTH16 : PLAN_PINOCCHIO; }

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
static int vk_install(std::unique_ptr<ResidentVk>& k, const uint8_t want[576], hipStream_t s, uint64_t* handle) {
    ZKCHK(k->want.alloc(576));
    HIPCHK(hipMemcpyAsync(k->want.p, want, 576, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));          // the tables are built, the caller's bytes are read
    *handle = g_vk.add(std::move(k));
    return ZK_OK;
}

static int vk_reserve(ResidentVk& k, uint32_t c, hipStream_t s) {
    if (c <= k.cap) return ZK_OK;
    HIPCHK(hipStreamSynchronize(s));
    const VkPlan& p = plan_of(k);
    const size_t n = c, in_bytes = ((size_t)p.stride + 32 * k.n_io) * n, out_bytes = 2 * n;
    const uint32_t nsum1 = k.protocol == 0 ? 1 : 2, nsum2 = k.protocol == 0 ? 0 : 1;
    k.cap = 0;
    ZKCHK(k.in.alloc(in_bytes));
    ZKCHK(k.b1.alloc(96 * p.n1 * n));
    ZKCHK(k.b2.alloc(192 * p.n2 * n));
    ZKCHK(k.a1.alloc(96 * p.n1 * n));
    ZKCHK(k.a2.alloc(192 * p.n2 * n));
    ZKCHK(k.verdict.alloc((p.n1 + p.n2) * n));
    ZKCHK(k.flags.alloc(4 * n));              // scalar-range byte | live | ok | code
    ZKCHK(k.sums.alloc((192 * nsum1 + 384 * nsum2) * n));
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

// proofs [0, c) of a slab: everything of the file's header, steps 1-7
static int vk_slab(ResidentVk& k, const uint8_t* io_scalars, const uint8_t* proofs, uint32_t c, uint8_t* ok, int32_t* status, hipStream_t s) {
    const VkPlan& p = plan_of(k);
    const size_t n = c, pb = (size_t)p.stride * n, sb = 32 * k.n_io * n;
    memcpy(k.host, proofs, pb);
    if (sb) memcpy(k.host + pb, io_scalars, sb);
    HIPCHK(hipMemcpyAsync(k.in.p, k.host, pb + sb, hipMemcpyHostToDevice, s));
    uint8_t *d_in = k.in.as<uint8_t>(), *bad = k.flags.as<uint8_t>(), *live = bad + n, *d_ok = bad + 2 * n, *code = bad + 3 * n;
    uint8_t *v1 = k.verdict.as<uint8_t>(), *v2 = v1 + p.n1 * n;
    const uint32_t* d_sc = reinterpret_cast<const uint32_t*>(d_in + pb);
    HIPCHK(hipMemsetAsync(bad, 0, n, s));
    hipLaunchKernelGGL(k_vk_gather, grid_for(n * (6 * p.n1 + 12 * p.n2), 256), dim3(256), 0, s, (const uint8_t*)d_in, c, p, k.b1.as<uint8_t>(), k.b2.as<uint8_t>());
    {
        ScopedTimer t("verify_point_checks", s);
        ZKCHK(points_decode_verdicts(CURVE_G2, k.a2.p, k.b2.p, p.n2 * n, v2, SUBGROUP_ENDO, s));
        ZKCHK(points_decode_verdicts(CURVE_G1, k.a1.p, k.b1.p, p.n1 * n, v1, SUBGROUP_ENDO, s));
    }
    if (sb) hipLaunchKernelGGL(k_vk_scalar_range, grid_for(k.n_io * n, 256), dim3(256), 0, s, d_sc, k.n_io * n, (uint32_t)k.n_io, bad);
    hipLaunchKernelGGL(k_vk_status, grid_for(n, 256), dim3(256), 0, s, (const uint8_t*)v1, (const uint8_t*)v2, (const uint8_t*)bad, c, p, code, live);
    HIPCHK(hipGetLastError());
    // the sums over the public inputs: dense XYZZ, zero bytes = the identity (n_io = 0)
    uint8_t* sum[3] = {k.sums.as<uint8_t>(), k.sums.as<uint8_t>() + 192 * n, k.sums.as<uint8_t>() + 384 * n};
    const int nsums = k.protocol == 0 ? 1 : 3;
    if (!k.n_io) HIPCHK(hipMemsetAsync(k.sums.p, 0, k.protocol == 0 ? 192 * n : 768 * n, s));
    else
        for (int q = 0; q < nsums; q++) ZKCHK(short_bases_run(*k.io[q], d_sc, live, c, sum[q], s));
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

static int vk_verify(uint64_t handle, int protocol, const uint8_t* io_scalars, const uint8_t* proofs, uint32_t count, uint8_t* ok, int32_t* status) {
    ResidentVk* kp;
    ZKCHK(vk_lookup(handle, protocol, &kp));
    if (!count) return ZK_OK;
    ResidentVk& k = *kp;
    if (!proofs || !ok || (k.n_io && !io_scalars)) ZK_FAIL(ZK_ERR_ARG, "verify_resident: null argument");
    if (count > VK_MAX_PROOFS) ZK_FAIL(ZK_ERR_ARG, "verify_resident: more than 2^24 proofs in one call");
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    ZKCHK(vk_reserve(k, count < VK_SLAB ? count : VK_SLAB, s));
    const size_t stride = plan_of(k).stride;
    for (uint32_t lo = 0; lo < count; lo += VK_SLAB) {
        const uint32_t c = count - lo < VK_SLAB ? count - lo : VK_SLAB;
        ZKCHK(vk_slab(k, k.n_io ? io_scalars + 32 * k.n_io * (size_t)lo : nullptr, proofs + stride * lo, c, ok + lo, status ? status + lo : nullptr, s));
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
    hipStream_t s = ctx().stream;
    auto k = std::make_unique<ResidentVk>();
    k->protocol = 0;
    k->n_io = n_io;
    uint8_t g2[384];
    memcpy(g2, gm, 192);
    memcpy(g2 + 192, d, 192);
    std::vector<uint8_t> v1, v2;
    ZKCHK(points_decode_two_lists(ltgm_io, n_io, g2, 2, "verify_point_checks", SUBGROUP_ENDO, k->key1, k->key2, v1, v2, s));
    const KeyDefect bad = groth16_key_defect(v1.data(), v2.data(), n_io);
    if (bad.verdict) ZK_FAIL(verdict_code(bad.verdict), bad.what);
    if (n_io) ZKCHK(short_bases_create(&k->io[0], CURVE_G1, k->key1.p, n_io, s));
    return vk_install(k, ab, s, handle);
}

int zk_pinocchio_vk_upload(const uint8_t* vk_g1, const uint8_t* vk_g2, size_t n_io, uint64_t* handle) {
    if (!vk_g1 || !vk_g2 || !handle) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_vk_upload: null argument");
    if (n_io > SHORT_BASES_MAX) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_vk_upload: a resident key holds at most 2^13 public inputs (zk_pinocchio_verify_many has no such limit)");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    auto k = std::make_unique<ResidentVk>();
    k->protocol = 1;
    k->n_io = n_io;
    std::vector<uint8_t> v1, v2;
    ZKCHK(points_decode_two_lists(vk_g1, 3 + 2 * n_io, vk_g2, 6 + n_io, "verify_point_checks", SUBGROUP_ENDO, k->key1, k->key2, v1, v2, s));
    const KeyDefect bad = pinocchio_key_defect(v1.data(), v2.data(), n_io);
    if (bad.verdict) ZK_FAIL(verdict_code(bad.verdict), bad.what);
    if (n_io) {
        ZKCHK(short_bases_create(&k->io[0], CURVE_G1, k->key1.as<uint8_t>() + 96 * 3, n_io, s));
        ZKCHK(short_bases_create(&k->io[1], CURVE_G1, k->key1.as<uint8_t>() + 96 * (3 + n_io), n_io, s));
        ZKCHK(short_bases_create(&k->io[2], CURVE_G2, k->key2.as<uint8_t>() + 192 * 6, n_io, s));
    }
    uint8_t gt_one[576];
    gt_one_bytes(gt_one);
    return vk_install(k, gt_one, s, handle);
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
    return vk_verify(handle, 0, io_scalars, proofs, count, ok, status);
}
int zk_pinocchio_verify_resident(uint64_t handle, const uint8_t* io_scalars, const uint8_t* proofs, uint32_t count, uint8_t* ok, int32_t* status) {
    return vk_verify(handle, 1, io_scalars, proofs, count, ok, status);
}
}
