// Resident MSM bases (include/zkmi355x.h: zk_bases_*, zk_msm_resident[_many]): a point list uploaded and checked ONCE, then multiplied by
// many scalar vectors -- G.apply_powers cs xis with the same xis again and again (src/lib/zk/curve.ml:112-118; sum_apply_powers,
// src/groth16/groth16.ml:116-121, calls it once per variable with the same list) and G.dot on the same key maps (curve.ml:94-103).
//
// A handle holds, built at upload and reused by every call (a call allocates nothing):
//   - the Pippenger bases of msm.hip over all n points (subgroup-checked, window tables at msm_auto_window(n, true), folded digits where legal)
//     and MAX_SORT_JOBS workspaces: products LONGER than short_max (and a lone short product on a short list, see res_run) run the existing sort -> accumulate
//     -> fix-up -> digit sums -> weight chain (msm_sort_accumulate_many / msm_reduce), up to four products per chain;
//   - a second, narrow table over the first min(n, short_max) points: SHORT_C = 5-bit signed digits, 51 folded windows (52 without the
//     subgroup check), 2^(c-1) = 16 buckets, entry [j * ns + i] = 2^(5 j) P_i in the 128-byte record layout of ec.cuh.  Size:
//     ns x 52 x 128 B for G1, x 256 B for G2 -- 54.5 MB / 109 MB at short_max = 2^13, 1.7 MB (G1, 256) / 0.85 MB (G2, 64) as shipped;
//   - one pinned host arena and its device twin, sized from n (resident_cap_scalars): [bytes out | flag | job descriptors | scalars].  One H2D copy carries the descriptors (with
//     zeroed completion counters), the zeroed scalar-range flag and the scalars of a batch of products; one D2H copy brings back the flag and
//     the encoded results.
//
// Short products (<= short_max scalars, all of a call's short products together, when it has two or more -- or one on a long list): TWO
// launches, no counting sort.
//   1 k_msm_short   one workgroup per (product, bucket b): its lanes stride over the product's (point, window) entries, recode the signed
//                   digit in place (msm_digits.cuh) and add +-T[j * ns + i] into a per-lane XYZZ accumulator when |digit| = b; an LDS tree
//                   sums the lanes, lane 0 multiplies by b (<= 4 doublings) and files b * B_b.  The workgroup that completes a product (agent-
//                   scope release / atomic ticket / acquire) checks the product's scalars against r and sums its 16 partials into one XYZZ point.
//   2 k_xyzz_to_bytes  (msm_points.hip) over every product of the batch, long ones included.
// short_max (per group) comes from the sweep of scripts/bench_msm_resident.py (profiles/msm_resident.json): the largest swept length at which
// the two-launch path beats the chain on the same handle for K = n products of length n.  It is a build constant (-DZK_RESIDENT_SHORT_MAX=k
// builds a variant for the sweep: 0 = every product long), reported by zk_bases_info; it is not an option.
#include "ec.cuh"
#include "handle_table.h"
#include "msm.cuh"
#include "msm_digits.cuh"

#include <memory>
#include <stdlib.h>
#include <string.h>

// short_max per group, from profiles/msm_resident.json (K = n products of length n in one call, ms per product, short path / chain):
// G1 n = 16: 0.037 / 0.104, 64: 0.028 / 0.105, 256: 0.072 / 0.131, 1024: 0.247 / 0.225;  G2 n = 16: 0.107 / 0.146, 64: 0.097 / 0.145, 256: 0.286 / 0.194.
// -DZK_RESIDENT_SHORT_MAX=k sets both (the sweep's variant libraries)
#ifdef ZK_RESIDENT_SHORT_MAX
#define ZK_RESIDENT_SHORT_MAX_G1 ZK_RESIDENT_SHORT_MAX
#define ZK_RESIDENT_SHORT_MAX_G2 ZK_RESIDENT_SHORT_MAX
#else
#define ZK_RESIDENT_SHORT_MAX_G1 256
#define ZK_RESIDENT_SHORT_MAX_G2 64
#endif

namespace zk {

static constexpr uint32_t RESIDENT_SHORT_MAX_G1 = ZK_RESIDENT_SHORT_MAX_G1, RESIDENT_SHORT_MAX_G2 = ZK_RESIDENT_SHORT_MAX_G2;
static_assert(RESIDENT_SHORT_MAX_G1 <= 8192 && RESIDENT_SHORT_MAX_G2 <= 8192, "short products: at most 2^13 scalars");
static constexpr uint32_t SHORT_C = 5;                     // window bits of the narrow table: 255 = 51 x 5, so folded digits need no carry window
static constexpr uint32_t SHORT_BUCKETS = 1u << (SHORT_C - 1);
static constexpr uint32_t SHORT_THREADS = 128;             // lanes per (product, bucket) workgroup: the LDS tree holds 128 raw XYZZ (32 / 64 KiB)
static constexpr uint32_t RESIDENT_MAX_JOBS = 256;         // products per batch (per H2D / D2H pair): 1 MiB (G1) / 2 MiB (G2) of bucket partials
// Scalars per batch: at least n (one product always fits), at most 64 full-length products and 2^18 scalars (8 MiB): a 16-point list stages
// 32 KiB, a 2^12-point one 8 MiB; K = n = 1024 products of length n run in 16 batches.
static inline uint64_t resident_cap_scalars(uint64_t n) {
    const uint64_t want = 64 * n < ((uint64_t)1 << 18) ? 64 * n : ((uint64_t)1 << 18);
    return n > want ? n : want;
}
// A LONE short product (the only one of its call): the short path costs about its length L, the chain over the zero-padded vector about the
// handle's n.  profiles/msm_resident.json: "short_pair_ms" G1 0.55 / 0.96 / 2.79 ms at L = 16 / 64 / 256, G2 1.58 / 2.98 ms at 16 / 64;
// a 16-scalar prefix on the chain ("prefix16_resident_ms", short_max 0 library) G1 1.08 / 2.02 ms at 2^16 / 2^20 points, G2 1.24 / 2.18 ms.
// It takes the short path when L * ratio < n: G1 L = 16 at 2^16 points 0.55 ms, at 2^20 0.54 ms; G2 L = 16 at 2^20 1.55 ms (plain run).  Set
// from those L = 16 points; near L = 2^19 / ratio the short path's cost (2.79 ms at L = 256 in G1) may pass the chain's, which is not measured.
static constexpr uint64_t LONE_RATIO_G1 = 2048, LONE_RATIO_G2 = 4096;

// One product of a batch, as the device sees it (16 B, in the H2D copy).  done: completion counter of k_msm_short (zero on arrival).
struct ResidentJob {
    uint32_t sc_off;       // first scalar (index into the batch's scalar block)
    uint32_t len;          // scalars
    uint32_t done;
    uint32_t pad;
};

// the narrow table's record -> the affine operand (canonical entries: -y = 2p - y)
FF_INLINE Aff<Fp> short_entry(const Fp*, const uint8_t* e, bool neg) {
    const TabRec r = tab_rec_load(e);
    Aff<Fp> a;
    a.x = tab_rec_x(r);
    if (neg) a.y = fe_neg(tab_rec_y(r));
    else a.y = tab_rec_y(r);
    return a;
}
FF_INLINE Aff<Fp2> short_entry(const Fp2*, const uint8_t* e, bool neg) {
    const Aff<Fp> a0 = short_entry((const Fp*)nullptr, e, neg), a1 = short_entry((const Fp*)nullptr, e + TAB_REC, neg);
    Aff<Fp2> a;
    a.x = {a0.x, a1.x};
    a.y = {a0.y, a1.y};
    return a;
}
// lanes [0, count) hold points in `lds` (raw layout); afterwards lane 0 holds their sum in `acc`.  count: a power of two <= blockDim.x
template <class F> FF_INLINE void lds_tree_sum(Xyzz<F>& acc, uint8_t* lds, uint32_t count) {
    constexpr int XB = RawLayout<F>::XYZZ;
    const uint32_t t = threadIdx.x;
    for (uint32_t s = count >> 1; s > 0; s >>= 1) {
        if (t < s) {
            const Xyzz<F> q = xyzz_load_raw<F>(lds + (uint64_t)XB * (t + s));
            xyzz_add(acc, q);
            xyzz_store_raw(lds + (uint64_t)XB * t, acc);
        }
        __syncthreads();
    }
}

template <class F>
__global__ __launch_bounds__(SHORT_THREADS) void k_msm_short(const uint8_t* __restrict__ table, DigitArgs da, ResidentJob* jobs,
                                                              const uint32_t* __restrict__ scalars, uint8_t* __restrict__ partial,
                                                              uint8_t* __restrict__ out_xyzz, int* __restrict__ flag) {
    constexpr int XB = RawLayout<F>::XYZZ;
    constexpr int ENTRY = TableLayout<F>::ENTRY;
    __shared__ __attribute__((aligned(16))) uint8_t lds[SHORT_THREADS * XB];
    const uint32_t t = threadIdx.x, bucket = blockIdx.x, nb = gridDim.x;
    const ResidentJob job = jobs[blockIdx.y];
    const uint32_t* sc = scalars + 8 * (uint64_t)job.sc_off;
    Xyzz<F> acc = xyzz_inf<F>();
    const uint64_t entries = (uint64_t)job.len * da.nw;
    for (uint64_t e = t; e < entries; e += SHORT_THREADS) {
        const uint32_t i = (uint32_t)(e / da.nw), j = (uint32_t)(e - (uint64_t)i * da.nw);
        uint32_t s[9], key, val;
        if (!digits_prepare(sc, i, da, s) || !digit_at(s, i, j, da, key, val) || key != bucket) continue;
        const Aff<F> q = short_entry((const F*)nullptr, table + (uint64_t)ENTRY * (val & 0x7fffffffu), (val >> 31) != 0);
        xyzz_madd(acc, q);
    }
    xyzz_store_raw(lds + (uint64_t)XB * t, acc);
    __syncthreads();
    lds_tree_sum(acc, lds, SHORT_THREADS);
    uint8_t* mine = partial + (uint64_t)XB * ((uint64_t)blockIdx.y * nb + bucket);
    if (t == 0) {
        // (bucket + 1) * B: double-and-add from the top bit of a 5-bit digit magnitude
        const uint32_t b = bucket + 1;
        Xyzz<F> r = acc;
        for (int k = 30 - __builtin_clz(b); k >= 0; k--) {
            r = xyzz_dbl(r);
            if (b >> k & 1) xyzz_add(r, acc);
        }
        xyzz_store_raw(mine, r);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // hand-off to the workgroup that completes the product: agent-scope release, ticket, agent-scope acquire (the partials of the other
    // buckets may have been written on another XCD)
    uint32_t* last = reinterpret_cast<uint32_t*>(lds);
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t prev = __hip_atomic_fetch_add(&jobs[blockIdx.y].done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last[0] = prev == nb - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!last[0]) return;
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    bool bad = false;
    for (uint32_t i = t; i < job.len; i += SHORT_THREADS) bad = bad || !fe_is_canonical(fe_load<FrParams>(sc + 8 * (uint64_t)i));
    if (bad) *flag = 1;
    acc = t < nb ? xyzz_load_raw<F>(partial + (uint64_t)XB * ((uint64_t)blockIdx.y * nb + t)) : xyzz_inf<F>();
    xyzz_store_raw(lds + (uint64_t)XB * t, acc);
    __syncthreads();
    lds_tree_sum(acc, lds, nb);
    if (t == 0) xyzz_store<F>(out_xyzz + (uint64_t)(XB / 4 * 3) * blockIdx.y, acc);     // dense XYZZ: 4 x 48 B (G1), 4 x 96 B (G2)
}
static_assert(RawLayout<Fp>::XYZZ / 4 * 3 == 192 && RawLayout<Fp2>::XYZZ / 4 * 3 == 384, "dense XYZZ = 3/4 of the raw layout");

// scalars >= r among n (the long products' zero-padded vectors)
__global__ void k_resident_check(const uint32_t* __restrict__ s, uint64_t n, int* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !fe_is_canonical(fe_load<FrParams>(s + 8 * i))) *flag = 1;
}

// ================================================================== host side
struct ResidentBases {
    Curve curve = CURVE_G1;
    uint64_t n = 0;
    MsmBases b;                               // all n points, window tables at msm_auto_window(n, true)
    MsmBases small;                           // the first ns points at SHORT_C bits (ns = 0: no short path)
    uint64_t ns = 0;
    uint64_t short_max = 0;
    DigitArgs da{};                           // recoding of the narrow table
    MsmWorkspace ws[MAX_SORT_JOBS];           // long products
    DevBuf pad[MAX_SORT_JOBS];                // their zero-padded scalar vectors (n x 32 B)
    uint32_t nws = 0;
    DevBuf xyzz;                              // RESIDENT_MAX_JOBS dense XYZZ results
    DevBuf partial;                           // RESIDENT_MAX_JOBS x 16 raw XYZZ bucket partials of the short kernel
    DevBuf arena;                             // [bytes out | flag | jobs | scalars]
    uint8_t* host = nullptr;                  // its pinned twin
    uint64_t cap_scalars = 0;
    size_t flag_off = 0;
    ~ResidentBases() {
        if (host) (void)hipHostFree(host);
    }
};

// its own range (handle_table.h): never the number of a key handle of either protocol, single- or multi-device, or of a verification key.
// Resident bases count as key handles: while one lives the device list stays (zk_set_device_list).
static HandleTable<ResidentBases>& g_res = *new HandleTable<ResidentBases>(HANDLES_RESIDENT_BASES, "unknown resident bases handle");
static void res_release() {
    if (!g_res.size()) return;
    DeviceScope ds(0);
    g_res.release_all();
}
static CleanupRegistrar g_res_cleanup(res_release);

static int res_lookup(uint64_t handle, ResidentBases** out) {
    if (!(*out = g_res.find(handle))) ZK_FAIL(ZK_ERR_HANDLE, g_res.unknown());
    return ZK_OK;
}

// wire: `points` holds wire bytes, 48 / 96 per point (zk_bases_upload_compressed)
static int res_upload(int group, const uint8_t* points, size_t n, uint64_t* handle, bool wire = false) {
    if (!handle || !points) ZK_FAIL(ZK_ERR_ARG, "zk_bases_upload: null argument");
    if (group != 0 && group != 1) ZK_FAIL(ZK_ERR_ARG, "zk_bases_upload: group must be 0 (G1) or 1 (G2)");
    if (n == 0) ZK_FAIL(ZK_ERR_ARG, "zk_bases_upload: empty point list");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    Ctx& c = ctx();
    hipStream_t s = c.stream;
    auto h = std::make_unique<ResidentBases>();
    ResidentBases& r = *h;
    r.curve = group == 0 ? CURVE_G1 : CURVE_G2;
    r.n = n;
    // the key uploads' checks (groth16.hip, pinocchio.hip): encoding, curve, [r] P = O unless ZK_KEY_SUBGROUP_CHECK=0 -- read here, once: the
    // handle keeps this verdict (without it no table folds)
    const bool chk = key_subgroup_check();
    if (wire) ZKCHK(msm_bases_from_wire(r.b, r.curve, points, n, msm_auto_window(n, true), true, s, chk));
    else ZKCHK(msm_bases_from_bytes(r.b, r.curve, points, n, msm_auto_window(n, true), true, s, chk));
    r.short_max = r.curve == CURVE_G1 ? RESIDENT_SHORT_MAX_G1 : RESIDENT_SHORT_MAX_G2;
    r.ns = n < r.short_max ? n : r.short_max;
    if (r.ns) {
        DevBuf dense;
        ZKCHK(dense.alloc(aff_bytes(r.curve) * r.ns));
        ZKCHK(msm_bases_dense(r.b, 0, r.ns, dense.p, s));
        ZKCHK(msm_bases_from_device_affine(r.small, r.curve, dense.p, r.ns, SHORT_C, true, s, chk));
        HIPCHK(hipStreamSynchronize(s));          // `dense` is released on return
        r.da = DigitArgs{r.ns, r.small.c, r.small.nw, 1u, SHORT_BUCKETS, {0, 0, 0, 0, 0, 0, 0, 0, 0}, r.small.ident.as<uint8_t>(), 0u, 0u, 0u, r.small.fold ? 1u : 0u};
        digit_constant(r.small.c, r.small.nw, r.da.K);
    }
    r.nws = MAX_SORT_JOBS;          // every length can take the chain: a lone short product does (res_run)
    for (uint32_t k = 0; k < r.nws; k++) {
        ZKCHK(msm_workspace_alloc(r.ws[k], r.b));
        ZKCHK(r.pad[k].alloc(32 * n));
    }
    const size_t ab = aff_bytes(r.curve);
    ZKCHK(r.xyzz.alloc(xyzz_bytes(r.curve) * RESIDENT_MAX_JOBS));
    ZKCHK(r.partial.alloc((size_t)(r.curve == CURVE_G1 ? RawLayout<Fp>::XYZZ : RawLayout<Fp2>::XYZZ) * SHORT_BUCKETS * RESIDENT_MAX_JOBS));
    r.cap_scalars = resident_cap_scalars(n);
    r.flag_off = ab * RESIDENT_MAX_JOBS;
    const size_t arena = r.flag_off + 16 + sizeof(ResidentJob) * RESIDENT_MAX_JOBS + 32 * r.cap_scalars;
    ZKCHK(r.arena.alloc(arena));
    HIPCHK(hipHostMalloc((void**)&r.host, arena, hipHostMallocDefault));
    HIPCHK(hipStreamSynchronize(s));
    *handle = g_res.add(std::move(h));
    return ZK_OK;
}

// One batch: jobs [0, nshort) short, [nshort, njobs) long, their scalars already in the pinned arena.  Leaves the encodings in r.host.
static int res_batch(ResidentBases& r, uint32_t njobs, uint32_t nshort, uint64_t nsc, int* bad) {
    Ctx& c = ctx();
    hipStream_t s = c.stream;
    const size_t ab = aff_bytes(r.curve), xb = xyzz_bytes(r.curve);
    const size_t jobs_off = r.flag_off + 16, sc_off = jobs_off + sizeof(ResidentJob) * njobs;
    uint8_t* d = r.arena.as<uint8_t>();
    const ResidentJob* hj = reinterpret_cast<const ResidentJob*>(r.host + jobs_off);
    memset(r.host + r.flag_off, 0, 16);
    HIPCHK(hipMemcpyAsync(d + r.flag_off, r.host + r.flag_off, sc_off + 32 * nsc - r.flag_off, hipMemcpyHostToDevice, s));
    int* d_flag = reinterpret_cast<int*>(d + r.flag_off);
    const uint32_t* d_sc = reinterpret_cast<const uint32_t*>(d + sc_off);
    if (nshort) {
        ScopedTimer t("msm_short", s);
        const dim3 grid(SHORT_BUCKETS, nshort);
        ResidentJob* d_jobs = reinterpret_cast<ResidentJob*>(d + jobs_off);
        if (r.curve == CURVE_G1)
            hipLaunchKernelGGL(k_msm_short<Fp>, grid, dim3(SHORT_THREADS), 0, s, (const uint8_t*)r.small.table.as<uint8_t>(), r.da, d_jobs, d_sc,
                               r.partial.as<uint8_t>(), r.xyzz.as<uint8_t>(), d_flag);
        else
            hipLaunchKernelGGL(k_msm_short<Fp2>, grid, dim3(SHORT_THREADS), 0, s, (const uint8_t*)r.small.table.as<uint8_t>(), r.da, d_jobs, d_sc,
                               r.partial.as<uint8_t>(), r.xyzz.as<uint8_t>(), d_flag);
        HIPCHK(hipGetLastError());
    }
    // long products: the existing chain, up to MAX_SORT_JOBS per chain, each over its zero-padded copy of the scalars (the tail adds nothing)
    for (uint32_t k = nshort; k < njobs; k += r.nws) {
        const uint32_t cnt = njobs - k < r.nws ? njobs - k : r.nws;
        MsmWorkspace* ws[MAX_SORT_JOBS];
        const void* sc[MAX_SORT_JOBS];
        void* outs[MAX_SORT_JOBS];
        for (uint32_t g = 0; g < cnt; g++) {
            const ResidentJob& j = hj[k + g];
            HIPCHK(hipMemcpyAsync(r.pad[g].p, d_sc + 8 * (uint64_t)j.sc_off, 32 * (size_t)j.len, hipMemcpyDeviceToDevice, s));
            if (j.len < r.n) HIPCHK(hipMemsetAsync(r.pad[g].as<uint8_t>() + 32 * (size_t)j.len, 0, 32 * (size_t)(r.n - j.len), s));
            hipLaunchKernelGGL(k_resident_check, grid_for(j.len, 256), dim3(256), 0, s, (const uint32_t*)r.pad[g].as<uint32_t>(), (uint64_t)j.len, d_flag);
            ws[g] = &r.ws[g];
            sc[g] = r.pad[g].p;
            outs[g] = r.xyzz.as<uint8_t>() + xb * (k + g);
        }
        ZKCHK(msm_sort_accumulate_many(r.b, ws, sc, cnt, s));
        ZKCHK(msm_reduce(r.b, ws, outs, cnt, s));
    }
    const size_t bytes_off = r.flag_off - ab * njobs;
    ZKCHK(points_xyzz_to_bytes_dev(r.curve, r.xyzz.p, njobs, d + bytes_off, s));
    HIPCHK(hipMemcpyAsync(r.host + bytes_off, d + bytes_off, ab * njobs + 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *bad = *reinterpret_cast<const int*>(r.host + r.flag_off);
    return ZK_OK;
}

// count products; product k = the first lens[k] points times scalars[off_k, off_k + lens[k]) -- off_k the running sum of lens
static int res_run(uint64_t handle, const uint8_t* scalars, const uint64_t* lens, uint32_t count, uint8_t* out) {
    ResidentBases* rp;
    ZKCHK(res_lookup(handle, &rp));
    ResidentBases& r = *rp;
    if (count && (!lens || !out)) ZK_FAIL(ZK_ERR_ARG, "msm_resident: null argument");
    uint64_t total = 0;
    for (uint32_t k = 0; k < count; k++) {
        if (lens[k] > r.n) ZK_FAIL(ZK_ERR_APPLY_POWERS, "apply_powers");      // curve.ml:116, before anything runs
        total += lens[k];
    }
    if (total && !scalars) ZK_FAIL(ZK_ERR_ARG, "msm_resident: null scalars");
    // The short path pays off in batches: its per-product tail (a 7-level LDS tree of single-lane XYZZ additions, <= 4 doublings, a 4-level
    // tree) is serial, and a LONE product waits for all of it, while the chain's cost follows the handle's n whatever the product's length.
    // So a call with one short product runs it on the chain unless the list is long against it (LONE_RATIO_*).
    uint32_t nshort_call = 0;
    uint64_t lone_len = 0;
    for (uint32_t q = 0; q < count; q++)
        if (lens[q] && lens[q] <= r.short_max) { nshort_call++; lone_len = lens[q]; }
    const uint64_t ratio = r.curve == CURVE_G1 ? LONE_RATIO_G1 : LONE_RATIO_G2;
    const uint64_t short_max = nshort_call >= 2 || (nshort_call == 1 && lone_len * ratio < r.n) ? r.short_max : 0;
    DeviceScope ds(0);
    const size_t ab = aff_bytes(r.curve);
    std::vector<uint32_t> order;              // the products of the current batch: short ones first
    std::vector<uint64_t> offs(count);
    uint64_t run = 0;
    for (uint32_t q = 0; q < count; q++) { offs[q] = run; run += lens[q]; }
    uint32_t k = 0;
    int bad_any = 0;
    while (k < count) {
        // fill a batch: at most RESIDENT_MAX_JOBS products and cap_scalars scalars (one product of <= n scalars always fits)
        std::vector<uint32_t> shorts, longs;
        uint64_t nsc = 0;
        for (; k < count; k++) {
            if (lens[k] == 0) {                                            // curve.ml:115: zero
                memset(out + ab * k, 0, ab);
                out[ab * k] = 0x40;
                continue;
            }
            if (shorts.size() + longs.size() == RESIDENT_MAX_JOBS || nsc + lens[k] > r.cap_scalars) break;
            (lens[k] <= short_max ? shorts : longs).push_back(k);
            nsc += lens[k];
        }
        order = shorts;
        order.insert(order.end(), longs.begin(), longs.end());
        if (order.empty()) break;
        const uint32_t njobs = (uint32_t)order.size();
        ResidentJob* hj = reinterpret_cast<ResidentJob*>(r.host + r.flag_off + 16);
        uint8_t* hsc = r.host + r.flag_off + 16 + sizeof(ResidentJob) * njobs;
        uint64_t o = 0;
        for (uint32_t q = 0; q < njobs; q++) {
            const uint32_t p = order[q];
            hj[q] = ResidentJob{(uint32_t)o, (uint32_t)lens[p], 0u, 0u};
            memcpy(hsc + 32 * o, scalars + 32 * offs[p], 32 * (size_t)lens[p]);
            o += lens[p];
        }
        int bad = 0;
        ZKCHK(res_batch(r, njobs, (uint32_t)shorts.size(), nsc, &bad));
        if (bad) bad_any = 1;
        const uint8_t* hb = r.host + r.flag_off - ab * njobs;
        for (uint32_t q = 0; q < njobs; q++) memcpy(out + ab * order[q], hb + ab * q, ab);
    }
    if (bad_any) ZK_FAIL(ZK_ERR_SCALAR_RANGE, "msm_resident: scalar >= r");
    return ZK_OK;
}

// ---- the short path alone, on device buffers (verify_resident.hip: a verification key's IO points, one product per proof)
// A narrow table over ALL n points (n <= SHORT_BASES_MAX), built from dense affine points that are already on the device and already known to lie in the
// subgroup.  No pinned arena, no chain, no host copy: scalars in, dense XYZZ out, both in device memory; nothing here waits for the stream.
struct ShortBases {
    Curve curve = CURVE_G1;
    uint64_t n = 0;
    MsmBases small;
    DigitArgs da{};
    DevBuf jobs, partial, flag;               // SHORT_BASES_CHUNK jobs at most per launch; grown on demand
    uint32_t cap_jobs = 0;
};
static constexpr uint32_t SHORT_BASES_CHUNK = 4096;          // products per launch (blockIdx.y): 16 / 32 MiB of bucket partials
// job i of a launch: the n scalars from i stride + first of the launch's block, none when live[i] == 0 (the product is then the identity, its scalars unread)
__global__ void k_short_jobs(ResidentJob* jobs, const uint8_t* __restrict__ live, uint32_t count, uint32_t n, uint32_t stride, uint32_t first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    jobs[i] = ResidentJob{i * stride + first, live[i] ? n : 0u, 0u, 0u};
}
int short_bases_create(ShortBases** out, Curve curve, const void* d_affine, uint64_t n, hipStream_t s) {
    if (n == 0 || n > SHORT_BASES_MAX) ZK_FAIL(ZK_ERR_ARG, "short bases: 1 .. 2^13 points");
    auto h = std::make_unique<ShortBases>();
    h->curve = curve;
    h->n = n;
    ZKCHK(msm_bases_from_device_affine(h->small, curve, d_affine, n, SHORT_C, true, s, true));
    h->da = DigitArgs{n, h->small.c, h->small.nw, 1u, SHORT_BUCKETS, {0, 0, 0, 0, 0, 0, 0, 0, 0}, h->small.ident.as<uint8_t>(), 0u, 0u, 0u, h->small.fold ? 1u : 0u};
    digit_constant(h->small.c, h->small.nw, h->da.K);
    ZKCHK(h->flag.alloc(16));
    *out = h.release();
    return ZK_OK;
}
void short_bases_free(ShortBases* b) { delete b; }
int short_bases_run(ShortBases& b, const uint32_t* d_scalars, const uint8_t* d_live, uint32_t count, uint64_t stride, uint64_t first, uint8_t* d_out_xyzz, hipStream_t s) {
    // ResidentJob::sc_off has 32 bits: a launch's last job begins below per * stride
    if (first + b.n > stride || stride > UINT32_MAX) ZK_FAIL(ZK_ERR_ARG, "short bases: the products' scalars lie outside a stride of 32 bits");
    const uint32_t fit = (uint32_t)(UINT32_MAX / stride), per = fit < SHORT_BASES_CHUNK ? fit : SHORT_BASES_CHUNK;
    const uint32_t want = count < per ? count : per;
    if (want > b.cap_jobs) {
        HIPCHK(hipStreamSynchronize(s));          // the buffers about to go may still be read
        ZKCHK(b.jobs.alloc(sizeof(ResidentJob) * (size_t)want));
        ZKCHK(b.partial.alloc((size_t)(b.curve == CURVE_G1 ? RawLayout<Fp>::XYZZ : RawLayout<Fp2>::XYZZ) * SHORT_BUCKETS * want));
        b.cap_jobs = want;
    }
    const size_t xb = xyzz_bytes(b.curve);
    ScopedTimer t("msm_short", s);
    for (uint32_t k = 0; k < count; k += per) {
        const uint32_t cnt = count - k < per ? count - k : per;
        hipLaunchKernelGGL(k_short_jobs, grid_for(cnt, 256), dim3(256), 0, s, b.jobs.as<ResidentJob>(), d_live + k, cnt, (uint32_t)b.n, (uint32_t)stride, (uint32_t)first);
        const dim3 grid(SHORT_BUCKETS, cnt);
        const uint32_t* sc = d_scalars + 8 * stride * k;
        if (b.curve == CURVE_G1)
            hipLaunchKernelGGL(k_msm_short<Fp>, grid, dim3(SHORT_THREADS), 0, s, (const uint8_t*)b.small.table.as<uint8_t>(), b.da, b.jobs.as<ResidentJob>(), sc,
                               b.partial.as<uint8_t>(), d_out_xyzz + xb * k, b.flag.as<int>());
        else
            hipLaunchKernelGGL(k_msm_short<Fp2>, grid, dim3(SHORT_THREADS), 0, s, (const uint8_t*)b.small.table.as<uint8_t>(), b.da, b.jobs.as<ResidentJob>(), sc,
                               b.partial.as<uint8_t>(), d_out_xyzz + xb * k, b.flag.as<int>());
        HIPCHK(hipGetLastError());
    }
    return ZK_OK;
}

}  // namespace zk

using namespace zk;
extern "C" {
int zk_bases_upload(int group, const uint8_t* points, size_t n, uint64_t* handle) { return res_upload(group, points, n, handle); }
int zk_bases_upload_compressed(int group, const uint8_t* points, size_t n, uint64_t* handle) { return res_upload(group, points, n, handle, true); }
int zk_bases_info(uint64_t handle, int* group, uint64_t* n, uint64_t* short_max) {
    ResidentBases* r;
    ZKCHK(res_lookup(handle, &r));
    if (group) *group = r->curve == CURVE_G1 ? 0 : 1;
    if (n) *n = r->n;
    if (short_max) *short_max = r->short_max;
    return ZK_OK;
}
int zk_bases_free(uint64_t handle) {
    if (!g_res.find(handle)) ZK_FAIL(ZK_ERR_HANDLE, g_res.unknown());
    DeviceScope ds(0);
    (void)hipStreamSynchronize(ctx().stream);
    g_res.take(handle);
    return ZK_OK;
}
int zk_msm_resident(uint64_t handle, const uint8_t* scalars, size_t nscalars, uint8_t* out) {
    if (!out) ZK_FAIL(ZK_ERR_ARG, "msm_resident: null output");
    const uint64_t len = nscalars;
    return res_run(handle, scalars, &len, 1, out);
}
int zk_msm_resident_many(uint64_t handle, const uint8_t* scalars, const uint64_t* lens, uint32_t count, uint8_t* out) {
    return res_run(handle, scalars, lens, count, out);
}
}
