// Pippenger multi-scalar multiplication over BLS12-381 G1 / G2 for gfx950.
//
// Computes the same group element as the reference's left folds of single scalar
// multiplications: G.apply_powers (src/lib/zk/curve.ml:112-118), G.dot / sum_map (:91-103).
//
// MI355X-first pipeline (all integer work; no MFMA):
//   1 count    scalars (32 B, coalesced) -> signed c-bit digits -> histogram of bucket ids
//   2 scan     exclusive prefix sum of the histogram (bucket -> start of its run)
//   3 scatter  point references (index | sign) written bucket-contiguously: a counting sort
//   4 accumulate  the sorted run is cut into equal chunks, one per lane: every lane does the same
//              number of mixed additions XYZZ += affine regardless of the digit distribution
//              (no per-bucket load imbalance); runs inside a chunk go straight to their bucket,
//              runs cut by a chunk border go to per-lane head / tail slots
//   5 fixup    one lane per bucket adds the few border partials of its run
//   6 reduce   sum_b (b+1) * B_b by per-lane running sums over 2^k-bucket slices + one small
//              scalar multiple per slice, then a wave-shuffle-free LDS tree per window
//   7 final    Horner over the windows (classic mode) -> one XYZZ point
// With `precomp` the base table holds 2^(c*j) * P_i for every window j (HBM is 288 GB: a 2^22
// Groth16 key costs 32 GB), all windows share ONE bucket set and step 7's 255 serial doublings
// disappear; this is the mode the resident proving key uses.
//
// Translation units (round 5 split the 1 400 lines this file had grown to): msm_points.hip -- encodings, the checks of incoming points, the window
// tables, fixed-base products; msm_sort.hip -- steps 1-3; msm_acc_g1.hip / msm_acc_g2.hip / msm_acc_g2i.hip -- step 4; msm_red.hip and msm_tail.hip --
// steps 5-7; msm_ba.hip -- the optional batch-affine rounds.  Here: workspaces, the dispatch of a product through those steps, and the C-ABI's
// zk_msm_g1/g2, zk_g1/g2_of_fr, zk_g1/g2_powers.
#include "ec.cuh"
#include "msm.cuh"
#include "msm_tail.cuh"

#include <stdlib.h>
#include <string.h>
#include <string>
#include <type_traits>

namespace zk {

// ------------------------------------------------------------------ accumulate: msm_acc_g1.hip / msm_acc_g2.hip; fix-up of the chunk partials and
// digit sums of the bucket reduction (one lane, or lane pair, per point): msm_red.hip -- a translation unit of its own, with the field products
// expanded in place
static constexpr uint32_t BA_FINISH_CHUNK = 8;       // sorted entries per lane of the XYZZ accumulate that follows the batch-affine rounds

// Work counters of one product's accumulate launch (profiling level 2 only: bench.py's ALU model counts the additions that really run).
// out[0] = sorted entries, out[1] = non-empty buckets, out[2] = runs that start on a chunk border, out[3] = runs that start on step 1 of a chunk.
__global__ void k_acc_stats(const uint32_t* __restrict__ offsets, uint32_t nb, uint32_t chunk, unsigned long long* __restrict__ out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) atomicAdd(&out[0], (unsigned long long)offsets[nb]);
    if (k >= nb) return;
    const uint32_t s = offsets[k], e = offsets[k + 1];
    if (e == s) return;
    atomicAdd(&out[1], 1ull);
    if (s % chunk == 0) atomicAdd(&out[2], 1ull);
    if (s % chunk == 1) atomicAdd(&out[3], 1ull);
}

// ================================================================== host side

uint32_t msm_auto_window(uint64_t n, bool precomp) {
    // work ~ nw * n additions + buckets * (2 reduce additions); pick the c minimizing it, capped so the
    // accumulate pass still has >= ~128k lanes of work
    double best = 1e300;
    uint32_t bc = 8;
    // resident keys: at most 2^15 buckets, so the whole histogram of the counting sort fits in LDS
    const uint32_t cmax = precomp ? 16 : 20;
    for (uint32_t c = 6; c <= cmax; c++) {
        double nw = msm_windows(c);          // the plain count: the choice per size stays the measured one (a folded width then runs with one window fewer)
        double buckets = (precomp ? 1.0 : nw) * (double)(1u << (c - 1));
        double cost = nw * (double)n + 3.0 * buckets;
        if (cost < best) { best = cost; bc = c; }
    }
    return bc;
}

// Batch-affine rounds before the XYZZ accumulate: halve the runs until ~2-3 entries per bucket are left (uniform digits; the
// XYZZ finisher takes whatever a skewed bucket still holds).  Resident keys only (one bucket set).
static uint32_t ba_rounds_for(const MsmBases& b, uint32_t nbuckets) {
    if (!b.precomp) return 0;
    // ZK_MSM_BA_ROUNDS: 0 = off, k > 0 = exactly k rounds (tests, experiments), unset = auto for the curves ZK_MSM_BA_CURVES names
    // (bit 0: G1, bit 1: G2).  Default: none -- measured on MI355X: the rounds re-read what they add from HBM, ~1 KB
    // per G1 addition in round 0 (two random 128-byte-line gathers of each table entry), and lose to the register-resident XYZZ
    // accumulate for G1; for G2 they break even.  Read per workspace, not cached: tests switch it.
    const int forced = opt_int(OPT_MSM_BA_ROUNDS, -1);
    if (forced == 0) return 0;
    if (forced > 0) return forced > 24 ? 24 : (uint32_t)forced;
    const int curves = opt_int(OPT_MSM_BA_CURVES, 0);
    if (!(curves & (b.curve == CURVE_G1 ? 1 : 2))) return 0;
    const uint64_t mean = b.n * b.nw / nbuckets;
    uint32_t r = 0;
    while (((uint64_t)8 << r) <= mean) r++;                 // mean in [8, 16) -> 1 round ... [2^(k+2), 2^(k+3)) -> k rounds
    return r > 24 ? 24 : r;
}
int msm_workspace_alloc(MsmWorkspace& w, const MsmBases& b, uint64_t max_nonzero, uint64_t launch_entries) {
    w.curve = b.curve; w.c = b.c; w.nw = b.nw; w.precomp = b.precomp; w.cap_points = b.n;
    const uint32_t nbw = 1u << (b.c - 1);
    w.nbuckets = (b.precomp ? 1 : b.nw) * nbw;
    const uint64_t maxN = b.n * b.nw;
    // >= 2 waves per SIMD when there is enough work; chunks of at least 16 entries (with a dozen proofs in flight the
    // chip is full anyway, and every chunk boundary costs a partial sum to store and to fix up: 8 -> 16 is +2.5 % proofs/s
    // at 2^16, 16..24 measure the same, 32 and up lose to the tail of the longest chunk)
    const uint64_t target_threads = opt_u64(OPT_MSM_TARGET_THREADS, 256 * 1024);   // tuning knob
    uint32_t chunk = (uint32_t)((maxN + target_threads - 1) / target_threads);
    const uint32_t chunk_min = (uint32_t)opt_int(OPT_MSM_CHUNK_MIN, 16);   // tuning knob
    if (launch_entries && chunk >= 64) {            // short chunks (small keys) already fill whole rounds: at 2^16, 2 rounds of 16-entry chunks beat 1 round of 32; 48 instead of 64 (the G2 product of a 2^20 key: one round of 208 instead of four of 52) measures the same
        // The caller knows how many sorted entries ONE accumulate launch carries (several products over these bases, e.g. Groth16's A and C):
        // cut it into a WHOLE number of rounds of the chip's resident lanes (256 CUs x 4 SIMDs x ACC_WAVES_G1 = ACC_WAVES_G2 = 2 waves x 64 lanes, half as many
        // chunks for the lane pairs of G2).  Every lane does the same number of additions, so a launch whose chunks fill 2.65 rounds costs three (2^20
        // constraints: 157 entries per chunk by the rule above; 208 makes it two rounds).
        const uint64_t round = b.curve == CURVE_G1 ? (uint64_t)256 * 4 * ACC_WAVES_G1 * 64 : (uint64_t)256 * 4 * ACC_WAVES_G2 * 64 / 2;
        const uint64_t k = (launch_entries + round * 208 - 1) / (round * 208);          // rounds, chunks of at most ~208 entries
        const uint64_t c2 = (launch_entries + k * round - 1) / (k * round);
        if (c2 > chunk_min) chunk = (uint32_t)c2;
        else chunk = chunk_min;
    }
    if (chunk < chunk_min) chunk = chunk_min;
    w.chunk = chunk;
    w.nthreads = (maxN + chunk - 1) / chunk;
    const size_t XB = b.curve == CURVE_G1 ? RawLayout<Fp>::XYZZ : RawLayout<Fp2>::XYZZ;      // intermediate points: raw layout
    ZKCHK(w.counts.alloc(4 * (size_t)(w.nbuckets + 1)));
    ZKCHK(w.offsets.alloc(4 * (size_t)(w.nbuckets + 1)));
    ZKCHK(w.cursor.alloc(4 * (size_t)(w.nbuckets + 1)));
    ZKCHK(w.sorted.alloc(4 * (size_t)maxN));
    w.sort_wgs = 0;
    w.sort_fine_bits = 0;
    static constexpr uint32_t COARSE_BINS = 512;
    // Two levels from 2^15 buckets and 2^20 (scalar, window) pairs up.  Above 2^15 buckets the histogram does not fit LDS; AT 2^15 it does (the
    // single-level sort below), but its 128 KiB per workgroup evict the accumulate workgroups of the other proofs in flight from every compute unit
    // the sort runs on: two levels (2 KiB + 20 KiB of LDS) measure +1.6 % proofs/s at 2^16, +1.9 % at 2^18 with the same single-proof latency.
    // ZK_SORT_TWO_LEVEL=0: never (A/B; above 2^15 buckets that is the global-atomic sort); ZK_SORT_TWO_LEVEL_MIN: log2 of the pair threshold.
    const int two_level = opt_int(OPT_SORT_TWO_LEVEL, 1);
    const int two_level_min = opt_int(OPT_SORT_TWO_LEVEL_MIN, w.nbuckets > 2 * SORT_MAX_BUCKETS ? 22 : 20);          // 2^16 buckets (c = 17) sort in two levels from 2^20 pairs like 2^15
    if (b.precomp && w.nbuckets >= SORT_MAX_BUCKETS && w.nbuckets / COARSE_BINS <= SORT_MAX_FINE && maxN >= ((uint64_t)1 << two_level_min) && two_level != 0) {
        w.sort_fine_bits = ceil_log2(w.nbuckets / COARSE_BINS);
        uint64_t wgs = maxN / (4 * (uint64_t)COARSE_BINS);
        w.sort_wgs = (uint32_t)(wgs > 256 ? 256 : wgs < 1 ? 1 : wgs);          // < 1: only when ZK_SORT_TWO_LEVEL_MIN forces the two levels on a handful of pairs
        ZKCHK(w.wgcount.alloc(4 * (size_t)COARSE_BINS * w.sort_wgs));
        ZKCHK(w.sorted2.alloc(8 * (size_t)maxN));
        ZKCHK(w.coarse.alloc(4 * (size_t)3 * (COARSE_BINS + 1)));
    } else if (b.precomp && w.nbuckets <= SORT_MAX_BUCKETS) {
        // every workgroup zeroes and flushes nbuckets counters: give it >= 4 pairs per counter to amortise that
        uint64_t wgs = maxN / (4 * (uint64_t)w.nbuckets);
        if (wgs > 256) wgs = 256;
        // tuning knob.  With scalar-major passes 8 workgroups already beat the global atomics (2^16: 37.3 -> 38.7-39.4 M constraints/s, the
        // sort 0.61 -> 0.45 ms per proof; below 8 -- pools of 2^14 constraints -- the global path wins: 23.6 M against 22.3-22.6); it was 64
        // with window-major passes
        const uint64_t min_wgs = opt_u64(OPT_SORT_MIN_WGS, 8);
        if (wgs >= min_wgs) {                               // below that too few workgroups: the global-atomic path is cheaper
            w.sort_wgs = (uint32_t)wgs;
            ZKCHK(w.wgcount.alloc(4 * (size_t)w.nbuckets * wgs));
        }
    }
    w.ba_rounds = ba_rounds_for(b, w.nbuckets);
    w.red_offsets = w.offsets.as<uint32_t>();
    w.red_chunk = w.chunk;
    uint64_t part_slots = w.nthreads;
    if (w.ba_rounds) {
        const uint64_t nz = max_nonzero && max_nonzero < b.n ? max_nonzero : b.n;
        w.ba_max_entries = nz * b.nw;
        const size_t PB = 2 * (b.curve == CURVE_G1 ? RawLayout<Fp>::ELEM : RawLayout<Fp2>::ELEM);
        w.ba_cap[0] = (w.ba_max_entries >> 1) + w.nbuckets;
        w.ba_cap[1] = (w.ba_max_entries >> 2) + w.nbuckets;
        ZKCHK(w.ba_offs.alloc(4 * (size_t)w.ba_rounds * (w.nbuckets + 1)));
        ZKCHK(w.ba_e[0].alloc(PB * w.ba_cap[0]));
        if (w.ba_rounds > 1) ZKCHK(w.ba_e[1].alloc(PB * w.ba_cap[1]));
        // the finisher works on what R rounds leave: short chunks (a few entries per bucket), one partial slot per chunk
        const uint64_t left = (w.ba_max_entries >> w.ba_rounds) + w.nbuckets;
        const uint64_t fin_threads = (left + BA_FINISH_CHUNK - 1) / BA_FINISH_CHUNK;
        if (fin_threads > part_slots) part_slots = fin_threads;
    }
    ZKCHK(w.buckets.alloc(XB * w.nbuckets));
    ZKCHK(w.head.alloc(XB * part_slots));
    ZKCHK(w.tail.alloc(XB * part_slots));
    ZKCHK(w.worklist.alloc(4 * (size_t)(w.nbuckets + 1)));
    const DigitPlan dp = digit_plan(b.c);
    ZKCHK(w.red.alloc(XB * (size_t)(dp.nd0 + dp.nd1) * (b.precomp ? 1 : b.nw)));
    ZKCHK(w.wsum.alloc(XB * tail_wsum_points(dp, b.precomp ? 1 : b.nw)));        // block sums of the weighting step (msm_tail.cuh)
    return ZK_OK;
}

// Steps 1-4 for `count` MSMs over the same bases: digits, counting sort, bucket accumulation (leaves raw bucket sums and
// chunk partials in the workspaces).  One chain of launches for all of them.
int msm_sort_accumulate_many(const MsmBases& b, MsmWorkspace* const* ws, const void* const* d_scalars, uint32_t count, hipStream_t s) {
    ZKCHK(msm_sort_launch(b, ws, d_scalars, count, s));          // msm_sort.hip: validates the batch (1..4 MSMs, matching workspaces)
    return msm_accumulate_sorted(b, ws, ws, count, s);
}
// Step 4 for `count` MSMs over the same bases: the bucket accumulation over sorted references.  from[i]: the workspace whose sort product i reads --
// ws[i] itself, or that of ANOTHER product with the same scalar vector over a base set of the same geometry (point count, window plan, identity
// flags, chunk length): Pinocchio's pools vv / vav, yy / yay, ww / waw carry the same scalars (pinocchio.ml:438-447,489-498) and sort them once.
int msm_accumulate_sorted(const MsmBases& b, MsmWorkspace* const* ws, MsmWorkspace* const* from, uint32_t count, hipStream_t s) {
    if (count == 0 || count > MAX_ACC_JOBS) ZK_FAIL(ZK_ERR_ARG, "msm_accumulate_sorted: 1..4 MSMs per batch");
    AccJobs aj{};
    for (uint32_t i = 0; i < count; i++) {
        MsmWorkspace& w = *ws[i];
        const MsmWorkspace& f = *from[i];
        if (w.c != b.c || w.precomp != b.precomp || w.curve != b.curve || w.cap_points < b.n || w.nbuckets != ws[0]->nbuckets || w.chunk != ws[0]->chunk ||
            f.c != w.c || f.nw != w.nw || f.precomp != w.precomp || f.cap_points != w.cap_points || f.nbuckets != w.nbuckets || f.chunk != w.chunk || f.nthreads != w.nthreads)
            ZK_FAIL(ZK_ERR_ARG, "msm: workspace does not match bases");
        if (&f != &w && (w.ba_rounds || f.ba_rounds)) ZK_FAIL(ZK_ERR_ARG, "msm: a shared sort does not combine with batch-affine rounds");
        aj.offsets[i] = f.offsets.as<uint32_t>(); aj.sorted[i] = f.sorted.as<uint32_t>();
        aj.buckets[i] = w.buckets.as<uint8_t>(); aj.head[i] = w.head.as<uint8_t>(); aj.tail[i] = w.tail.as<uint8_t>();
    }
    MsmWorkspace& w = *ws[0];
    uint32_t rounds = w.ba_rounds;
    for (uint32_t i = 0; i < count; i++)
        if (ws[i]->ba_rounds < rounds) rounds = ws[i]->ba_rounds;
    {
        // the whole bucket-accumulation stage of the batch (batch-affine rounds + the XYZZ accumulate) is ONE timed family span
        ScopedTimer t(b.curve == CURVE_G1 ? "msm_accumulate_g1" : "msm_accumulate_g2", s, 1);
        if (rounds) {
            ZKCHK(msm_batch_affine_rounds(b, ws, count, rounds, s));
            uint64_t max_entries = 0;
            for (uint32_t i = 0; i < count; i++) {
                MsmWorkspace& wi = *ws[i];
                wi.red_offsets = wi.ba_offs.as<uint32_t>() + (uint64_t)(rounds - 1) * (w.nbuckets + 1);
                wi.red_chunk = BA_FINISH_CHUNK;
                aj.offsets[i] = wi.red_offsets;
                aj.pts[i] = wi.ba_e[(rounds - 1) & 1].as<uint8_t>();
                if (wi.ba_max_entries > max_entries) max_entries = wi.ba_max_entries;
            }
            const uint64_t left = (max_entries >> rounds) + w.nbuckets;
            ZKCHK(msm_accumulate_launch(b.curve, (left + BA_FINISH_CHUNK - 1) / BA_FINISH_CHUNK, b.table.p, aj, count, w.nbuckets, BA_FINISH_CHUNK, s, true));
        } else {
            for (uint32_t i = 0; i < count; i++) { ws[i]->red_offsets = from[i]->offsets.as<uint32_t>(); ws[i]->red_chunk = ws[i]->chunk; }
            ZKCHK(msm_accumulate_launch(b.curve, w.nthreads, b.table.p, aj, count, w.nbuckets, w.chunk, s));
        }
    }
    if (ctx().profiling >= 2 && !rounds) {
        // what the launch really did (un-overlapped measurement pass only: this synchronises): chunks = lanes that ran, copies = first entries of a
        // chunk or of a run (no product), second steps = the 6-product addition of two affine points, everything else a full mixed addition
        DevBuf st;
        ZKCHK(st.alloc(32));
        unsigned long long h[4], tot[4] = {0, 0, 0, 0}, chunks = 0;
        for (uint32_t i = 0; i < count; i++) {
            HIPCHK(hipMemsetAsync(st.p, 0, 32, s));
            hipLaunchKernelGGL(k_acc_stats, grid_for(w.nbuckets, 256), dim3(256), 0, s, (const uint32_t*)from[i]->offsets.as<uint32_t>(), w.nbuckets, w.chunk, st.as<unsigned long long>());
            HIPCHK(hipMemcpyAsync(h, st.p, 32, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (int q = 0; q < 4; q++) tot[q] += h[q];
            chunks += (h[0] + w.chunk - 1) / w.chunk;
        }
        const char* f = b.curve == CURVE_G1 ? "msm_accumulate_g1" : "msm_accumulate_g2";
        const unsigned long long copies = chunks + tot[1] - tot[2], second = chunks > tot[3] ? chunks - tot[3] : 0;
        profile_count((std::string(f) + ":entries").c_str(), tot[0]);
        profile_count((std::string(f) + ":copies").c_str(), copies);
        profile_count((std::string(f) + ":second_steps").c_str(), second);
        profile_count((std::string(f) + ":full_additions").c_str(), tot[0] > copies + second ? tot[0] - copies - second : 0);
    }
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
int msm_sort_accumulate(const MsmBases& b, MsmWorkspace& w, const void* d_scalars, hipStream_t s) {
    MsmWorkspace* ws[1] = {&w};
    const void* sc[1] = {d_scalars};
    return msm_sort_accumulate_many(b, ws, sc, 1, s);
}
// Steps 5-7 for a batch of MSMs in one chain of launches: n1 products in G1 (bases b1) and n2 in G2 (bases b2), all with
// the same window plan.  outs[i]: one dense XYZZ point each.
int msm_reduce_mixed(const MsmBases* b1, MsmWorkspace* const* ws1, void* const* outs1, uint32_t n1,
                     const MsmBases* b2, MsmWorkspace* const* ws2, void* const* outs2, uint32_t n2, hipStream_t s) {
    if (n1 + n2 == 0 || n1 + n2 > MAX_TAIL_JOBS) ZK_FAIL(ZK_ERR_ARG, "msm_reduce: 1..8 MSMs per batch");
    const MsmBases& b = n1 ? *b1 : *b2;
    if (n1 && n2 && (b1->c != b2->c || b1->nw != b2->nw || b1->precomp != b2->precomp)) ZK_FAIL(ZK_ERR_ARG, "msm_reduce: one window plan per batch");
    const uint32_t nwin = b.precomp ? 1 : b.nw;
    TailJobs jobs{};
    jobs.n1 = n1;
    uint64_t max_lanes = 0, max_chunks = 0;
    uint32_t max_nb = 0;
    for (uint32_t i = 0; i < n1 + n2; i++) {
        MsmWorkspace& w = i < n1 ? *ws1[i] : *ws2[i - n1];
        const MsmBases& bi = i < n1 ? *b1 : *b2;
        if (w.c != bi.c || w.precomp != bi.precomp || w.curve != bi.curve || bi.curve != (i < n1 ? CURVE_G1 : CURVE_G2))
            ZK_FAIL(ZK_ERR_ARG, "msm_reduce: workspace does not match its bases");
        jobs.j[i] = TailJob{w.red_offsets, w.buckets.as<uint8_t>(), w.head.as<uint8_t>(), w.tail.as<uint8_t>(), w.worklist.as<uint32_t>(),
                            w.red.as<uint8_t>(), w.wsum.as<uint8_t>(), (uint8_t*)(i < n1 ? outs1[i] : outs2[i - n1]), w.nbuckets, w.red_chunk};
        HIPCHK(hipMemsetAsync(w.worklist.p, 0, 4, s));
        const uint64_t lanes = (uint64_t)w.nbuckets * (i < n1 ? 1 : 2);
        if (lanes > max_lanes) max_lanes = lanes;
        if (w.nbuckets > max_nb) max_nb = w.nbuckets;
        const uint64_t chunks = w.red_chunk == w.chunk ? w.nthreads : ~(uint64_t)0;      // after batch-affine rounds the chunk count is not the workspace's: per bucket
        if (chunks > max_chunks) max_chunks = chunks;
    }
    const uint32_t count = n1 + n2;
    const char* fam = n2 == 0 ? "msm_reduce_g1" : (n1 == 0 ? "msm_reduce_g2" : "msm_reduce");
    ScopedTimer t(fam, s);
    const DigitPlan dp = digit_plan(b.c);
    const bool wide = dp.nd0 > DW_POINTS;
    // bucket sums -> digit sums: on slots (msm_tail.hip) where the chain is latency-bound, one lane per point where the launch is throughput-bound
    // (msm_tail.cuh).  ZK_TAIL_SLOTS = 0 / 1 forces one form of the digit sums, ZK_TAIL_FIXUP_SLOTS = 1 puts the fix-up on slots (A/B runs, latency-first
    // deployments).  Digit sums -> product: always msm_tail.hip.
    // (cached; read per call only under ZK_TEST_FORMS=1, where the GPU suite flips them inside one process to hold every form to the oracle)
    const int force = opt_int(OPT_TAIL_SLOTS, -1), force_fixup = opt_int(OPT_TAIL_FIXUP_SLOTS, -1);
    const bool by_chunk_ok = opt_on(OPT_FIXUP_BY_CHUNK, true);      // A/B switch
    const bool sums_on_slots = force < 0 ? !wide : force != 0;
    if (force_fixup > 0) {                                 // default: lanes at every width (fewer instructions: +1.5 % proofs/s at 2^16, +0.8 % at 2^18; slots: -0.3 ms of a lone 2^18 proof)
        ZKCHK(msm_tail_fixup_slots(jobs, count, n2, max_nb, s));
    } else {
        ScopedTimer t1("msm_reduce:fixup", s);
        // one worker per bucket, or per chunk border where those are fewer (msm_red.hip: k_msm_fixup)
        ZKCHK(msm_red_fixup_launch(jobs, count, n2, by_chunk_ok && max_chunks < max_nb, by_chunk_ok && max_chunks < max_nb ? max_chunks : max_nb, max_nb, s));
    }
    if (sums_on_slots) {
        ZKCHK(msm_tail_digit_sums_slots(jobs, count, n2, nwin, b.c, s));
    } else {
        const uint32_t wg_env = (uint32_t)opt_int(OPT_DS_WIDE_GROUP, 0);          // a kernel-form switch like the ones above
        ScopedTimer t2("msm_reduce:digit_sums", s);
        ZKCHK(msm_red_digit_sums_launch(jobs, count, n2, nwin, dp, wide, wg_env, s));
    }
    return msm_tail_weight_slots(jobs, count, n2, nwin, b.c, s);
}
int msm_reduce(const MsmBases& b, MsmWorkspace* const* ws, void* const* outs, uint32_t count, hipStream_t s) {
    return b.curve == CURVE_G1 ? msm_reduce_mixed(&b, ws, outs, count, nullptr, nullptr, nullptr, 0, s)
                               : msm_reduce_mixed(nullptr, nullptr, nullptr, 0, &b, ws, outs, count, s);
}
int msm_run(const MsmBases& b, MsmWorkspace& w, const void* d_scalars, void* d_out, hipStream_t s) {
    ZKCHK(msm_sort_accumulate(b, w, d_scalars, s));
    MsmWorkspace* ws[1] = {&w};
    void* outs[1] = {d_out};
    return msm_reduce(b, ws, outs, 1, s);
}
// Fr canonical check on device scalars
__global__ void k_check_scalars(const uint32_t* s, uint64_t n, int* flag) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr a = fe_load<FrParams>(s + 8 * i);
    if (!fe_is_canonical(a)) *flag = 1;
}
// powers: out[i] = s^i (canonical), sequential products split over lanes by fast exponentiation
__global__ void k_fr_powers(uint32_t* out, const uint32_t* s_canon, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr base = fe_to_mont(fe_load<FrParams>(s_canon)), acc = fe_one<FrParams>();
    for (uint64_t e = i; e; e >>= 1) {
        if (e & 1) acc = fe_mul(acc, base);
        base = fe_sqr(base);
    }
    fe_store<FrParams>(out + 8 * i, fe_from_mont(acc));
}

static int msm_api(Curve curve, const uint8_t* bases, size_t nbases, const uint8_t* scalars, size_t nscalars, uint32_t window_bits, uint8_t* out) {
    if (!out) ZK_FAIL(ZK_ERR_ARG, "msm: null output");
    if (nscalars > nbases) ZK_FAIL(ZK_ERR_APPLY_POWERS, "apply_powers");        // curve.ml:116
    ZKCHK(ensure_init());
    Ctx& c = ctx();
    if (nscalars == 0) {                                                        // curve.ml:115: zero
        memset(out, 0, aff_bytes(curve));
        out[0] = 0x40;
        return ZK_OK;
    }
    if (!bases || !scalars) ZK_FAIL(ZK_ERR_ARG, "msm: null input");
    MsmBases b;
    MsmWorkspace w;
    // ZK_MSM_API_PRECOMP=1 runs this entry point through the resident-key machinery (window tables, one bucket set, batch-affine
    // rounds): how the tests reach those kernels with adversarial base sets (duplicates, negations, the identity)
    const bool precomp = opt_on(OPT_MSM_API_PRECOMP, false);
    ZKCHK(msm_bases_from_bytes(b, curve, bases, nscalars, window_bits, precomp, c.stream));
    ZKCHK(msm_workspace_alloc(w, b));
    DevBuf sc, res, flag;
    ZKCHK(sc.alloc(32 * nscalars));
    ZKCHK(res.alloc(xyzz_bytes(curve)));
    ZKCHK(flag.alloc(4));
    HIPCHK(hipMemsetAsync(flag.p, 0, 4, c.stream));
    HIPCHK(hipMemcpyAsync(sc.p, scalars, 32 * nscalars, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(k_check_scalars, grid_for(nscalars, 256), dim3(256), 0, c.stream, sc.as<uint32_t>(), (uint64_t)nscalars, flag.as<int>());
    ZKCHK(msm_run(b, w, sc.p, res.p, c.stream));
    int h = 0;
    HIPCHK(hipMemcpyAsync(&h, flag.p, 4, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    if (h) ZK_FAIL(ZK_ERR_SCALAR_RANGE, "msm: scalar >= r");
    return points_xyzz_to_bytes(curve, res.p, 1, out, c.stream);
}
static int of_fr_api(Curve curve, const uint8_t* scalars, size_t n, uint8_t* out) {
    if (n && (!scalars || !out)) ZK_FAIL(ZK_ERR_ARG, "of_Fr: null");
    ZKCHK(ensure_init());
    if (!n) return ZK_OK;
    Ctx& c = ctx();
    DevBuf sc, aff, bytes, flag;
    ZKCHK(sc.alloc(32 * n));
    ZKCHK(aff.alloc(aff_bytes(curve) * n));
    ZKCHK(bytes.alloc(aff_bytes(curve) * n));
    ZKCHK(flag.alloc(4));
    HIPCHK(hipMemsetAsync(flag.p, 0, 4, c.stream));
    HIPCHK(hipMemcpyAsync(sc.p, scalars, 32 * n, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(k_check_scalars, grid_for(n, 256), dim3(256), 0, c.stream, sc.as<uint32_t>(), (uint64_t)n, flag.as<int>());
    ZKCHK(fixed_base_mul(curve, aff.p, sc.p, n, c.stream));
    ZKCHK(points_affine_to_bytes(curve, bytes.p, aff.p, n, c.stream));
    int h = 0;
    HIPCHK(hipMemcpyAsync(&h, flag.p, 4, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(out, bytes.p, aff_bytes(curve) * n, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    if (h) ZK_FAIL(ZK_ERR_SCALAR_RANGE, "of_Fr: scalar >= r");
    return ZK_OK;
}
static int powers_api(Curve curve, uint32_t d, const uint8_t* s32, uint8_t* out) {
    if (!s32 || !out) ZK_FAIL(ZK_ERR_ARG, "powers: null");
    ZKCHK(ensure_init());
    Ctx& c = ctx();
    uint64_t n = (uint64_t)d + 1;
    DevBuf s, sc, aff, bytes, flag;
    ZKCHK(s.alloc(32));
    ZKCHK(sc.alloc(32 * n));
    ZKCHK(aff.alloc(aff_bytes(curve) * n));
    ZKCHK(bytes.alloc(aff_bytes(curve) * n));
    ZKCHK(flag.alloc(4));
    HIPCHK(hipMemsetAsync(flag.p, 0, 4, c.stream));
    HIPCHK(hipMemcpyAsync(s.p, s32, 32, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(k_check_scalars, dim3(1), dim3(64), 0, c.stream, s.as<uint32_t>(), (uint64_t)1, flag.as<int>());
    hipLaunchKernelGGL(k_fr_powers, grid_for(n, 256), dim3(256), 0, c.stream, sc.as<uint32_t>(), s.as<uint32_t>(), n);
    ZKCHK(fixed_base_mul(curve, aff.p, sc.p, n, c.stream));
    ZKCHK(points_affine_to_bytes(curve, bytes.p, aff.p, n, c.stream));
    int h = 0;
    HIPCHK(hipMemcpyAsync(&h, flag.p, 4, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(out, bytes.p, aff_bytes(curve) * n, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    if (h) ZK_FAIL(ZK_ERR_SCALAR_RANGE, "powers: scalar >= r");
    return ZK_OK;
}

}  // namespace zk

using namespace zk;
extern "C" {
int zk_msm_g1(const uint8_t* bases, size_t nbases, const uint8_t* scalars, size_t nscalars, uint32_t window_bits, uint8_t out[96]) {
    return msm_api(CURVE_G1, bases, nbases, scalars, nscalars, window_bits, out);
}
int zk_msm_g2(const uint8_t* bases, size_t nbases, const uint8_t* scalars, size_t nscalars, uint32_t window_bits, uint8_t out[192]) {
    return msm_api(CURVE_G2, bases, nbases, scalars, nscalars, window_bits, out);
}
static int decompress_api(Curve curve, const uint8_t* in, size_t n, uint8_t* out) {
    if (n && (!in || !out)) ZK_FAIL(ZK_ERR_ARG, "decompress_batch: null");
    ZKCHK(ensure_init());
    return points_decompress(curve, in, n, out, ctx().stream);
}
int zk_g1_decompress_batch(const uint8_t* in, size_t n, uint8_t* out) { return decompress_api(CURVE_G1, in, n, out); }
int zk_g2_decompress_batch(const uint8_t* in, size_t n, uint8_t* out) { return decompress_api(CURVE_G2, in, n, out); }
// the square roots and the sign rule of the two entry points above on bare field elements (the self tests of include/zkmi355x.h, next to zk_selftest_fp)
int zk_selftest_sqrt(int field, const uint8_t* a, size_t n, uint8_t* root, uint8_t* is_square) {
    if (!a || !root || !is_square || !n || (field != 0 && field != 1)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_sqrt: null argument, no elements, or a field other than 0 (Fp) / 1 (Fp2)");
    ZKCHK(ensure_init());
    return points_selftest_sqrt(field, a, n, root, is_square, ctx().stream);
}
// the two subgroup tests side by side on encoded points (k_subgroup_verdict of msm_points.hip): method 0 = [r] P = O, 1 = by endomorphism
int zk_selftest_subgroup(int group, int method, const uint8_t* points, size_t n, uint8_t* verdict) {
    if (!points || !verdict || !n || (group != 0 && group != 1) || (method != 0 && method != 1))
        ZK_FAIL(ZK_ERR_ARG, "zk_selftest_subgroup: null argument, no points, a group other than 0 (G1) / 1 (G2), or a method other than 0 / 1");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    return points_selftest_subgroup(group ? CURVE_G2 : CURVE_G1, method ? SUBGROUP_ENDO : SUBGROUP_ORDER, points, n, verdict, ctx().stream);
}
// the decompression launch and the subgroup launch of a resident key's compressed slab front (verify_resident.hip) on bare points
int zk_selftest_point_decompress(int group, const uint8_t* in, size_t n, uint8_t* out, uint8_t* verdict) {
    if (!in || !out || !verdict || !n || (group != 0 && group != 1))
        ZK_FAIL(ZK_ERR_ARG, "zk_selftest_point_decompress: null argument, no points, or a group other than 0 (G1) / 1 (G2)");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    return points_selftest_decompress(group ? CURVE_G2 : CURVE_G1, in, n, out, verdict, ctx().stream);
}
// the conversion launch of zk_*_prove_many_compressed (k_proofs_to_wire of msm_points.hip) on XYZZ points the caller chooses
int zk_selftest_proof_wire(int group, const uint8_t* affine, const uint8_t* z, size_t n, uint8_t* out) {
    if (!affine || !z || !out || !n || n >= ((size_t)1 << 24) || (group != 0 && group != 1))
        ZK_FAIL(ZK_ERR_ARG, "zk_selftest_proof_wire: null argument, no points, or a group other than 0 (G1) / 1 (G2)");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    return points_selftest_proof_wire(group ? CURVE_G2 : CURVE_G1, affine, z, n, out, ctx().stream);
}
int zk_g1_of_fr(const uint8_t* scalars, size_t n, uint8_t* out) { return of_fr_api(CURVE_G1, scalars, n, out); }
int zk_g2_of_fr(const uint8_t* scalars, size_t n, uint8_t* out) { return of_fr_api(CURVE_G2, scalars, n, out); }
int zk_g1_powers(uint32_t d, const uint8_t s[32], uint8_t* out) { return powers_api(CURVE_G1, d, s, out); }
int zk_g2_powers(uint32_t d, const uint8_t s[32], uint8_t* out) { return powers_api(CURVE_G2, d, s, out); }
}

