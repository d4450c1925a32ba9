// Pinocchio Protocol 2 prove on gfx950: Compute.f / ZKCompute.f (src/pinocchio/pinocchio.ml:210-248,
// 427-514) on the kernels of the Groth16 path (second protocol of the scope table, row a9).
//
// With c = the witness, c_mid its restriction to the mids, h = QAP.eval's quotient and the blinding
// scalars dv, dw, dy (drawn in that order, :428-430) the eight proof elements are multi-scalar
// products over the evaluation key (:37-60); every blinding term is folded into the product whose base
// it multiplies, and  - one * dy  rides on si[0] = g^(s^0) = G1.one:
//   vv'   = <vv   | vt,              c_mid | dv>                      (:438-439)
//   ww'   = <ww   | wt,              c_mid | dw>            in G2     (:442-443)
//   yy'   = <yy   | yt,              c_mid | dy>                      (:446-447)
//   h'    = <si | v_all | w_all,     h + dv dw Z - dy e_0 | dw c | dv c>   (:450,481-486; t = apply_powers Z si, :431)
//   vavv' = <vav  | vavt,            c_mid | dv>                      (:489-490)
//   waww' = <waw  | wawt,            c_mid | dw>            in G2     (:493-494)
//   yayy' = <yay  | yayt,            c_mid | dy>                      (:497-498)
//   bvwy' = <bvwy | vbt | wbt | ybt, c_mid | dv | dw | dy>            (:500-505)
// NonZK.prove (Compute.f) is the same with dv = dw = dy = 0.
//
// The COMPACT h pool (round 5; default, ZK_PIN_COMPACT_H=0 / a key that fails the check below keeps the layout above).  v_all[k] = [v_k(s)] and
// w_all[k] = [w_k(s)] are 2 m of the h product's n + 1 + 2 m points (2 n + 4 of 3 n + 5 in the iterated-cubic benchmark) and serve the blinding only:
//   sum_k (dw c_k) [v_k(s)] = dw [v(s)],   v = sum_k c_k v_k  -- the very polynomial QAP.eval builds,
// so with the coefficients of v, w the prover already holds (the tau-power Fr stage) the two terms ride on si:
//   h' = <si, h + dv dw Z - dy e_0 + dw v + dv w>                                    n + 1 points,
// and with the derived key, where v, w exist as VALUES (v(n + t) for t < n - 1 from the extrapolation, a_i on 0 .. n-1),
//   v = kappa_v X^(n-1) + (a polynomial of degree <= n - 2),   kappa_v = sum_i a_i c_i  (leading coefficient of the interpolant),
//   h' = <[lambda_t(s)] | [Z(s)] | [1] | [s^(n-1)],  h(n+t) + dw (v(n+t) - kappa_v (n+t)^(n-1)) + dv (w(n+t) - kappa_w (n+t)^(n-1)) | dv dw | -dy | dw kappa_v + dv kappa_w>
// n + 2 points.  Same group element, same bytes -- PROVIDED the key's v_all / w_all are what KeyGen.generate makes them (pinocchio.ml:104-109,
// 140-147): that is checked at upload on the key's own points (pin_compact_check: <v_all, rho> = <si, coefficients of sum_k rho_k v_k> for a
// pseudo-random rho, likewise w_all); a key that fails keeps the full pool and is used point by point exactly as the reference uses it.
#include "device_group.cuh"
#include "ec.cuh"
#include "handle_table.h"
#include "prove_many.cuh"

#include <memory>
#include <random>
#include <string.h>

namespace zk {

static constexpr int PIN_G1 = 6, PIN_G2 = 2;

// Everything one proof in flight needs: the pipelined form keeps several of them busy on one key
// (one stream each -- see groth16.hip for why not three).
struct PinSlot {
    FrScratch fs;
    MsmWorkspace ws1[PIN_G1], ws2[PIN_G2];
    DevBuf scal1[PIN_G1], scal2[PIN_G2];
    DevBuf wit_raw, deltas, results, out_dev;
    DevBuf kappa;                     // compact derived pool: kappa_v | kappa_w | the partial sums of frstage_leading_coeffs
    hipStream_t st = nullptr;
    hipStream_t s1 = nullptr, s2 = nullptr;      // slot 0 only: the G2 pair and the h pool run beside the five I_mid pools while the proof is alone
    hipEvent_t done = nullptr, fork = nullptr, join1 = nullptr, join2 = nullptr;
    uint8_t* host = nullptr;          // pinned: proof 960 B | flags 4 B | deltas 96 B
    bool busy = false;
    ~PinSlot() {
        if (st) (void)hipStreamDestroy(st);
        if (s1) (void)hipStreamDestroy(s1);
        if (s2) (void)hipStreamDestroy(s2);
        if (fork) { (void)hipEventDestroy(fork); (void)hipEventDestroy(join1); (void)hipEventDestroy(join2); }
        if (done) (void)hipEventDestroy(done);
        if (host) (void)hipHostFree(host);
    }
};
static constexpr uint32_t PIN_MAX_SLOTS = 15;
struct PinKey {
    uint32_t n = 0, m = 0, n_mid = 0;
    // A whole key is shard 0 of 1.  A shard of a multi-device key (PinGroup below) holds the points [lo, hi) of every pool -- the pools are cut in `world`
    // equal slices -- with its own window tables; full = the pool's length.  An EMPTY slice (a pool shorter than the device list) has no base set at all.
    uint32_t rank = 0, world = 1;
    uint64_t full1[PIN_G1] = {}, lo1[PIN_G1] = {}, hi1[PIN_G1] = {};
    uint64_t full2[PIN_G2] = {}, lo2[PIN_G2] = {}, hi2[PIN_G2] = {};
    FrStage fr;
    MsmBases g1[PIN_G1], g2[PIN_G2];
    DevBuf mid_idx, wit_resident;
    bool have_witness = false;
    bool lagrange = false;              // pool 5 holds [lambda_t(s)] (n-1) | [Z(s)] | [1] | v_all | w_all instead of si (n+1) | v_all | w_all
    // One sort per distinct scalar vector (round 5): vv|vt and vav|vavt carry (c_mid | dv), yy|yt and yay|yayt (c_mid | dy), ww|wt and waw|wawt (c_mid | dw)
    // (pinocchio.ml:438-447,489-498).  share1[i] / share2[i] = the pool whose sorted references pool i's bucket accumulation reads, -1 = its own: set at
    // upload when the two base sets have the same geometry AND the same identity flags (msm_bases_same_geometry; v_k = 0 makes both of a pair the identity).
    int share1[PIN_G1] = {-1, -1, -1, -1, -1, -1}, share2[PIN_G2] = {-1, -1};
    bool in_subgroup = true;            // the upload's verdict on ZK_KEY_SUBGROUP_CHECK, read once: were this key's points checked -- for every pool built
                                        // from them, the derived h pool too (a shard whose slice was empty at upload has no MsmBases to ask)
    bool compact = false;               // pool 5 without v_all | w_all: si (n+1), or derived [lambda_t(s)] (n-1) | [Z(s)] | [1] | [s^(n-1)]  (header comment)
    DevBuf pw;                          // compact + derived: (n + t)^(n-1), t < n - 1
    std::unique_ptr<PinSlot> slots[PIN_MAX_SLOTS];
};
int derive_shifted_bases_g1(const FrStage& f, const uint8_t* d_si, uint8_t* d_out, hipStream_t s);   // lagrange_derive.hip
static HandleTable<PinKey>& g_pin = *new HandleTable<PinKey>(HANDLES_PINOCCHIO, "unknown Pinocchio key handle");

static inline dim3 g1d(uint64_t n, unsigned t = 256) { return dim3((unsigned)((n + t - 1) / t)); }

struct PinScalPtrs {
    uint32_t* s1[PIN_G1];
    uint32_t* s2[PIN_G2];
};
// the inputs of the h product's scalar vector, by key form (PinKey::lagrange, PinKey::compact)
struct PinHArgs {
    const uint32_t* h;          // tau-power: n - 1 coefficients; derived: h(n + t), t < n - 1
    const uint32_t* z;          // Z's n + 1 coefficients
    const uint32_t* vco;        // compact, tau-power: the coefficients of v and w (n each)
    const uint32_t* wco;
    const uint32_t* sa;         // compact, derived: the convolution outputs Sa_j, Sb_j at j = n + t (v(j) = zt[t] Sa_j), zt, (n + t)^(n-1), kappa_v | kappa_w
    const uint32_t* sb;
    const uint32_t* zt;
    const uint32_t* pw;
    const uint32_t* kappa;
    uint32_t lagrange, compact;
};
static inline uint64_t pin_h_points(uint32_t n, uint32_t m, bool lagrange, bool compact) {
    return compact ? (uint64_t)n + (lagrange ? 2 : 1) : (uint64_t)n + 1 + 2 * (uint64_t)m;
}
// one lane per entry of the longest vector (the h pool, or the pools over the mids where the compact h pool is shorter)
__global__ void k_pinocchio_scalars(PinScalPtrs out, PinHArgs ha, const uint32_t* __restrict__ wit_mont, const uint32_t* __restrict__ mid_idx,
                                    const uint32_t* __restrict__ deltas, uint32_t n, uint32_t m, uint32_t n_mid) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lagrange = ha.lagrange;
    const uint64_t ph = ha.compact ? (uint64_t)n + (lagrange ? 2 : 1) : (uint64_t)n + 1 + 2 * (uint64_t)m;
    if (i >= ph && i >= (uint64_t)n_mid + 3) return;
    const Fr dv = fe_to_mont(fe_load<FrParams>(deltas)), dw = fe_to_mont(fe_load<FrParams>(deltas + 8)),
             dy = fe_to_mont(fe_load<FrParams>(deltas + 16));
    const uint32_t* h = ha.h;
    const uint32_t* z = ha.z;
    // pool 5: h'
    if (i < ph) {
        Fr x;
        if (ha.compact && lagrange) {
            const Fr kv = fe_load<FrParams>(ha.kappa), kw = fe_load<FrParams>(ha.kappa + 8);
            if (i + 1 < n) {
                const Fr p = fe_load<FrParams>(ha.pw + 8 * i), zt = fe_load<FrParams>(ha.zt + 8 * i);
                const Fr ve = fe_sub(fe_mul(zt, fe_load<FrParams>(ha.sa + 8 * ((uint64_t)n + i))), fe_mul(kv, p));      // (v - kappa_v X^(n-1))(n + t)
                const Fr we = fe_sub(fe_mul(zt, fe_load<FrParams>(ha.sb + 8 * ((uint64_t)n + i))), fe_mul(kw, p));
                x = fe_add(fe_load<FrParams>(h + 8 * i), fe_add(fe_mul(dw, ve), fe_mul(dv, we)));
            } else if (i + 1 == n) x = fe_mul(dv, dw);                                   // [Z(s)]
            else if (i == n) x = fe_neg(dy);                                             // [1]
            else x = fe_add(fe_mul(dw, kv), fe_mul(dv, kw));                             // [s^(n-1)]
        } else if (ha.compact) {
            x = fe_mul(fe_mul(dv, dw), fe_load<FrParams>(z + 8 * i));                    // dv dw Z_i, i <= n
            if (i + 1 < n) x = fe_add(x, fe_load<FrParams>(h + 8 * i));
            if (i < n) x = fe_add(x, fe_add(fe_mul(dw, fe_load<FrParams>(ha.vco + 8 * i)), fe_mul(dv, fe_load<FrParams>(ha.wco + 8 * i))));
            if (i == 0) x = fe_sub(x, dy);
        } else if (i <= n && lagrange) {
            // derived key: h through its VALUES on n .. 2n-2 against [lambda_t(s)], then dv dw on the single point [Z(s)], -dy on [1]
            if (i + 1 < n) x = fe_load<FrParams>(h + 8 * i);
            else if (i + 1 == n) x = fe_mul(dv, dw);
            else x = fe_neg(dy);
        } else if (i <= n) {
            x = fe_mul(fe_mul(dv, dw), fe_load<FrParams>(z + 8 * i));            // dv dw Z_i
            if (i + 1 < n) x = fe_add(x, fe_load<FrParams>(h + 8 * i));          // h has n - 1 coefficients
            if (i == 0) x = fe_sub(x, dy);
        } else if (i <= (uint64_t)n + m) x = fe_mul(dw, fe_load<FrParams>(wit_mont + 8 * (i - n - 1)));
        else x = fe_mul(dv, fe_load<FrParams>(wit_mont + 8 * (i - n - 1 - m)));
        fe_store<FrParams>(out.s1[5] + 8 * i, fe_from_mont(x));
    }
    // pools over the mids
    if (i < (uint64_t)n_mid + 3) {
        Fr c = fe_zero<FrParams>();
        const bool is_mid = i < n_mid;
        if (is_mid) c = fe_load<FrParams>(wit_mont + 8 * (uint64_t)mid_idx[i]);
        const uint64_t e = i - n_mid;      // index among the appended single points
        auto put = [&](uint32_t* dst, uint32_t extras, const Fr& e0, const Fr& e1, const Fr& e2) {
            if (!dst) return;                                    // a pool that reads another pool's sort (PinKey::share1 / share2)
            if (is_mid) fe_store<FrParams>(dst + 8 * i, fe_from_mont(c));
            else if (e < extras) fe_store<FrParams>(dst + 8 * i, fe_from_mont(e == 0 ? e0 : (e == 1 ? e1 : e2)));
        };
        put(out.s1[0], 1, dv, dv, dv);       // vv | vt
        put(out.s1[1], 1, dy, dy, dy);       // yy | yt
        put(out.s1[2], 1, dv, dv, dv);       // vav | vavt
        put(out.s1[3], 1, dy, dy, dy);       // yay | yayt
        put(out.s1[4], 3, dv, dw, dy);       // bvwy | vbt | wbt | ybt
        put(out.s2[0], 1, dw, dw, dw);       // ww | wt
        put(out.s2[1], 1, dw, dw, dw);       // waw | wawt
    }
}

// ---- the compact h pool's precondition: v_all / w_all are the images of the key's own powers si (header comment)
static bool pin_compact_wanted() { return opt_on(OPT_PIN_COMPACT_H, true); }          // read per key (set-up path)
// The seed of rho.  The check is a random linear combination, and it is worth its 2^-254 only if rho cannot be known before the key's bytes are fixed:
// with a seed anybody can compute (rounds 1-5: a constant mixed with n and m) a key with v_all[i] += [a] G, v_all[j] -= [a rho_i / rho_j] G passes, is
// proved from si, and the proof differs from what ZKCompute.f computes from that key.  So the seed is a digest of the very bytes that are checked
// (si | v_all | w_all: changing a point changes every rho) mixed with 64 bits of entropy drawn once per process (the digest is no cryptographic hash;
// the entropy is what a key's author cannot have seen).  Verdicts do not depend on the draw: a key KeyGen.generate made passes under every rho, a key
// that breaks the relation fails under all but a negligible share (2^-64: the seed's width) of the draws.
static uint64_t pin_rho_seed(const uint8_t* bytes, size_t len, uint32_t n, uint32_t m) {
    static const uint64_t process_entropy = [] {
        std::random_device rd;
        return ((uint64_t)rd() << 32) | (uint64_t)rd();
    }();
    uint64_t h = 0x5EEDC0DE2026ull ^ ((uint64_t)n << 32) ^ m;
    for (size_t i = 0; i + 8 <= len; i += 8) {          // len is a multiple of 96
        uint64_t w;
        memcpy(&w, bytes + i, 8);
        h = (h ^ w) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    h ^= process_entropy;
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    return h ^ (h >> 31);
}
// rho[k]: pseudo-random canonical scalars below 2^254 (splitmix64 of seed and index)
__global__ void k_pin_rho(uint32_t* __restrict__ rho, uint64_t m, uint64_t seed) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    Fr r;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint64_t x = seed + (4 * k + q + 1) * 0x9E3779B97F4A7C15ull;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        x ^= x >> 31;
        r.v[2 * q] = (uint32_t)x;
        r.v[2 * q + 1] = (uint32_t)(x >> 32);
    }
    r.v[7] &= 0x3fffffffu;
    fe_store<FrParams>(rho + 8 * k, r);
}
// four scalar vectors over si | v_all | w_all (canonical):  0: coefficients of v_rho on si,  1: rho on v_all,  2: coefficients of w_rho on si,  3: rho on w_all
__global__ void k_pin_check_scalars(uint32_t* __restrict__ out, const uint32_t* __restrict__ vco, const uint32_t* __restrict__ wco,
                                    const uint32_t* __restrict__ rho, uint32_t n, uint32_t m) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t ph = (uint64_t)n + 1 + 2 * (uint64_t)m;
    if (i >= ph) return;
    const Fr zero = fe_zero<FrParams>();
    Fr x[4] = {zero, zero, zero, zero};
    if (i < n) { x[0] = fe_from_mont(fe_load<FrParams>(vco + 8 * i)); x[2] = fe_from_mont(fe_load<FrParams>(wco + 8 * i)); }
    else if (i > n && i <= (uint64_t)n + m) x[1] = fe_load<FrParams>(rho + 8 * (i - n - 1));
    else if (i > (uint64_t)n + m) x[3] = fe_load<FrParams>(rho + 8 * (i - n - 1 - m));
#pragma unroll
    for (int q = 0; q < 4; q++) fe_store<FrParams>(out + 8 * (q * ph + i), x[q]);
}
// *ok = the key's v_all / w_all equal sum_j (v_k)_j si[j] / sum_j (w_k)_j si[j] for every variable k (up to the chance of a random combination under `seed`).
// `full`: si | v_all | w_all as a plain (one-window) base set.
static int pin_compact_check(const FrStage& fr, const MsmBases& full, uint32_t n, uint32_t m, uint64_t seed, bool* ok, hipStream_t s) {
    *ok = false;
    const uint64_t ph = (uint64_t)n + 1 + 2 * (uint64_t)m;
    if (full.n != ph) ZK_FAIL(ZK_ERR_ARG, "pin_compact_check: unexpected pool length");
    FrScratch fs;
    MsmWorkspace w;
    DevBuf rho, scal, res;
    ZKCHK(frstage_scratch_alloc(fr, fs));
    ZKCHK(msm_workspace_alloc(w, full));
    ZKCHK(rho.alloc(32 * (size_t)m));
    ZKCHK(scal.alloc(32 * 4 * (size_t)ph));
    ZKCHK(res.alloc(4 * xyzz_bytes(CURVE_G1)));
    hipLaunchKernelGGL(k_pin_rho, g1d(m), dim3(256), 0, s, rho.as<uint32_t>(), (uint64_t)m, seed);
    HIPCHK(hipGetLastError());
    ZKCHK(frstage_eval(fr, fs, rho.p, s));          // v_rho = sum_k rho_k v_k and w_rho as coefficient vectors (rho satisfies no gate: flags and h are not read)
    hipLaunchKernelGGL(k_pin_check_scalars, g1d(ph), dim3(256), 0, s, scal.as<uint32_t>(), (const uint32_t*)fs.d.as<uint32_t>(),
                       (const uint32_t*)(fs.d.as<uint32_t>() + 8 * (uint64_t)fr.n2), (const uint32_t*)rho.as<uint32_t>(), n, m);
    HIPCHK(hipGetLastError());
    for (int q = 0; q < 4; q++) ZKCHK(msm_run(full, w, scal.as<uint8_t>() + 32 * q * ph, res.as<uint8_t>() + q * xyzz_bytes(CURVE_G1), s));
    uint8_t pts[4 * 96];
    ZKCHK(points_xyzz_to_bytes(CURVE_G1, res.p, 4, pts, s));          // synchronises
    *ok = memcmp(pts, pts + 96, 96) == 0 && memcmp(pts + 192, pts + 288, 96) == 0;
    return ZK_OK;
}

// the G1 generator, uncompressed (x | y big-endian): what si[0] of an evaluation key has to be (pin_key_build)
static const uint8_t G1_GENERATOR_BYTES[96] = {
    0x17, 0xf1, 0xd3, 0xa7, 0x31, 0x97, 0xd7, 0x94, 0x26, 0x95, 0x63, 0x8c, 0x4f, 0xa9, 0xac, 0x0f,
    0xc3, 0x68, 0x8c, 0x4f, 0x97, 0x74, 0xb9, 0x05, 0xa1, 0x4e, 0x3a, 0x3f, 0x17, 0x1b, 0xac, 0x58,
    0x6c, 0x55, 0xe8, 0x3f, 0xf9, 0x7a, 0x1a, 0xef, 0xfb, 0x3a, 0xf0, 0x0a, 0xdb, 0x22, 0xc6, 0xbb,
    0x08, 0xb3, 0xf4, 0x81, 0xe3, 0xaa, 0xa0, 0xf1, 0xa0, 0x9e, 0x30, 0xed, 0x74, 0x1d, 0x8a, 0xe4,
    0xfc, 0xf5, 0xe0, 0x95, 0xd5, 0xd0, 0x0a, 0xf6, 0x00, 0xdb, 0x18, 0xcb, 0x2c, 0x04, 0xb3, 0xed,
    0xd0, 0x3c, 0xc7, 0x44, 0xa2, 0x88, 0x8a, 0xe4, 0x0c, 0xaa, 0x23, 0x29, 0x46, 0xc5, 0xe7, 0xe1};
static int pin_lookup(uint64_t handle, PinKey** out) {
    if (!(*out = g_pin.find(handle))) ZK_FAIL(ZK_ERR_HANDLE, g_pin.unknown());
    return ZK_OK;
}
static inline void pin_slice(uint64_t full, uint32_t rank, uint32_t world, uint64_t* lo, uint64_t* hi) {
    *lo = full * rank / world;
    *hi = full * (rank + 1) / world;
}

// which products read another product's sort (PinKey::share1 / share2), decided per key once its base sets exist
static int pin_decide_shared_sort(PinKey& k, hipStream_t s) {
    if (!opt_on(OPT_PIN_SHARED_SORT, true)) return ZK_OK;          // 0: every product sorts for itself (A/B, tests)
    auto try_share = [&](const MsmBases& a, const MsmBases& b, int* slot, int from) -> int {
        if (!a.n || !b.n) return ZK_OK;
        bool same = false;
        ZKCHK(msm_bases_same_geometry(a, b, &same, s));
        if (same) *slot = from;
        return ZK_OK;
    };
    ZKCHK(try_share(k.g1[0], k.g1[2], &k.share1[2], 0));
    ZKCHK(try_share(k.g1[1], k.g1[3], &k.share1[3], 1));
    ZKCHK(try_share(k.g2[0], k.g2[1], &k.share2[1], 0));
    return ZK_OK;
}
// Builds a key -- whole (rank 0 of world 1) or rank's shard -- on the CURRENT virtual device; nothing is registered under a handle.
// compact_in: -1 = decide here (the upload's consistency check of v_all / w_all against si, header comment: needs the WHOLE h pool, so rank 0 of a
// group runs it and hands its verdict to the other shards), 0 / 1 = the verdict.
static int pin_key_build(std::unique_ptr<PinKey>& out, uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid,
                         const uint8_t* pk_g1, size_t pk_g1_points, const uint8_t* pk_g2, size_t pk_g2_points, uint32_t rank, uint32_t world, int compact_in,
                         bool wire = false) {
    // wire: pk_g1 / pk_g2 hold wire bytes, 48 / 96 per point (zk_pinocchio_pk_upload_compressed): the same regrouping at half the stride, every pool
    // through msm_bases_from_wire
    if (!mid || !pk_g1 || !pk_g2) ZK_FAIL(ZK_ERR_ARG, "pinocchio pk_upload: null argument");
    const size_t B1 = wire ? 48 : 96, B2 = wire ? 96 : 192;
    Ctx& c = ctx();
    auto key = std::make_unique<PinKey>();
    PinKey& k = *key;
    k.n = n; k.m = m; k.rank = rank; k.world = world;
    k.in_subgroup = key_subgroup_check();
    std::vector<uint32_t> mids;
    for (uint32_t i = 0; i < m; i++)
        if (mid[i]) mids.push_back(i);
    const uint64_t nm = k.n_mid = (uint32_t)mids.size();
    if (n < 1) ZK_FAIL(ZK_ERR_ARG, "pinocchio pk_upload: need at least 1 constraint");      // an EMPTY I_mid is fine: the pools keep their appended single points
    if (pk_g1_points != 5 * nm + (n + 1) + 2 * (uint64_t)m + 7) ZK_FAIL(ZK_ERR_DOMAIN, "pinocchio pk_upload: G1 key length");
    if (pk_g2_points != 2 * nm + (n + 1) + 2) ZK_FAIL(ZK_ERR_DOMAIN, "pinocchio pk_upload: G2 key length");
    // si[0] must be the generator: ZKCompute.f subtracts `one * dy` -- G1.one, not a point of the key (pinocchio.ml:485) -- and the library lets that term
    // ride on si[0] (the h pool has no base of its own for it).  True of every key KeyGen.generate makes (si[0] = [s^0]); a key that breaks it is refused
    // here rather than proved with other bytes than the reference's.
    // (on the wire the generator is its abscissa under the compression bit: y is the smaller root, so no sign bit)
    bool si0_is_one = wire ? (pk_g1[48 * (5 * nm)] == (G1_GENERATOR_BYTES[0] | 0x80) && memcmp(pk_g1 + 48 * (5 * nm) + 1, G1_GENERATOR_BYTES + 1, 47) == 0)
                           : memcmp(pk_g1 + 96 * (5 * nm), G1_GENERATOR_BYTES, 96) == 0;
    if (!si0_is_one)
        ZK_FAIL(ZK_ERR_ARG, "pinocchio pk_upload: si[0] is not the G1 generator (the blinding term -dy * one of pinocchio.ml:485 rides on si[0])");
    ZKCHK(frstage_init(k.fr, n, m, L, R, O, c.stream));
    // slices of the flattened key (pinocchio.ml:37-60; layout in include/zkmi355x.h)
    const uint8_t *VV = pk_g1, *YY = VV + B1 * nm, *VAV = YY + B1 * nm, *YAY = VAV + B1 * nm, *BV = YAY + B1 * nm,
                  *SI = BV + B1 * nm, *VALL = SI + B1 * (uint64_t)(n + 1), *WALL = VALL + B1 * (uint64_t)m, *ONES = WALL + B1 * (uint64_t)m;
    const uint8_t *WW = pk_g2, *WAW = WW + B2 * nm, *ONES2 = WAW + B2 * nm + B2 * (uint64_t)(n + 1);
    std::vector<uint8_t> buf;
    auto bases = [&](MsmBases& b, Curve cv, const uint8_t* bytes, uint64_t cnt, bool precomp) -> int {
        return wire ? msm_bases_from_wire(b, cv, bytes, cnt, 0, precomp, c.stream, k.in_subgroup) : msm_bases_from_bytes(b, cv, bytes, cnt, 0, precomp, c.stream, k.in_subgroup);
    };
    // pool idx = base[0 .. cnt) | extras, of which this shard keeps [lo, hi)
    auto pool1 = [&](int idx, const uint8_t* base, uint64_t cnt, std::initializer_list<const uint8_t*> extras) -> int {
        const uint64_t full = cnt + extras.size();
        k.full1[idx] = full;
        pin_slice(full, rank, world, &k.lo1[idx], &k.hi1[idx]);
        const uint64_t lo = k.lo1[idx], hi = k.hi1[idx];
        if (hi == lo) return ZK_OK;
        buf.clear();
        if (lo < cnt) buf.assign(base + B1 * lo, base + B1 * (hi < cnt ? hi : cnt));
        uint64_t e = cnt;
        for (auto x : extras) {
            if (e >= lo && e < hi) buf.insert(buf.end(), x, x + B1);
            e++;
        }
        return bases(k.g1[idx], CURVE_G1, buf.data(), buf.size() / B1, true);
    };
    ZKCHK(pool1(0, VV, nm, {ONES + B1 * 0}));
    ZKCHK(pool1(1, YY, nm, {ONES + B1 * 1}));
    ZKCHK(pool1(2, VAV, nm, {ONES + B1 * 2}));
    ZKCHK(pool1(3, YAY, nm, {ONES + B1 * 3}));
    ZKCHK(pool1(4, BV, nm, {ONES + B1 * 4, ONES + B1 * 5, ONES + B1 * 6}));
    const uint64_t ph_full = (uint64_t)n + 1 + 2 * (uint64_t)m;          // si | v_all | w_all are contiguous in the key
    int compact = compact_in;
    if (compact < 0) compact = 0;
    if (compact_in < 0 && pin_compact_wanted()) {
        // every point is decoded and checked as before (of_bytes_exn); the pool then keeps v_all | w_all only if they fail the check of the header comment
        MsmBases full;
        ZKCHK(bases(full, CURVE_G1, SI, ph_full, false));
        bool ok = false;
        ZKCHK(pin_compact_check(k.fr, full, n, m, pin_rho_seed(SI, B1 * ph_full, n, m), &ok, c.stream));          // the bytes the caller handed over, wire or not
        compact = ok ? 1 : 0;
    }
    k.compact = compact != 0;
    ZKCHK(pool1(5, SI, k.compact ? (uint64_t)n + 1 : ph_full, {}));          // this shard's slice decodes and checks its own points (rank 0 has seen all of them when it ran the check)
    auto pool2 = [&](int idx, const uint8_t* base, const uint8_t* extra) -> int {
        k.full2[idx] = nm + 1;
        pin_slice(nm + 1, rank, world, &k.lo2[idx], &k.hi2[idx]);
        const uint64_t lo = k.lo2[idx], hi = k.hi2[idx];
        if (hi == lo) return ZK_OK;
        buf.clear();
        if (lo < nm) buf.assign(base + B2 * lo, base + B2 * (hi < nm ? hi : nm));
        if (hi == nm + 1) buf.insert(buf.end(), extra, extra + B2);
        return bases(k.g2[idx], CURVE_G2, buf.data(), buf.size() / B2, true);
    };
    ZKCHK(pool2(0, WW, ONES2));
    ZKCHK(pool2(1, WAW, ONES2 + B2));
    ZKCHK(pin_decide_shared_sort(k, c.stream));
    ZKCHK(k.mid_idx.alloc(4 * (nm ? nm : 1)));
    if (nm) HIPCHK(hipMemcpyAsync(k.mid_idx.p, mids.data(), 4 * nm, hipMemcpyHostToDevice, c.stream));
    ZKCHK(k.wit_resident.alloc(32 * (size_t)m));
    HIPCHK(hipStreamSynchronize(c.stream));
    out = std::move(key);
    return ZK_OK;
}

// ---- the derivation of the h pool (zk_pinocchio_pk_derive_lagrange), in two halves so that a multi-device key can run the first on one device
// d_old: the WHOLE h pool as uploaded, dense affine (si | v_all | w_all, or si alone when compact), on the current device.
// pool_out: the whole derived pool, dense affine:  [lambda_t(s)] (n-1) | [Z(s)] | [1] | [s^(n-1)]   resp.   ... | [1] | v_all | w_all
static int pin_derive_pool(const PinKey& k, const uint8_t* d_old, DevBuf& pool_out, hipStream_t s) {
    const uint32_t n = k.n;
    const uint64_t ph = pin_h_points(n, k.m, true, k.compact);
    ZKCHK(pool_out.alloc(96 * ph));
    uint8_t* pool = pool_out.as<uint8_t>();
    const uint8_t* si = d_old;
    // [lambda_t(s)], t < n - 1
    ZKCHK(derive_shifted_bases_g1(k.fr, si, pool, s));
    // [Z(s)] = sum_i Z_i [s^i]: one MSM over the n + 1 powers with the canonical coefficients of Z
    {
        MsmBases b;
        MsmWorkspace w;
        DevBuf zc, res, bytes, flag;
        ZKCHK(msm_bases_from_device_affine(b, CURVE_G1, si, (uint64_t)n + 1, 0, false, s));
        ZKCHK(msm_workspace_alloc(w, b));
        ZKCHK(zc.alloc(32 * ((size_t)n + 1)));
        ZKCHK(res.alloc(xyzz_bytes(CURVE_G1)));
        ZKCHK(bytes.alloc(96));
        ZKCHK(flag.alloc(4));
        ZKCHK(fr_from_mont(zc.p, k.fr.z.p, (uint64_t)n + 1, s));
        ZKCHK(msm_run(b, w, zc.p, res.p, s));
        ZKCHK(points_xyzz_to_bytes_dev(CURVE_G1, res.p, 1, bytes.p, s));
        HIPCHK(hipMemsetAsync(flag.p, 0, 4, s));
        ZKCHK(points_bytes_to_affine(CURVE_G1, pool + 96 * (uint64_t)(n - 1), bytes.p, 1, flag.as<int>(), s));
        HIPCHK(hipStreamSynchronize(s));
    }
    HIPCHK(hipMemcpyAsync(pool + 96 * (uint64_t)n, si, 96, hipMemcpyDeviceToDevice, s));                                       // [1] = si[0]
    if (k.compact) HIPCHK(hipMemcpyAsync(pool + 96 * ((uint64_t)n + 1), si + 96 * (uint64_t)(n - 1), 96, hipMemcpyDeviceToDevice, s));    // [s^(n-1)]
    else HIPCHK(hipMemcpyAsync(pool + 96 * ((uint64_t)n + 1), si + 96 * ((uint64_t)n + 1), 96 * 2 * (uint64_t)k.m, hipMemcpyDeviceToDevice, s));   // v_all | w_all
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}
// d_pool: the whole derived pool on the current device; the key takes its slice of it (own window tables), the Fr stage flips to the values of h
static int pin_install_derived(PinKey& k, const uint8_t* d_pool, hipStream_t s) {
    const uint32_t n = k.n;
    const uint64_t ph = pin_h_points(n, k.m, true, k.compact);
    const MsmBases& old = k.g1[5];
    uint64_t lo, hi;
    pin_slice(ph, k.rank, k.world, &lo, &hi);
    MsmBases nb;
    if (hi > lo) ZKCHK(msm_bases_from_device_affine(nb, CURVE_G1, d_pool + 96 * lo, hi - lo, old.n ? old.c : 0, true, s, k.in_subgroup));   // derived from checked points: msm.cuh, msm_fold
    if (k.compact) {
        ZKCHK(k.pw.alloc(32 * (size_t)(n > 1 ? n - 1 : 1)));
        ZKCHK(frstage_shifted_powers(k.pw.p, n, n - 1, n - 1, s));
    }
    ZKCHK(frstage_init_lagrange(k.fr, s));
    HIPCHK(hipStreamSynchronize(s));
    k.g1[5] = std::move(nb);
    k.full1[5] = ph; k.lo1[5] = lo; k.hi1[5] = hi;
    k.lagrange = true;
    for (uint32_t i = 0; i < PIN_MAX_SLOTS; i++) k.slots[i].reset();          // the h pool changed its length (compact) and the Fr scratch its form: slots are rebuilt on demand
    return ZK_OK;
}
// A whole key from pools the library generated itself (keygen.hip): d_g1 / d_g2 hold the evaluation key in the layout of zk_pinocchio_pk_upload as
// dense affine points on the current device; d_hl != nullptr: [lambda_t(s)] (n-1) | [Z(s)] as well, and the key comes out in its derived form (what
// upload + zk_pinocchio_pk_derive_lagrange leave).  No decoding and no checks: every point is [e] G for an exponent computed here, so it has order r
// (in_subgroup = true: folded windows are allowed, msm.cuh) and v_all / w_all satisfy the relation behind the compact h pool by construction -- the
// rho check of the upload is skipped, ZK_PIN_COMPACT_H alone decides.
int pin_key_from_device(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t* d_g1, const uint8_t* d_g2,
                        const uint8_t* d_hl, uint64_t* handle) {
    Ctx& c = ctx();
    auto key = std::make_unique<PinKey>();
    PinKey& k = *key;
    k.n = n; k.m = m;
    k.in_subgroup = true;
    std::vector<uint32_t> mids;
    for (uint32_t i = 0; i < m; i++)
        if (mid[i]) mids.push_back(i);
    const uint64_t nm = k.n_mid = (uint32_t)mids.size();
    ZKCHK(frstage_init(k.fr, n, m, L, R, O, c.stream));
    const uint64_t SI = 5 * nm, ONES = SI + (n + 1) + 2 * (uint64_t)m, ONES2 = 2 * nm + (n + 1);
    DevBuf tmp;
    ZKCHK(tmp.alloc(192 * (nm + 3)));
    // pool = key[base, base + nm) | key[extra, extra + nextra)
    auto pool = [&](MsmBases& b, Curve cv, const uint8_t* d_key, uint64_t base, uint64_t extra, uint64_t nextra, uint64_t* full, uint64_t* hi) -> int {
        const size_t pb = aff_bytes(cv);
        if (nm) HIPCHK(hipMemcpyAsync(tmp.p, d_key + pb * base, pb * nm, hipMemcpyDeviceToDevice, c.stream));
        HIPCHK(hipMemcpyAsync(tmp.as<uint8_t>() + pb * nm, d_key + pb * extra, pb * nextra, hipMemcpyDeviceToDevice, c.stream));
        *full = *hi = nm + nextra;
        ZKCHK(msm_bases_from_device_affine(b, cv, tmp.p, nm + nextra, 0, true, c.stream, true));
        HIPCHK(hipStreamSynchronize(c.stream));          // tmp is reused by the next pool
        return ZK_OK;
    };
    for (int i = 0; i < 4; i++) ZKCHK(pool(k.g1[i], CURVE_G1, d_g1, i * nm, ONES + i, 1, &k.full1[i], &k.hi1[i]));
    ZKCHK(pool(k.g1[4], CURVE_G1, d_g1, 4 * nm, ONES + 4, 3, &k.full1[4], &k.hi1[4]));
    ZKCHK(pool(k.g2[0], CURVE_G2, d_g2, 0, ONES2, 1, &k.full2[0], &k.hi2[0]));
    ZKCHK(pool(k.g2[1], CURVE_G2, d_g2, nm, ONES2 + 1, 1, &k.full2[1], &k.hi2[1]));
    k.compact = pin_compact_wanted();
    const uint8_t* si = d_g1 + 96 * SI;
    if (!d_hl) {
        const uint64_t ph = pin_h_points(n, m, false, k.compact);          // si, or si | v_all | w_all: contiguous in the key
        ZKCHK(msm_bases_from_device_affine(k.g1[5], CURVE_G1, si, ph, 0, true, c.stream, true));
        k.full1[5] = k.hi1[5] = ph;
    } else {
        // the pool pin_derive_pool builds:  [lambda_t(s)] (n-1) | [Z(s)] | [1] = si[0] | [s^(n-1)] = si[n-1]   resp.   ... | [1] | v_all | w_all
        DevBuf hp;
        ZKCHK(hp.alloc(96 * pin_h_points(n, m, true, k.compact)));
        HIPCHK(hipMemcpyAsync(hp.p, d_hl, 96 * (uint64_t)n, hipMemcpyDeviceToDevice, c.stream));
        HIPCHK(hipMemcpyAsync(hp.as<uint8_t>() + 96 * (uint64_t)n, si, 96, hipMemcpyDeviceToDevice, c.stream));
        if (k.compact) HIPCHK(hipMemcpyAsync(hp.as<uint8_t>() + 96 * ((uint64_t)n + 1), si + 96 * (uint64_t)(n - 1), 96, hipMemcpyDeviceToDevice, c.stream));
        else HIPCHK(hipMemcpyAsync(hp.as<uint8_t>() + 96 * ((uint64_t)n + 1), si + 96 * ((uint64_t)n + 1), 96 * 2 * (uint64_t)m, hipMemcpyDeviceToDevice, c.stream));
        ZKCHK(pin_install_derived(k, hp.as<uint8_t>(), c.stream));          // synchronises: hp has been read
    }
    ZKCHK(pin_decide_shared_sort(k, c.stream));
    ZKCHK(k.mid_idx.alloc(4 * (nm ? nm : 1)));
    if (nm) HIPCHK(hipMemcpyAsync(k.mid_idx.p, mids.data(), 4 * nm, hipMemcpyHostToDevice, c.stream));
    ZKCHK(k.wit_resident.alloc(32 * (size_t)m));
    HIPCHK(hipStreamSynchronize(c.stream));
    *handle = g_pin.add(std::move(key));
    return ZK_OK;
}
static int pin_check_idle(PinKey& k, const char* who) {
    for (uint32_t i = 0; i < PIN_MAX_SLOTS; i++)
        if (k.slots[i] && k.slots[i]->busy) ZK_FAIL(ZK_ERR_ARG, who);
    return ZK_OK;
}
// this shard's slice of pool `pool` (0..5 G1, 6..7 G2) as uncompressed points -- wire: as wire bytes -- at out (host)
static int pin_slice_points(PinKey& k, int pool, uint8_t* out, bool wire = false) {
    const MsmBases& b = pool < PIN_G1 ? k.g1[pool] : k.g2[pool - PIN_G1];
    if (!b.n) return ZK_OK;
    Ctx& c = ctx();
    DevBuf bytes, dense;
    ZKCHK(dense.alloc(aff_bytes(b.curve) * b.n));
    ZKCHK(msm_bases_dense(b, 0, b.n, dense.p, c.stream));
    if (wire) return points_affine_to_wire(b.curve, dense.p, b.n, out, c.stream);
    ZKCHK(bytes.alloc(aff_bytes(b.curve) * b.n));
    ZKCHK(points_affine_to_bytes(b.curve, bytes.p, dense.p, b.n, c.stream));
    HIPCHK(hipMemcpyAsync(out, bytes.p, aff_bytes(b.curve) * b.n, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    return ZK_OK;
}

static int pin_slot_get(PinKey& k, uint32_t idx, PinSlot** out) {
    if (idx >= PIN_MAX_SLOTS) ZK_FAIL(ZK_ERR_ARG, "pinocchio: slot index out of range (max 15 proofs in flight)");
    if (!k.slots[idx]) {
        auto sl = std::make_unique<PinSlot>();
        ZKCHK(frstage_scratch_alloc(k.fr, sl->fs));
        // scalar vectors over the FULL pools (any shard may own a proof's Fr stage); workspaces for the shard's own base sets
        for (int i = 0; i < PIN_G1; i++) { if (k.g1[i].n) ZKCHK(msm_workspace_alloc(sl->ws1[i], k.g1[i])); ZKCHK(sl->scal1[i].alloc(32 * k.full1[i])); }
        for (int i = 0; i < PIN_G2; i++) { if (k.g2[i].n) ZKCHK(msm_workspace_alloc(sl->ws2[i], k.g2[i])); ZKCHK(sl->scal2[i].alloc(32 * k.full2[i])); }
        ZKCHK(sl->wit_raw.alloc(32 * (size_t)k.m));
        ZKCHK(sl->deltas.alloc(96));
        ZKCHK(sl->kappa.alloc(32 * (2 + 2 * (size_t)LEAD_BLOCKS)));
        ZKCHK(sl->results.alloc(PIN_G1 * xyzz_bytes(CURVE_G1) + PIN_G2 * xyzz_bytes(CURVE_G2)));
        ZKCHK(sl->out_dev.alloc(960));
        HIPCHK(hipStreamCreateWithFlags(&sl->st, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&sl->done, hipEventDisableTiming));
        if (idx == 0 && k.world == 1 && !opt_is_set(OPT_SERIAL_STREAMS)) {
            // the slot of the synchronous zk_pinocchio_prove: two more streams, used only while no other proof is in flight (groth16.hip, slot 0)
            HIPCHK(hipStreamCreateWithFlags(&sl->s1, hipStreamNonBlocking));
            HIPCHK(hipStreamCreateWithFlags(&sl->s2, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&sl->fork, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&sl->join1, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&sl->join2, hipEventDisableTiming));
        }
        HIPCHK(hipHostMalloc((void**)&sl->host, 1088, hipHostMallocDefault));
        k.slots[idx] = std::move(sl);
    }
    *out = k.slots[idx].get();
    return ZK_OK;
}

// First half of a proof, on the slot's stream: the Fr stage, then the eight scalar vectors over the FULL pools.  all_vectors: also the vectors of
// pools that read another pool's sort on THIS key (a multi-device key's other shards decide on their own slices).
static int pin_scalars_enqueue(PinKey& k, PinSlot& sl, const uint8_t* sol, const uint8_t dv[32], const uint8_t dw[32], const uint8_t dy[32], bool all_vectors) {
    hipStream_t s0 = sl.st;
    const void* wit = k.wit_resident.p;
    if (sol) {
        HIPCHK(hipMemcpyAsync(sl.wit_raw.p, sol, 32 * (size_t)k.m, hipMemcpyHostToDevice, s0));
        wit = sl.wit_raw.p;
    } else if (!k.have_witness) ZK_FAIL(ZK_ERR_ARG, "no witness: pass sol or call zk_pinocchio_set_witness first");
    memcpy(sl.host + 992, dv, 32); memcpy(sl.host + 1024, dw, 32); memcpy(sl.host + 1056, dy, 32);
    HIPCHK(hipMemcpyAsync(sl.deltas.p, sl.host + 992, 96, hipMemcpyHostToDevice, s0));
    if (k.lagrange) ZKCHK(frstage_eval_lagrange(k.fr, sl.fs, wit, s0));
    else ZKCHK(frstage_eval(k.fr, sl.fs, wit, s0));
    PinScalPtrs ptrs;
    for (int i = 0; i < PIN_G1; i++) ptrs.s1[i] = all_vectors || k.share1[i] < 0 ? sl.scal1[i].as<uint32_t>() : nullptr;
    for (int i = 0; i < PIN_G2; i++) ptrs.s2[i] = all_vectors || k.share2[i] < 0 ? sl.scal2[i].as<uint32_t>() : nullptr;
    const uint64_t ph = pin_h_points(k.n, k.m, k.lagrange, k.compact);
    PinHArgs ha{};
    ha.h = sl.fs.h.as<uint32_t>(); ha.z = k.fr.z.as<uint32_t>();
    ha.lagrange = k.lagrange ? 1u : 0u; ha.compact = k.compact ? 1u : 0u;
    if (k.compact && k.lagrange) {
        uint32_t* kap = sl.kappa.as<uint32_t>();
        ZKCHK(frstage_leading_coeffs(k.fr, sl.fs, kap, kap + 16, s0));
        ha.sa = sl.fs.bufA.as<uint32_t>(); ha.sb = sl.fs.bufA.as<uint32_t>() + 8 * (uint64_t)k.fr.S;
        ha.zt = k.fr.zt.as<uint32_t>(); ha.pw = k.pw.as<uint32_t>(); ha.kappa = kap;
    } else if (k.compact) {
        ha.vco = sl.fs.d.as<uint32_t>(); ha.wco = sl.fs.d.as<uint32_t>() + 8 * (uint64_t)k.fr.n2;
    }
    const uint64_t lanes = ph > (uint64_t)k.n_mid + 3 ? ph : (uint64_t)k.n_mid + 3;
    hipLaunchKernelGGL(k_pinocchio_scalars, g1d(lanes), dim3(256), 0, s0, ptrs, ha, (const uint32_t*)sl.fs.wit.as<uint32_t>(),
                       (const uint32_t*)k.mid_idx.as<uint32_t>(), (const uint32_t*)sl.deltas.as<uint32_t>(), k.n, k.m, k.n_mid);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sl.host + 960, sl.fs.flag.p, 4, hipMemcpyDeviceToHost, s0));
    return ZK_OK;
}
// proof byte offsets: vv 0 | ww 96 | yy 288 | h 384 | vavv 480 | waww 576 | yayy 768 | bvwy 864
static constexpr uint32_t PIN_OFF1[PIN_G1] = {0, 288, 480, 768, 864, 384};
static constexpr uint32_t PIN_OFF2[PIN_G2] = {96, 576};
// Second half: the eight products over this key's slices of the pools, scalars from sl.scal*[i] + lo.  raw: the XYZZ (partial) sums stay in sl.results --
// six G1 then two G2 points, the identity for an empty slice -- for the first device of a multi-device key to add up; else affine bytes in sl.out_dev.
static int pin_msms_enqueue(PinKey& k, PinSlot& sl, bool raw) {
    hipStream_t s0 = sl.st;
    char* res = sl.results.as<char>();
    char* out = sl.out_dev.as<char>();
    const size_t x1 = xyzz_bytes(CURVE_G1), x2 = xyzz_bytes(CURVE_G2);
    auto sc1 = [&](int i) { return (const void*)(sl.scal1[i].as<char>() + 32 * k.lo1[i]); };
    auto sc2 = [&](int i) { return (const void*)(sl.scal2[i].as<char>() + 32 * k.lo2[i]); };
    // One group of products on one stream: sort + bucket accumulation per MSM; the reductions of every product whose pool got the same
    // window plan go out as ONE mixed G1 / G2 chain of launches (from 2^16 constraints up that is the whole group); one to-bytes launch.
    // G1 products [lo1, hi1), G2 products [lo2, hi2).
    auto group = [&](int lo1, int hi1, int lo2, int hi2, hipStream_t st) -> int {
        // a pool whose scalar vector another pool of the group has sorted reads that sort (the source has the lower index: it ran first on this stream) --
        // unless a workspace of the pair runs batch-affine rounds (msm_accumulate_sorted refuses that pair): then it sorts the same vector itself.  Decided
        // here, not at upload: the rounds are chosen when the slot's workspaces are allocated (ZK_MSM_BA_ROUNDS / ZK_MSM_BA_CURVES as they are then).
        for (int i = lo2; i < hi2; i++) {
            if (!k.g2[i].n) { HIPCHK(hipMemsetAsync(res + PIN_G1 * x1 + i * x2, 0, x2, st)); continue; }          // empty slice: the identity
            const int f = k.share2[i];
            if (f >= lo2 && f < i && !sl.ws2[i].ba_rounds && !sl.ws2[f].ba_rounds) { MsmWorkspace *w1[1] = {&sl.ws2[i]}, *f1[1] = {&sl.ws2[f]}; ZKCHK(msm_accumulate_sorted(k.g2[i], w1, f1, 1, st)); }
            else ZKCHK(msm_sort_accumulate(k.g2[i], sl.ws2[i], f < 0 ? sc2(i) : sc2(f), st));
        }
        for (int i = lo1; i < hi1; i++) {
            if (!k.g1[i].n) { HIPCHK(hipMemsetAsync(res + i * x1, 0, x1, st)); continue; }
            const int f = k.share1[i];
            if (f >= lo1 && f < i && !sl.ws1[i].ba_rounds && !sl.ws1[f].ba_rounds) { MsmWorkspace *w1[1] = {&sl.ws1[i]}, *f1[1] = {&sl.ws1[f]}; ZKCHK(msm_accumulate_sorted(k.g1[i], w1, f1, 1, st)); }
            else ZKCHK(msm_sort_accumulate(k.g1[i], sl.ws1[i], f < 0 ? sc1(i) : sc1(f), st));
        }
        bool done1[PIN_G1] = {}, done2[PIN_G2] = {};
        for (int i = lo1; i < hi1; i++) done1[i] = !k.g1[i].n;
        for (int i = lo2; i < hi2; i++) done2[i] = !k.g2[i].n;
        for (;;) {
            int lead_c = -1, lead_nw = -1;
            for (int i = lo1; i < hi1 && lead_c < 0; i++) if (!done1[i]) { lead_c = (int)k.g1[i].c; lead_nw = (int)k.g1[i].nw; }
            for (int i = lo2; i < hi2 && lead_c < 0; i++) if (!done2[i]) { lead_c = (int)k.g2[i].c; lead_nw = (int)k.g2[i].nw; }
            if (lead_c < 0) break;
            MsmWorkspace *w1[PIN_G1], *w2[PIN_G2];
            void *o1[PIN_G1], *o2[PIN_G2];
            const MsmBases *b1 = nullptr, *b2 = nullptr;
            uint32_t n1 = 0, n2 = 0;
            for (int i = lo1; i < hi1; i++)
                if (!done1[i] && (int)k.g1[i].c == lead_c && (int)k.g1[i].nw == lead_nw) { w1[n1] = &sl.ws1[i]; o1[n1] = res + i * x1; n1++; done1[i] = true; b1 = &k.g1[i]; }
            for (int i = lo2; i < hi2; i++)
                if (!done2[i] && (int)k.g2[i].c == lead_c && (int)k.g2[i].nw == lead_nw) { w2[n2] = &sl.ws2[i]; o2[n2] = res + PIN_G1 * x1 + i * x2; n2++; done2[i] = true; b2 = &k.g2[i]; }
            ZKCHK(msm_reduce_mixed(b1, w1, o1, n1, b2, w2, o2, n2, st));
        }
        if (raw) return ZK_OK;
        uint32_t o1[PIN_G1], o2[PIN_G2];
        for (int i = lo1; i < hi1; i++) o1[i - lo1] = PIN_OFF1[i];
        for (int i = lo2; i < hi2; i++) o2[i - lo2] = PIN_OFF2[i];
        return proof_points_to_bytes_dev(res + lo1 * x1, hi1 - lo1, o1, res + PIN_G1 * x1 + lo2 * x2, hi2 - lo2, o2, out, st);
    };
    // fork only while this is the one proof in flight on the key (single-proof latency); with others in flight every slot keeps to one stream
    bool forked = sl.s1 != nullptr && ctx().profiling < 2 && !raw;
    for (uint32_t i = 0; forked && i < PIN_MAX_SLOTS; i++)
        if (k.slots[i] && k.slots[i].get() != &sl && k.slots[i]->busy) forked = false;
    if (forked) {
        HIPCHK(hipEventRecord(sl.fork, s0));
        HIPCHK(hipStreamWaitEvent(sl.s1, sl.fork, 0));
        HIPCHK(hipStreamWaitEvent(sl.s2, sl.fork, 0));
        ZKCHK(group(0, 0, 0, PIN_G2, sl.s1));                  // the G2 pair: the longest reduction chain
        HIPCHK(hipEventRecord(sl.join1, sl.s1));
        ZKCHK(group(5, 6, 0, 0, sl.s2));                       // the h pool
        HIPCHK(hipEventRecord(sl.join2, sl.s2));
        ZKCHK(group(0, 5, 0, 0, s0));                          // the five pools over I_mid
        HIPCHK(hipStreamWaitEvent(s0, sl.join1, 0));
        HIPCHK(hipStreamWaitEvent(s0, sl.join2, 0));
    } else {
        ZKCHK(group(0, PIN_G1, 0, PIN_G2, s0));                // all eight products: one chain of reductions, one to-bytes launch
    }
    return ZK_OK;
}

// ================================================================== multi-device keys: N GPUs behind ONE handle (round 5; device_group.cuh is the shared part)
// With a device list of N entries (zk_set_devices / zk_set_device_list) zk_pinocchio_pk_upload builds one SHARD per entry -- 1/N of the points of each
// of the eight pools -- and returns one handle.  A proof runs over the devices as device_group.cuh describes: the Fr stage and the eight scalar vectors
// once on the slot's owner, the eight products over every device's slices (pinocchio.ml:438-505: each is a sum over key points, so it splits by points),
// 1 920 bytes of XYZZ partial sums per device to the first one.
// The consistency check behind the compact h pool runs on the first device (it needs the whole h pool), and so does the derivation of the h bases; the
// derived pool then travels to every device, which installs its slice.
struct PinGroupTraits {
    using Key = PinKey;
    using Slot = PinSlot;
    static constexpr uint32_t MAX_SLOTS = PIN_MAX_SLOTS, G1 = PIN_G1, G2 = PIN_G2, PROOF_BYTES = 960;
    static constexpr const uint32_t *OFF1 = PIN_OFF1, *OFF2 = PIN_OFF2;
    static int slot_get(Key& k, uint32_t idx, Slot** out) { return pin_slot_get(k, idx, out); }
    static hipStream_t stream(Slot& sl) { return sl.st; }
    static void* results(Slot& sl) { return sl.results.p; }
    static const uint8_t* flags(Slot& sl) { return sl.host + 960; }
    static constexpr const char* BROKEN = "multi-device Pinocchio key is inconsistent after a failed derivation: free it";
    static constexpr const char* SLOT_RANGE = "pinocchio: slot index out of range (max 15 proofs in flight)";
    static constexpr const char* SLOT_BUSY = "slot still has a proof in flight: call zk_pinocchio_prove_wait first";
    static constexpr const char* WAIT_NEVER_USED = "zk_pinocchio_prove_wait: slot never used";
    static constexpr const char* SET_WITNESS_BUSY = "zk_pinocchio_set_witness: a proof is in flight on this key";
};
struct PinGroup : DeviceGroup<PinGroupTraits> {
    uint32_t n = 0, m = 0;
};
static HandleTable<PinGroup>& g_pin_groups = *new HandleTable<PinGroup>(HANDLES_PINOCCHIO_GROUP, "unknown Pinocchio key handle");
static void pin_release() {
    g_pin.release_all();
    g_pin_groups.release_all([](PinGroup& g) { g.destroy(); });
}
static CleanupRegistrar g_pin_cleanup(pin_release);
static int pin_group_upload(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t* pk_g1, size_t pk_g1_points,
                            const uint8_t* pk_g2, size_t pk_g2_points, uint64_t* handle, bool wire = false) {
    const int N = ctx_count();
    auto grp = std::make_unique<PinGroup>();
    PinGroup& g = *grp;
    g.n = n; g.m = m;
    g.sub.resize(N);
    int rc = ZK_OK, compact = -1;
    // the shards one after another (set-up work; the kernels of one card's shards would take turns anyway, groth16_multi.hip): the first one decides the
    // form of the h pool for all
    for (int v = 0; v < N && rc == ZK_OK; v++) {
        DeviceScope ds(v);
        try {
            rc = pin_key_build(g.sub[v], n, m, L, R, O, mid, pk_g1, pk_g1_points, pk_g2, pk_g2_points, (uint32_t)v, (uint32_t)N, compact, wire);
        } catch (const std::exception& e) {
            rc = set_error(ZK_ERR_HIP, e.what(), __FILE__, __LINE__);
        }
        if (rc == ZK_OK && v == 0) compact = g.sub[0]->compact ? 1 : 0;
    }
    if (rc != ZK_OK) {
        g.destroy();
        return rc;
    }
    *handle = g_pin_groups.add(std::move(grp));
    return ZK_OK;
}
static int pin_group_prove_async(PinGroup& g, const uint8_t* sol, const uint8_t dv[32], const uint8_t dw[32], const uint8_t dy[32], uint32_t slot) {
    return g.prove_async(
        slot, [&](PinKey& ko, PinSlot& so) { return pin_scalars_enqueue(ko, so, sol, dv, dw, dy, true); },
        [](int v, PinKey& k, PinSlot& sv, int owner, PinSlot& so) -> int {
            if (v != owner) {
                // this device's slices of the vectors it sorts itself (a pool that reads another pool's sort on THIS shard needs none)
                for (int i = 0; i < PIN_G1; i++)
                    if (k.g1[i].n && k.share1[i] < 0)
                        ZKCHK(copy_between(sv.scal1[i].as<char>() + 32 * k.lo1[i], v, so.scal1[i].as<char>() + 32 * k.lo1[i], owner, 32 * (k.hi1[i] - k.lo1[i]), sv.st));
                for (int i = 0; i < PIN_G2; i++)
                    if (k.g2[i].n && k.share2[i] < 0)
                        ZKCHK(copy_between(sv.scal2[i].as<char>() + 32 * k.lo2[i], v, so.scal2[i].as<char>() + 32 * k.lo2[i], owner, 32 * (k.hi2[i] - k.lo2[i]), sv.st));
            }
            return pin_msms_enqueue(k, sv, true);
        });
}
static int pin_group_derive(PinGroup& g) {
    if (g.sub[0]->lagrange) return ZK_OK;
    ZKCHK(g.check_idle("zk_pinocchio_pk_derive_lagrange: a proof is in flight on this key"));
    ZKCHK(g.sync_all());
    const int N = (int)g.sub.size();
    PinKey& k0 = *g.sub[0];
    const uint64_t ph_old = k0.full1[5], ph = pin_h_points(k0.n, k0.m, true, k0.compact);
    // ---- gather the h pool as uploaded on the first device (window 0 of a shard's tables IS its slice in pool order)
    DevBuf old_dense;
    {
        DeviceScope ds(0);
        ZKCHK(old_dense.alloc(96 * ph_old));
    }
    for (int v = 0; v < N; v++) {
        DeviceScope ds(v);
        PinKey& k = *g.sub[v];
        if (!k.g1[5].n) continue;
        Ctx& c = ctx();
        DevBuf t;
        ZKCHK(t.alloc(96 * k.g1[5].n));
        ZKCHK(msm_bases_dense(k.g1[5], 0, k.g1[5].n, t.p, c.stream));
        ZKCHK(copy_between(old_dense.as<char>() + 96 * k.lo1[5], 0, t.p, v, 96 * k.g1[5].n, c.stream));
        HIPCHK(hipStreamSynchronize(c.stream));
    }
    // ---- derive on the first device, send the whole derived pool to every device
    std::vector<DevBuf> pool(N);
    {
        DeviceScope ds(0);
        ZKCHK(pin_derive_pool(k0, old_dense.as<uint8_t>(), pool[0], ctx().stream));          // nothing of the key has changed yet
    }
    for (int v = 1; v < N; v++) {
        DeviceScope ds(v);
        ZKCHK(pool[v].alloc(96 * ph));
        ZKCHK(copy_between(pool[v].p, v, pool[0].p, 0, 96 * ph, ctx().stream));
        HIPCHK(hipStreamSynchronize(ctx().stream));
    }
    // ---- install: from the first commit on the key is only consistent once every device has succeeded
    g.drop_slots();          // group slots refer to the shards' slots, which the install replaces
    for (int v = 0; v < N; v++) {
        DeviceScope ds(v);
        const int rc = pin_install_derived(*g.sub[v], pool[v].as<uint8_t>(), ctx().stream);
        if (rc != ZK_OK) {
            g.broken = true;
            return rc;
        }
    }
    return ZK_OK;
}

// ================================================================== zk_pinocchio_prove_many_compressed (prove_many.cuh holds the loop both protocols share)
// A proof's row is its slot's results: the six G1 sums in pool order (vv, yy, vavv, yayy, bvwy, h), then ww, waww.  The record is the eight points in
// declaration order (pinocchio.ml:195-208): vv 0 | ww 48 | yy 144 | h 192 | vavv 240 | waww 288 | yayy 384 | bvwy 432.
static constexpr uint32_t PIN_ROW_BYTES = PIN_G1 * 192 + PIN_G2 * 384, PIN_WIRE_BYTES = 480;
static inline ProofWire pin_wire_g1() { return {PIN_G1, PIN_ROW_BYTES, 0, PIN_WIRE_BYTES, {0, 144, 240, 384, 432, 192}}; }
static inline ProofWire pin_wire_g2() { return {PIN_G2, PIN_ROW_BYTES, PIN_G1 * 192, PIN_WIRE_BYTES, {48, 288, 0, 0, 0, 0}}; }
// a key held whole on one device: proof i in its raw form on its slot (one stream: a raw proof never forks), the sums into the row behind it
struct PinMany {
    static constexpr uint32_t ROW_BYTES = PIN_ROW_BYTES, WIRE_BYTES = PIN_WIRE_BYTES;
    PinKey& k;
    const uint8_t *sols, *blind;
    static ProofWire wire1() { return pin_wire_g1(); }
    static ProofWire wire2() { return pin_wire_g2(); }
    int enqueue(uint32_t i, uint32_t slot, void* d_row) {
        PinSlot* slp;
        ZKCHK(pin_slot_get(k, slot, &slp));
        PinSlot& sl = *slp;
        if (sl.busy) ZK_FAIL(ZK_ERR_ARG, "slot still has a proof in flight: call zk_pinocchio_prove_wait first");
        const uint8_t* d = blind + 96 * (size_t)i;
        ZKCHK(pin_scalars_enqueue(k, sl, sols ? sols + 32 * (size_t)k.m * i : nullptr, d, d + 32, d + 64, false));
        ZKCHK(pin_msms_enqueue(k, sl, true));
        HIPCHK(hipMemcpyAsync(d_row, sl.results.p, ROW_BYTES, hipMemcpyDeviceToDevice, sl.st));
        HIPCHK(hipEventRecord(sl.done, sl.st));
        sl.busy = true;
        return ZK_OK;
    }
    int finish(uint32_t slot) {
        PinSlot& sl = *k.slots[slot];
        HIPCHK(hipEventSynchronize(sl.done));
        sl.busy = false;
        return status_of_flags(sl.host + 960);
    }
};
// a multi-device key: proof by proof through the group's slot 0, the sums the first device added up as the proof's row (groth16_multi.hip: GroupMany)
struct PinGroupMany {
    static constexpr uint32_t ROW_BYTES = PIN_ROW_BYTES, WIRE_BYTES = PIN_WIRE_BYTES;
    PinGroup& g;
    const uint8_t *sols, *blind;
    int last = ZK_OK;
    static ProofWire wire1() { return pin_wire_g1(); }
    static ProofWire wire2() { return pin_wire_g2(); }
    int enqueue(uint32_t i, uint32_t, void* d_row) {
        uint8_t proof[960];
        const uint8_t* d = blind + 96 * (size_t)i;
        ZKCHK(pin_group_prove_async(g, sols ? sols + 32 * (size_t)g.m * i : nullptr, d, d + 32, d + 64, 0));
        last = g.prove_wait(0, proof);
        if (!prove_status_is_per_proof(last)) return last;
        DeviceScope ds(0);
        hipStream_t cs = ctx().stream2;          // the stream the sums were written on
        HIPCHK(hipMemcpyAsync(d_row, g.sums(0), ROW_BYTES, hipMemcpyDeviceToDevice, cs));
        HIPCHK(hipStreamSynchronize(cs));
        return ZK_OK;
    }
    int finish(uint32_t) { return last; }
};

}  // namespace zk

using namespace zk;
static int pin_upload_lagrange(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t* pk_g1, size_t pk_g1_points,
                               const uint8_t* pk_g2, size_t pk_g2_points, const uint8_t* h_lagrange, uint64_t* handle, bool wire);
extern "C" {

int zk_pinocchio_pk_upload(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid,
                           const uint8_t* pk_g1, size_t pk_g1_points, const uint8_t* pk_g2, size_t pk_g2_points, uint64_t* handle) {
    if (!handle || !mid || !pk_g1 || !pk_g2) ZK_FAIL(ZK_ERR_ARG, "pinocchio pk_upload: null argument");
    ZKCHK(ensure_init());
    if (ctx_count() > 1) return pin_group_upload(n, m, L, R, O, mid, pk_g1, pk_g1_points, pk_g2, pk_g2_points, handle);
    std::unique_ptr<PinKey> key;
    ZKCHK(pin_key_build(key, n, m, L, R, O, mid, pk_g1, pk_g1_points, pk_g2, pk_g2_points, 0, 1, -1));
    *handle = g_pin.add(std::move(key));
    return ZK_OK;
}
// zk_pinocchio_pk_upload plus the derived h bases handed in by the caller: the ordinary upload (every check, the compact check included), then
// h_lagrange = [lambda_t(s)] (n-1) | [Z(s)] decoded and checked like any key point, then pool 5 installed exactly as after a derivation.  That the
// points belong to the key's si is the caller's promise (include/zkmi355x.h).
int zk_pinocchio_pk_upload_lagrange(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid,
                                    const uint8_t* pk_g1, size_t pk_g1_points, const uint8_t* pk_g2, size_t pk_g2_points, const uint8_t* h_lagrange, uint64_t* handle) {
    if (!handle || !mid || !pk_g1 || !pk_g2 || !h_lagrange || !L || !R || !O) ZK_FAIL(ZK_ERR_ARG, "pinocchio pk_upload_lagrange: null argument");
    ZKCHK(ensure_init());
    return pin_upload_lagrange(n, m, L, R, O, mid, pk_g1, pk_g1_points, pk_g2, pk_g2_points, h_lagrange, handle, false);
}
static int pin_upload_lagrange(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t* pk_g1, size_t pk_g1_points,
                               const uint8_t* pk_g2, size_t pk_g2_points, const uint8_t* h_lagrange, uint64_t* handle, bool wire) {
    if (ctx_count() > 1) ZK_FAIL(ZK_ERR_ARG, "pinocchio pk_upload_lagrange: single-device keys only (a multi-device key derives its h bases: zk_pinocchio_pk_derive_lagrange)");
    Ctx& c = ctx();
    std::unique_ptr<PinKey> key;
    ZKCHK(pin_key_build(key, n, m, L, R, O, mid, pk_g1, pk_g1_points, pk_g2, pk_g2_points, 0, 1, -1, wire));
    PinKey& k = *key;
    MsmBases hl;          // decoding, curve equation and (unless ZK_KEY_SUBGROUP_CHECK=0) the subgroup test, as for every point of the key
    if (wire) ZKCHK(msm_bases_from_wire(hl, CURVE_G1, h_lagrange, n, 0, false, c.stream, k.in_subgroup));
    else ZKCHK(msm_bases_from_bytes(hl, CURVE_G1, h_lagrange, n, 0, false, c.stream, k.in_subgroup));
    const uint64_t ph = pin_h_points(n, m, true, k.compact);
    DevBuf pool;
    ZKCHK(pool.alloc(96 * ph));
    uint8_t* p = pool.as<uint8_t>();
    ZKCHK(msm_bases_dense(hl, 0, n, p, c.stream));
    ZKCHK(msm_bases_dense(k.g1[5], 0, 1, p + 96 * (uint64_t)n, c.stream));                                                  // [1] = si[0]
    if (k.compact) ZKCHK(msm_bases_dense(k.g1[5], n - 1, 1, p + 96 * ((uint64_t)n + 1), c.stream));                         // [s^(n-1)]
    else ZKCHK(msm_bases_dense(k.g1[5], (uint64_t)n + 1, 2 * (uint64_t)m, p + 96 * ((uint64_t)n + 1), c.stream));           // v_all | w_all
    ZKCHK(pin_install_derived(k, p, c.stream));
    *handle = g_pin.add(std::move(key));
    return ZK_OK;
}
// The evaluation key from its wire bytes (include/zkmi355x.h); h_lagrange != NULL: as zk_pinocchio_pk_upload_lagrange.  The pools are regrouped and decoded
// one by one (and slice by slice over a device list), so a refusal says only that some pool holds a bad point: the call then reads the lists in the
// caller's order -- G1, the G2 points the key keeps, h_lagrange -- for the verdict of the FIRST one.  A good key never pays for that pass.
int zk_pinocchio_pk_upload_compressed(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t* pk_g1, size_t pk_g1_points,
                                      const uint8_t* pk_g2, size_t pk_g2_points, const uint8_t* h_lagrange, uint64_t* handle) {
    if (!handle || !mid || !pk_g1 || !pk_g2 || !L || !R || !O) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_pk_upload_compressed: null argument");
    ZKCHK(ensure_init());
    int rc;
    if (h_lagrange) rc = pin_upload_lagrange(n, m, L, R, O, mid, pk_g1, pk_g1_points, pk_g2, pk_g2_points, h_lagrange, handle, true);
    else if (ctx_count() > 1) rc = pin_group_upload(n, m, L, R, O, mid, pk_g1, pk_g1_points, pk_g2, pk_g2_points, handle, true);
    else {
        std::unique_ptr<PinKey> key;
        rc = pin_key_build(key, n, m, L, R, O, mid, pk_g1, pk_g1_points, pk_g2, pk_g2_points, 0, 1, -1, true);
        if (rc == ZK_OK) *handle = g_pin.add(std::move(key));
    }
    if (rc != ZK_ERR_ARG && rc != ZK_ERR_NOT_ON_CURVE) return rc;
    if (h_lagrange && ctx_count() > 1) return rc;
    uint64_t nm = 0;
    for (uint32_t i = 0; i < m; i++) nm += mid[i] ? 1 : 0;
    if (pk_g1_points != 5 * nm + (n + 1) + 2 * (uint64_t)m + 7 || pk_g2_points != 2 * nm + (n + 1) + 2) return rc;
    const bool chk = key_subgroup_check();
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    int first = points_wire_check(CURVE_G1, pk_g1, pk_g1_points, chk, s);
    if (first == ZK_OK) first = points_wire_check(CURVE_G2, pk_g2, 2 * nm, chk, s);                                     // ww | waw
    if (first == ZK_OK) first = points_wire_check(CURVE_G2, pk_g2 + 96 * (2 * nm + (n + 1)), 2, chk, s);                // the two appended points
    if (first == ZK_OK && h_lagrange) first = points_wire_check(CURVE_G1, h_lagrange, n, chk, s);
    return first != ZK_OK ? first : rc;
}
// The h pool of an uploaded key (si | v_all | w_all, or si alone: compact) rewritten for the VALUES of h: [lambda_t(s)]_1 derived from the powers si in the
// exponent (lagrange_derive.hip: the transposed interpolation over the points n .. 2n-2), [Z(s)]_1 = <si, Z> once, [1] = si[0], and for the compact form
// [s^(n-1)] = si[n-1].  Same proofs; the per-proof basis conversion disappears (only h ever needed coefficients: v(s), w(s) come from the per-variable pools).
int zk_pinocchio_pk_derive_lagrange(uint64_t handle) {
    if (PinGroup* g = g_pin_groups.find(handle)) return pin_group_derive(*g);
    PinKey* kp;
    ZKCHK(pin_lookup(handle, &kp));
    PinKey& k = *kp;
    if (k.lagrange) return ZK_OK;
    ZKCHK(pin_check_idle(k, "zk_pinocchio_pk_derive_lagrange: a proof is in flight on this key"));
    HIPCHK(hipDeviceSynchronize());
    Ctx& c = ctx();
    const uint64_t ph_old = pin_h_points(k.n, k.m, false, k.compact);
    if (k.g1[5].n != ph_old) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_pk_derive_lagrange: unexpected pool length");
    DevBuf pool, old_dense;
    ZKCHK(old_dense.alloc(96 * ph_old));
    ZKCHK(msm_bases_dense(k.g1[5], 0, ph_old, old_dense.p, c.stream));            // window 0 = the pool as uploaded, back in the dense affine format
    ZKCHK(pin_derive_pool(k, old_dense.as<uint8_t>(), pool, c.stream));
    return pin_install_derived(k, pool.as<uint8_t>(), c.stream);
}
static int pin_pool_points(uint64_t handle, int pool, uint8_t* out, size_t capacity_points, size_t* count, bool wire) {
    if (pool < 0 || pool >= PIN_G1 + PIN_G2) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_pool_points: pool 0..5 (G1) or 6..7 (G2)");
    if (PinGroup* g = g_pin_groups.find(handle)) {          // the handle holds the whole pools (its devices' slices are an internal matter)
        PinKey& k0 = *g->sub[0];
        const uint64_t total = pool < PIN_G1 ? k0.full1[pool] : k0.full2[pool - PIN_G1];
        if (count) *count = total;
        if (!out) return ZK_OK;
        if (capacity_points < total) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_pool_points: buffer too small");
        ZKCHK(g->check_idle("zk_pinocchio_pool_points: a proof is in flight on this key"));
        const size_t pb = (pool < PIN_G1 ? 96 : 192) / (wire ? 2 : 1);
        for (size_t v = 0; v < g->sub.size(); v++) {
            DeviceScope ds((int)v);
            PinKey& k = *g->sub[v];
            ZKCHK(pin_slice_points(k, pool, out + pb * (pool < PIN_G1 ? k.lo1[pool] : k.lo2[pool - PIN_G1]), wire));
        }
        return ZK_OK;
    }
    PinKey* kp;
    ZKCHK(pin_lookup(handle, &kp));
    const MsmBases& b = pool < PIN_G1 ? kp->g1[pool] : kp->g2[pool - PIN_G1];
    if (count) *count = b.n;
    if (!out) return ZK_OK;
    if (capacity_points < b.n) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_pool_points: buffer too small");
    return pin_slice_points(*kp, pool, out, wire);
}
int zk_pinocchio_pool_points(uint64_t handle, int pool, uint8_t* out, size_t capacity_points, size_t* count) {
    return pin_pool_points(handle, pool, out, capacity_points, count, false);
}
int zk_pinocchio_pool_points_compressed(uint64_t handle, int pool, uint8_t* out, size_t capacity_points, size_t* count) {
    return pin_pool_points(handle, pool, out, capacity_points, count, true);
}
int zk_pinocchio_pk_free(uint64_t handle) {
    if (std::unique_ptr<PinGroup> g = g_pin_groups.take(handle)) {
        (void)g->sync_all();
        g->destroy();
        return ZK_OK;
    }
    if (!g_pin.find(handle)) ZK_FAIL(ZK_ERR_HANDLE, g_pin.unknown());
    (void)hipDeviceSynchronize();
    g_pin.take(handle);
    return ZK_OK;
}
int zk_pinocchio_reserve_slots(uint64_t handle, uint32_t count) {
    if (count > PIN_MAX_SLOTS) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_reserve_slots: at most 15 slots");
    if (PinGroup* g = g_pin_groups.find(handle)) return g->reserve_slots(count);
    PinKey* kp;
    ZKCHK(pin_lookup(handle, &kp));
    for (uint32_t i = 0; i < count; i++) {
        PinSlot* sl;
        ZKCHK(pin_slot_get(*kp, i, &sl));
    }
    return ZK_OK;
}
int zk_pinocchio_set_witness(uint64_t handle, const uint8_t* sol) {
    if (!sol) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_set_witness: null");
    if (PinGroup* g = g_pin_groups.find(handle)) return g->set_witness(sol);
    PinKey* kp;
    ZKCHK(pin_lookup(handle, &kp));
    Ctx& c = ctx();
    (void)hipDeviceSynchronize();      // no proof may still be reading the previous witness
    HIPCHK(hipMemcpyAsync(kp->wit_resident.p, sol, 32 * (size_t)kp->m, hipMemcpyHostToDevice, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    kp->have_witness = true;
    return ZK_OK;
}
// Enqueues one proof on the slot's stream and returns without waiting:
// Fr stage -> the eight scalar vectors -> eight MSMs -> affine bytes -> pinned host buffer.
int zk_pinocchio_prove_async(uint64_t handle, const uint8_t* sol, const uint8_t dv[32], const uint8_t dw[32], const uint8_t dy[32], uint32_t slot) {
    if (!dv || !dw || !dy) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_prove_async: null argument");
    if (PinGroup* g = g_pin_groups.find(handle)) return pin_group_prove_async(*g, sol, dv, dw, dy, slot);
    PinKey* kp;
    ZKCHK(pin_lookup(handle, &kp));
    PinKey& k = *kp;
    PinSlot* slp;
    ZKCHK(pin_slot_get(k, slot, &slp));
    PinSlot& sl = *slp;
    if (sl.busy) ZK_FAIL(ZK_ERR_ARG, "slot still has a proof in flight: call zk_pinocchio_prove_wait first");
    ZKCHK(pin_scalars_enqueue(k, sl, sol, dv, dw, dy, false));
    ZKCHK(pin_msms_enqueue(k, sl, false));
    HIPCHK(hipMemcpyAsync(sl.host, sl.out_dev.p, 960, hipMemcpyDeviceToHost, sl.st));
    HIPCHK(hipEventRecord(sl.done, sl.st));
    sl.busy = true;
    return ZK_OK;
}
int zk_pinocchio_prove_wait(uint64_t handle, uint32_t slot, uint8_t proof[960]) {
    if (!proof) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_prove_wait: null proof");
    if (PinGroup* g = g_pin_groups.find(handle)) return g->prove_wait(slot, proof);
    PinKey* kp;
    ZKCHK(pin_lookup(handle, &kp));
    if (slot >= PIN_MAX_SLOTS || !kp->slots[slot]) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_prove_wait: slot never used");
    PinSlot& sl = *kp->slots[slot];
    if (!sl.busy) ZK_FAIL(ZK_ERR_ARG, "no proof in flight on this slot");
    HIPCHK(hipEventSynchronize(sl.done));
    sl.busy = false;
    ZKCHK(status_of_flags(sl.host + 960));
    memcpy(proof, sl.host, 960);
    return ZK_OK;
}
// A batch of proofs in one call, out as wire bytes (include/zkmi355x.h)
int zk_pinocchio_prove_many_compressed(uint64_t handle, const uint8_t* sols, const uint8_t* blind, uint32_t count, uint32_t in_flight, uint8_t* proofs, int32_t* status) {
    ZKCHK(prove_many_check_args(blind, proofs, status, count, in_flight, "zk_pinocchio_prove_many_compressed: null blind, proofs or status"));
    if (!count) return ZK_OK;
    PinGroup* g = g_pin_groups.find(handle);
    if (!g && !g_pin.find(handle)) ZKCHK(ensure_init());          // without a device no handle exists: say that, not that this one is unknown
    if (g) {
        if (!sols && !g->sub[0]->have_witness) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_prove_many_compressed: no witness: pass sols or call zk_pinocchio_set_witness first");
        ZKCHK(g->check_idle("zk_pinocchio_prove_many_compressed: a proof is in flight on this key: call zk_pinocchio_prove_wait first"));
        PinGroupMany many{*g, sols, blind};
        DeviceScope ds(0);
        return prove_many_run(many, count, 1, proofs, status, ctx().stream2);
    }
    PinKey* kp;
    ZKCHK(pin_lookup(handle, &kp));
    PinKey& k = *kp;
    if (!sols && !k.have_witness) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_prove_many_compressed: no witness: pass sols or call zk_pinocchio_set_witness first");
    ZKCHK(pin_check_idle(k, "zk_pinocchio_prove_many_compressed: a proof is in flight on this key: call zk_pinocchio_prove_wait first"));
    in_flight = prove_many_in_flight(in_flight, count);
    for (uint32_t i = 0; i < in_flight; i++) {
        PinSlot* sl;
        ZKCHK(pin_slot_get(k, i, &sl));
    }
    PinMany many{k, sols, blind};
    return prove_many_run(many, count, in_flight, proofs, status, ctx().stream);
}
int zk_pinocchio_prove(uint64_t handle, const uint8_t* sol, const uint8_t dv[32], const uint8_t dw[32], const uint8_t dy[32],
                       uint8_t proof[960]) {
    if (!sol) ZK_FAIL(ZK_ERR_ARG, "zk_pinocchio_prove: null argument");
    ZKCHK(zk_pinocchio_prove_async(handle, sol, dv, dw, dy, 0));
    return zk_pinocchio_prove_wait(handle, 0, proof);
}
}
