// Signed-digit recoding of the scalars of a Pippenger product (msm.cuh: the window layout): shared by the counting sort of msm_sort.hip and the
// short products of msm_resident.hip.
#pragma once
#include "ec.cuh"
#include "msm.cuh"

namespace zk {

// ------------------------------------------------------------------ digits
// Signed c-bit digits d_j in [-(2^(c-1) - 1), 2^(c-1)] with sum_j d_j 2^(cj) = s.  Adding the constant
// K = sum_j (2^(c-1) - 1) 2^(cj) turns the recoding into plain base-2^c digit extraction:
// d_j = ((s + K) >> cj & mask) - (2^(c-1) - 1), so every (scalar, window) pair is independent and
// gets its own lane: one atomic per lane in flight instead of nw dependent ones.
struct DigitArgs {
    uint64_t n;
    uint32_t c, nw, precomp, nb_per_window;
    uint32_t K[9];         // the recoding constant, 288 bits
    const uint8_t* ident;  // precomp: 1 = base i is the identity: it never enters a bucket (nullptr: no filter)
    uint32_t coarse_shift;  // two-level sort, level 1: histogram / rank by bucket >> coarse_shift and emit (bucket, reference) records
    uint32_t scalar_major;  // LDS sorts: a workgroup owns a range of SCALARS and files all their digits (each scalar is read once per pass,
                            // not once per window: 13-16x less scalar traffic in the two passes); 0: a range of (scalar, window) pairs, window-major
    uint32_t alias_windows; // EXPERIMENT, compiled in only with -DZK_EXPERIMENTS (scripts/table_alias_ab.sh; results WRONG by design): every window
                            // reads window 0's table entries -- same additions and gathers, 1/16 of the table footprint.  Always 0 in the shipped library.
    uint32_t fold;          // digits of min(s, r - s), sign carried to every digit (msm.cuh: msm_windows): bit 31 of the ninth word of a prepared scalar is the sign
};
// scalar i plus the recoding constant (9 words); false: the scalar is zero or its base is the identity -- no digit of it enters a bucket
FF_INLINE bool digits_prepare(const uint32_t* __restrict__ scalars, uint64_t i, const DigitArgs& a, uint32_t s[9]) {
    const uint32_t* sp = scalars + 8 * i;
    uint4 lo = reinterpret_cast<const uint4*>(sp)[0], hi = reinterpret_cast<const uint4*>(sp)[1];
    s[0] = lo.x; s[1] = lo.y; s[2] = lo.z; s[3] = lo.w; s[4] = hi.x; s[5] = hi.y; s[6] = hi.z; s[7] = hi.w; s[8] = 0;
    if ((s[0] | s[1] | s[2] | s[3] | s[4] | s[5] | s[6] | s[7]) == 0) return false;
    if (a.ident && a.ident[i]) return false;
    uint32_t flip = 0;
    if (a.fold) {                                        // wave-uniform
        uint32_t t[8];
        int64_t bw = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            bw += (int64_t)FR_MOD[k] - (int64_t)s[k];
            t[k] = (uint32_t)bw;
            bw >>= 32;
        }
        bool less = false, decided = false;              // t < s, from the top word down (r is odd: t != s)
#pragma unroll
        for (int k = 7; k >= 0; k--) {
            if (!decided && t[k] != s[k]) { less = t[k] < s[k]; decided = true; }
        }
        if (less) {
            flip = 0x80000000u;
#pragma unroll
            for (int k = 0; k < 8; k++) s[k] = t[k];
        }
    }
    uint64_t cy = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        cy += (uint64_t)s[k] + a.K[k];
        s[k] = (uint32_t)cy;
        cy >>= 32;
    }
    s[8] |= flip;                                        // c nw <= 276 bits: the ninth word uses 20 bits at most
    return true;
}
FF_INLINE bool digit_at(const uint32_t s[9], uint64_t i, uint32_t j, const DigitArgs& a, uint32_t& key, uint32_t& val);
FF_INLINE bool digit_of(const uint32_t* __restrict__ scalars, uint64_t i, uint32_t j, const DigitArgs& a, uint32_t& key, uint32_t& val) {
    uint32_t s[9];
    return digits_prepare(scalars, i, a, s) && digit_at(s, i, j, a, key, val);
}
FF_INLINE bool digit_at(const uint32_t s[9], uint64_t i, uint32_t j, const DigitArgs& a, uint32_t& key, uint32_t& val) {
    const uint32_t off = j * a.c, w = off >> 5, b = off & 31;
    uint32_t x0 = 0, x1 = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) {        // static indexing keeps the scalar in registers
        if ((int)w == k) x0 = s[k];
        if ((int)w + 1 == k) x1 = k == 8 ? s[k] & 0x7fffffffu : s[k];
    }
    const uint64_t x = ((uint64_t)x1 << 32) | x0;
    const uint32_t e = (uint32_t)(x >> b) & ((1u << a.c) - 1);
    const uint32_t bias = (1u << (a.c - 1)) - 1;
    if (e == bias) return false;                        // digit 0
    const uint32_t below = e < bias ? 1u : 0u;
    const uint32_t d = below ? bias - e : e - bias;      // the digit's magnitude
    const uint32_t neg = below ^ (s[8] >> 31);           // ... its sign, turned round for a folded scalar
    key = (a.precomp ? 0u : j * a.nb_per_window) + (d - 1);
#ifdef ZK_EXPERIMENTS
    val = (uint32_t)(a.precomp && !a.alias_windows ? (uint64_t)j * a.n + i : i) | (neg << 31);
#else
    val = (uint32_t)(a.precomp ? (uint64_t)j * a.n + i : i) | (neg << 31);
#endif
    return true;
}
// host side: K = sum_j (2^(c-1) - 1) 2^(cj) over the nw windows, 288 bits
static inline void digit_constant(uint32_t c, uint32_t nw, uint32_t K[9]) {
    for (int k = 0; k < 9; k++) K[k] = 0;
    for (uint32_t j = 0; j < nw; j++) {               // K += (2^(c-1) - 1) << (c*j)
        uint64_t v = ((uint64_t)1 << (c - 1)) - 1;
        uint32_t off = j * c, wd = off >> 5, sh = off & 31;
        unsigned __int128 add = (unsigned __int128)v << sh;
        uint64_t cy = 0;
        for (uint32_t k = wd; k < 9; k++) {
            cy += (uint64_t)K[k] + (uint32_t)(add & 0xffffffffu);
            K[k] = (uint32_t)cy;
            cy >>= 32;
            add >>= 32;
            if (!add && !cy) break;
        }
    }
}

}  // namespace zk
