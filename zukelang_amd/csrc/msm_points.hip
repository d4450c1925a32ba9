// Points of BLS12-381 G1 / G2 on their way into and out of the multi-scalar multiplications of msm.hip: the byte <-> Montgomery conversions of
// the ZCash encoding, the checks the reference applies to incoming points (of_bytes_exn, src/lib/zk/curve.ml:199-212: encoding, curve equation,
// prime-order subgroup), the resident window tables 2^(c j) P_i of a base set, the fixed-base products s_i G of keygen (curve.ml:106-109,180)
// and the sum of partial results across devices.  Split off msm.hip in round 5 (one translation unit per concern: points / sort / dispatch).
#include "ec.cuh"
#include "endo_consts.cuh"
#include "msm.cuh"

#include <stdlib.h>
#include <string.h>

namespace zk {

// ------------------------------------------------------------------ byte <-> Montgomery conversions
// 48 B big-endian <-> 12 little-endian dense words (the plain integer, not Montgomery)
FF_INLINE FpWords fpw_from_be(const uint8_t* p) {
    FpWords r;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < 12; i++) r.w[i] = __builtin_bswap32(w[11 - i]);
    return r;
}
FF_INLINE void fpw_to_be(uint8_t* p, const FpWords& a) {
    uint32_t* w = reinterpret_cast<uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < 12; i++) w[11 - i] = __builtin_bswap32(a.w[i]);
}
FF_INLINE bool fpw_canonical(const FpWords& a) { return words_are_canonical<FpParams>(a.w); }

// the ONE encoding of the identity: `first` (the infinity bit next to the form's compression bit), then zeros -- the sign bit is not free either
FF_INLINE bool canonical_infinity(const uint8_t* p, int len, uint8_t first) {
    uint32_t o = p[0] ^ first;
    for (int k = 1; k < len; k++) o |= p[k];
    return o == 0;
}
// G1: x | y ; G2: x1 | x0 | y1 | y0  (ZCash uncompressed)
FF_INLINE int aff_decode(Aff<Fp>& out, const uint8_t* p) {
    uint8_t flags = p[0];
    if (flags & 0x80) return 2;                       // compressed encodings are not accepted here
    if (flags & 0x40) { out = aff_inf<Fp>(); return canonical_infinity(p, 96, 0x40) ? 0 : 2; }
    const FpWords x = fpw_from_be(p), y = fpw_from_be(p + 48);
    if (!fpw_canonical(x) || !fpw_canonical(y)) return 2;
    out = {fp_to_mont(x), fp_to_mont(y)};
    return 0;
}
FF_INLINE int aff_decode(Aff<Fp2>& out, const uint8_t* p) {
    uint8_t flags = p[0];
    if (flags & 0x80) return 2;
    if (flags & 0x40) { out = aff_inf<Fp2>(); return canonical_infinity(p, 192, 0x40) ? 0 : 2; }
    const FpWords x1 = fpw_from_be(p), x0 = fpw_from_be(p + 48), y1 = fpw_from_be(p + 96), y0 = fpw_from_be(p + 144);
    if (!fpw_canonical(x0) || !fpw_canonical(x1) || !fpw_canonical(y0) || !fpw_canonical(y1)) return 2;
    out = {{fp_to_mont(x0), fp_to_mont(x1)}, {fp_to_mont(y0), fp_to_mont(y1)}};
    return 0;
}
FF_INLINE void aff_encode(uint8_t* p, const Aff<Fp>& a) {
    if (aff_is_inf(a)) {
        uint32_t* w = reinterpret_cast<uint32_t*>(p);
        for (int i = 0; i < 24; i++) w[i] = 0;
        p[0] = 0x40;
        return;
    }
    fpw_to_be(p, fp_from_mont(a.x));
    fpw_to_be(p + 48, fp_from_mont(a.y));
}
FF_INLINE void aff_encode(uint8_t* p, const Aff<Fp2>& a) {
    if (aff_is_inf(a)) {
        uint32_t* w = reinterpret_cast<uint32_t*>(p);
        for (int i = 0; i < 48; i++) w[i] = 0;
        p[0] = 0x40;
        return;
    }
    fpw_to_be(p, fp_from_mont(a.x.c1));
    fpw_to_be(p + 48, fp_from_mont(a.x.c0));
    fpw_to_be(p + 96, fp_from_mont(a.y.c1));
    fpw_to_be(p + 144, fp_from_mont(a.y.c0));
}

// THE decoder: the bytes of one uncompressed point -> the checked dense affine point at dst (the identity when rejected) and its kind, 0 good | 2 bad
// encoding | 1 not on the curve; `bad(kind)` is called where a defect is found (the flag kernel files its bit there).  One input divides the callers:
// 96 / 192 ZERO bytes, the infinity bit NOT set.  (0, 0) is how this library's own affine format spells the identity, and aff_on_curve passes it.
//   ZERO_IS_IDENTITY   key lists and MSM bases (k_bytes_to_affine: msm_bases_from_bytes, the pool point of pinocchio.hip) accept the string as the
//                      identity: buffers that went through the library's affine format arrive that way.
//   ZERO_IS_OFF_CURVE  the verifiers' wire points (k_bytes_to_affine_verdict: points_decode_verdicts) call it a point that fails the curve equation, as
//                      g1_decode / g2_decode of pairing_host.hip do.
enum ZeroString { ZERO_IS_IDENTITY, ZERO_IS_OFF_CURVE };
template <ZeroString Z, class F, class Bad> FF_INLINE uint8_t point_decode(uint8_t* dst, const uint8_t* src, Bad&& bad) {
    Aff<F> a;
    uint8_t kind = 0;
    if (aff_decode(a, src)) { kind = 2; bad(2); }
    else if ((Z == ZERO_IS_OFF_CURVE && !(src[0] & 0x40) && aff_is_inf(a)) || !aff_on_curve(a)) { kind = 1; bad(1); }
    if (kind) a = aff_inf<F>();
    aff_store<F>(dst, a);
    return kind;
}
// one flag word per list: bit 1 = some point is not on the curve, bit 2 = some encoding is bad (msm_bases_from_bytes reads them by kind priority)
template <class F> __global__ void k_bytes_to_affine(uint8_t* dst, const uint8_t* src, uint64_t n, int* flag) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = FieldOps<F>::WORDS * 8;
    point_decode<ZERO_IS_IDENTITY, F>(dst + B * i, src + B * i, [&](int kind) { atomicOr(flag, kind); });
}
// one verdict byte per point (the verifiers: a proof's bad point is that proof's status, not the call's)
template <class F> __global__ void k_bytes_to_affine_verdict(uint8_t* dst, const uint8_t* src, uint64_t n, uint8_t* verdict) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = FieldOps<F>::WORDS * 8;
    verdict[i] = point_decode<ZERO_IS_OFF_CURVE, F>(dst + B * i, src + B * i, [](int) {});
}
template <class F> __global__ void k_affine_to_bytes(uint8_t* dst, const uint8_t* src, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = FieldOps<F>::WORDS * 8;
    aff_encode(dst + B * i, aff_load<F>(src + B * i));
}
template <class F> __global__ void k_xyzz_to_bytes(uint8_t* dst, const uint8_t* src, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = FieldOps<F>::WORDS * 8;
    aff_encode(dst + B * i, xyzz_to_aff(xyzz_load<F>(src + 2 * B * i)));
}

// All points of a proof in ONE launch (single-lane conversions, each with its own inversion, side by side instead of
// one after the other): blocks [0, n1) take the G1 points g1[i] -> out + off.g1[i], blocks [n1, n1 + n2) the G2 points.
struct ProofOffsets {
    uint32_t g1[8], g2[4];
};
__global__ __launch_bounds__(64) void k_proof_to_bytes(const uint8_t* g1, uint32_t n1, const uint8_t* g2, ProofOffsets off, uint8_t* out) {
    if (threadIdx.x != 0) return;
    const uint32_t b = blockIdx.x;
    if (b < n1) aff_encode(out + off.g1[b], xyzz_to_aff(xyzz_load<Fp>(g1 + 192 * (size_t)b)));
    else aff_encode(out + off.g2[b - n1], xyzz_to_aff(xyzz_load<Fp2>(g2 + 384 * (size_t)(b - n1))));
}

// ------------------------------------------------------------------ of_compressed_bytes_exn over whole lists (curve.ml:199-212; round 5)
// The reference's JSON holds every key point COMPRESSED (Bls12_381.G1/G2.to_compressed_bytes): a 2^20-constraint key is five million square roots and
// subgroup checks on the way in -- half an hour of one host core through zk_g1/g2_decompress, a second here.  One lane per point: x from its 48 / 96
// big-endian bytes, y = sqrt(x^3 + b) by the power (p - 3) / 4 (p = 3 mod 4; in Fp2 two of them, through the norm), the sign bit's choice of root, then the
// subgroup check and the encoder above.  Same verdicts as the host functions: kind 2 = bad encoding (compression bit missing, coordinate >= p, infinity
// bit on a string that is not C0 00 .. 00), 1 = x is not the abscissa of a curve point, 4 = outside the subgroup (k_subgroup_check).  A list fails with
// the verdict of its FIRST bad element, as a reader that decodes the elements in order does: every bad lane files index << 3 | kind under atomicMin.
FF_INLINE void first_failure(unsigned long long* first, uint64_t i, int kind) { atomicMin(first, (unsigned long long)(i << 3) | (unsigned long long)kind); }
__device__ static const uint32_t FP_ROOT_EXP[12] = {0xffffeaaau, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                                                    0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};      // (p - 3) / 4, 379 bits
__device__ static const uint32_t FP_HALF_PM1[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u,
                                                    0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};      // (p - 1) / 2
template <int A> FF_INLINE FpB<2> fp_red2(const FpB<A>& a) { return fe_mul(a, fp_one()); }          // the same value below 2 p
FF_INLINE FpB<2> fp_half() {                               // 1/2 = (p + 1) / 2, a constant: no inversion
    FpWords h;
#pragma unroll
    for (int k = 0; k < 12; k++) h.w[k] = FP_HALF_PM1[k];
    h.w[0] += 1;                                           // the low word of (p - 1) / 2 ends in ...d555: no carry
    return fp_to_mont(h);
}
FF_INLINE FpB<2> fp_select(bool c, const FpB<2>& a, const FpB<2>& b) {
    FpB<2> r;
#pragma unroll
    for (int i = 0; i < FPL; i++) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
}
// THE power of the square roots: a^((p - 3) / 4).  The exponent is a constant, every lane takes the same branches.  With w = a^((p - 3) / 4):
//   w a = a^((p + 1) / 4), a square root of a when a is a square (p = 3 mod 4);   w^2 a = a^((p - 1) / 2), the quadratic character of a;
//   w = 1 / (w a) when that character is 1 -- the inverse of the root comes with the root.
__device__ __noinline__ FpB<2> fp_pow_root(const FpB<2>& a) {
    FpB<2> acc = a;                                        // bit 378
    for (int i = 377; i >= 0; i--) {
        acc = fe_sqr(acc);
        if ((FP_ROOT_EXP[i >> 5] >> (i & 31)) & 1u) acc = fe_mul(acc, a);
    }
    return acc;
}
FF_INLINE bool fp_sqrt_dev(FpB<2>& out, const FpB<2>& a) {          // one power
    out = fe_mul(fp_pow_root(a), a);
    return fe_eq(fe_sqr(out), a);
}
template <int A> FF_INLINE bool fp_is_large(const FpB<A>& y) {          // canonical integer of y > (p - 1) / 2: the ZCash sign of a coordinate
    const FpWords w = fp_from_mont(y);
    bool gt = false, decided = false;
#pragma unroll
    for (int k = 11; k >= 0; k--)
        if (!decided && w.w[k] != FP_HALF_PM1[k]) { gt = w.w[k] > FP_HALF_PM1[k]; decided = true; }
    return gt;
}
// "is this y the larger one of y, -y": the ZCash sign of a point.  Fp: the canonical integer above (p - 1) / 2.  Fp2: the same question put to the
// imaginary part, and to the real part when the imaginary part is zero.  The decompression kernels and zk_selftest_sqrt both decide here.
FF_INLINE bool y_is_larger(const FpB<2>& y) { return fp_is_large(y); }
FF_INLINE bool y_is_larger(const Fp2B<2>& y) { return fe_is_zero(y.c1) ? fp_is_large(y.c0) : fp_is_large(y.c1); }
// a square root of a in Fp2 = Fp[u] / (u^2 + 1) (either one: the caller fixes the sign); false: a is not a square.  TWO powers, one after the other,
// no inversion, and no branch on data stands around either power: what depends on a is chosen among computed values.
//   a1 != 0:  n = a0^2 + a1^2,  s = n^((p + 1) / 4)  (s^2 = n when a is a square: its norm is one),  t = (a0 + s) / 2,  w = t^((p - 3) / 4),
//             chi = w^2 t.  chi = 1: sqrt(t) = w t and 1 / sqrt(t) = w, the root is (w t, a1 w / 2).  chi = -1: (w t)^2 = -t, and
//             (a1 w / 2)^2 - (w t)^2 = (4 t^2 - a1^2) / (4 t) = a0,  2 (a1 w / 2)(-w t) = a1: the root is (a1 w / 2, -w t).
//   a1 == 0:  the first power runs on a0 instead of n: w a0 is a root of a0 (character 1: the root is real) or of -a0 (the root is (w a0) u).  The
//             second power runs all the same and its result is dropped.
// Whatever went wrong on the way -- n no square, t = 0 -- shows in the last line: root^2 == a.
FF_INLINE bool fp2_sqrt_dev(Fp2B<2>& out, const Fp2B<2>& a) {
    const bool real = fe_is_zero(a.c1);
    const FpB<2> in1 = fp_select(real, a.c0, fp_red2(fe_add(fe_sqr(a.c0), fe_sqr(a.c1))));
    const FpB<2> w1 = fp_pow_root(in1);
    const FpB<2> s = fe_mul(w1, in1);
    const FpB<2> half = fp_half();
    const FpB<2> t = fe_mul(fe_add(a.c0, s), half);
    const FpB<2> w2 = fp_pow_root(t);
    if (real) {
        if (fe_eq(fe_mul(fe_sqr(w1), a.c0), fp_one())) out = {s, fp_zero()};
        else out = {fp_zero(), s};
    } else {
        const FpB<2> wt = fe_mul(w2, t), other = fe_mul(fe_mul(a.c1, w2), half);
        if (fe_eq(fe_mul(fe_sqr(w2), t), fp_one())) out = {wt, other};
        else out = {other, fp_red2(fe_neg(wt))};
    }
    const Fp2B<4> sq = fe_sqr(out);
    return fe_eq(sq.c0, a.c0) && fe_eq(sq.c1, a.c1);
}
// THE decompressor, one per group: the 48 / 96 wire bytes of a point (xb, a 16-byte aligned copy the function may overwrite) -> the affine point
// (the identity when rejected) and its kind, 0 good | 2 bad encoding | 1 the abscissa is on no curve point.  The flag rules stand here and nowhere
// else: the list kernels (k_decompress_*, which file the first failure of a list) and the verifiers' verdict kernel (k_decompress_verdict) call it.
FF_INLINE uint8_t point_decompress(Aff<Fp>& out, uint8_t* xb) {
    const uint8_t f0 = xb[0];
    out = aff_inf<Fp>();
    if (!(f0 & 0x80)) return 2;
    if (f0 & 0x40) return canonical_infinity(xb, 48, 0xC0) ? 0 : 2;
    xb[0] &= 0x1f;
    const FpWords xw = fpw_from_be(xb);
    if (!fpw_canonical(xw)) return 2;
    const FpB<2> x = fp_to_mont(xw);
    const FpB<2> rhs = fp_red2(fe_add(fe_mul(fe_sqr(x), x), FieldOps<Fp>::curve_b()));
    FpB<2> y;
    if (!fp_sqrt_dev(y, rhs)) return 1;
    if (y_is_larger(y) != ((f0 & 0x20) != 0)) y = fp_red2(fe_neg(y));
    out = {x, y};
    return 0;
}
FF_INLINE uint8_t point_decompress(Aff<Fp2>& out, uint8_t* xb) {          // xb: x.c1 (with the flags) | x.c0
    const uint8_t f0 = xb[0];
    out = aff_inf<Fp2>();
    if (!(f0 & 0x80)) return 2;
    if (f0 & 0x40) return canonical_infinity(xb, 96, 0xC0) ? 0 : 2;
    xb[0] &= 0x1f;
    const FpWords x1w = fpw_from_be(xb), x0w = fpw_from_be(xb + 48);
    if (!fpw_canonical(x1w) || !fpw_canonical(x0w)) return 2;
    const Fp2B<2> x = {fp_to_mont(x0w), fp_to_mont(x1w)};
    const auto cube = fe_mul(fe_sqr(x), x);
    const Fp2 b = FieldOps<Fp2>::curve_b();
    const Fp2B<2> rhs = {fp_red2(fe_add(cube.c0, b.c0)), fp_red2(fe_add(cube.c1, b.c1))};
    Fp2B<2> y;
    if (!fp2_sqrt_dev(y, rhs)) return 1;
    if (y_is_larger(y) != ((f0 & 0x20) != 0)) y = {fp_red2(fe_neg(y.c0)), fp_red2(fe_neg(y.c1))};
    out = {Fp2(x), Fp2(y)};
    return 0;
}
// the point's wire bytes (a multiple of 16, at a 16-byte aligned address) -> the lane's copy
template <int BYTES> FF_INLINE void wire_load(uint8_t* xb, const uint8_t* __restrict__ src) {
#pragma unroll
    for (int k = 0; k < BYTES / 16; k++) reinterpret_cast<uint4*>(xb)[k] = reinterpret_cast<const uint4*>(src)[k];
}
// a list of compressed points: dense affine out, and the list's first failure
template <class F> __global__ __launch_bounds__(128) void k_decompress(uint8_t* __restrict__ dense, const uint8_t* __restrict__ in, uint64_t n, unsigned long long* first) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int CB = FieldOps<F>::WORDS * 4, B = FieldOps<F>::WORDS * 8;
    alignas(16) uint8_t xb[CB];
    wire_load<CB>(xb, in + (size_t)CB * i);
    Aff<F> out;
    const uint8_t kind = point_decompress(out, xb);
    if (kind) first_failure(first, i, kind);
    aff_store<F>(dense + (size_t)B * i, out);
}
// The way back (to_compressed_bytes, curve.ml:213-219): a dense affine list -> wire bytes, one lane per point.  Out of Montgomery form, x big-endian
// (G2: x.c1 | x.c0), the sign bit by y_is_larger -- the rule the decompressor reads it by -- and C0 00 .. 00 for the identity; 16-byte stores.
FF_INLINE void wire_encode(uint8_t* xb, const Aff<Fp>& a) { fpw_to_be(xb, fp_from_mont(a.x)); }
FF_INLINE void wire_encode(uint8_t* xb, const Aff<Fp2>& a) {
    fpw_to_be(xb, fp_from_mont(a.x.c1));
    fpw_to_be(xb + 48, fp_from_mont(a.x.c0));
}
FF_INLINE bool wire_sign(const Aff<Fp>& a) { return y_is_larger(fp_red2(a.y)); }
FF_INLINE bool wire_sign(const Aff<Fp2>& a) { return y_is_larger(Fp2B<2>{fp_red2(a.y.c0), fp_red2(a.y.c1)}); }
template <class F> __global__ __launch_bounds__(128) void k_compress(uint8_t* __restrict__ out, const uint8_t* __restrict__ dense, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int CB = FieldOps<F>::WORDS * 4, B = FieldOps<F>::WORDS * 8;
    const Aff<F> a = aff_load<F>(dense + (size_t)B * i);
    alignas(16) uint8_t xb[CB];
    if (aff_is_inf(a)) {
#pragma unroll
        for (int k = 0; k < CB / 16; k++) reinterpret_cast<uint4*>(xb)[k] = make_uint4(0, 0, 0, 0);
        xb[0] = 0xC0;
    } else {
        wire_encode(xb, a);
        xb[0] |= wire_sign(a) ? 0xA0 : 0x80;
    }
#pragma unroll
    for (int k = 0; k < CB / 16; k++) reinterpret_cast<uint4*>(out + (size_t)CB * i)[k] = reinterpret_cast<const uint4*>(xb)[k];
}
// The verifiers' form (verify_resident.hip): `per` points of every item -- a proof -- read where they lie in the item's wire bytes, point q of item j
// at in + stride j + off[q], into the dense list dense[per j + q] with one verdict byte each.  Strides and offsets are multiples of 16.
struct WireSlots {
    uint32_t per, stride;
    uint32_t off[6];
};
template <class F> __global__ __launch_bounds__(128) void k_decompress_verdict(uint8_t* __restrict__ dense, const uint8_t* __restrict__ in, uint64_t n, WireSlots w,
                                                                              uint8_t* __restrict__ verdict) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int CB = FieldOps<F>::WORDS * 4, B = FieldOps<F>::WORDS * 8;
    const uint64_t item = i / w.per;
    alignas(16) uint8_t xb[CB];
    wire_load<CB>(xb, in + (size_t)w.stride * item + w.off[i - item * w.per]);
    Aff<F> out;
    verdict[i] = point_decompress(out, xb);
    aff_store<F>(dense + (size_t)B * i, out);
}
// The provers' form (zk_*_prove_many_compressed; ProofWire, msm.cuh): the XYZZ sums of a whole batch of proofs -> the proofs' wire records, one lane per
// point.  xyzz_to_aff without its early exit: the inversion is the lockstep one (fp_inv.cuh), 0 for 0, so a lane that holds the identity runs the same
// instructions as its neighbours and ends with x = y = 0; what it writes is chosen at the end.  The point's slot in the record comes out of the
// argument struct by a chain of selects over constant indices, the lane's bytes are written at constant indices: nothing is indexed at run time.
template <class F> FF_INLINE Aff<F> xyzz_to_aff_lockstep(const Xyzz<F>& p) {
    const auto i = fe_inv(fe_mul(p.zz, p.zzz));
    const auto izz = fe_mul(i, p.zzz);
    const auto izzz = fe_mul(i, p.zz);
    return {fe_mul(p.x, izz), fe_mul(p.y, izzz)};
}
template <class F> __global__ __launch_bounds__(128) void k_proofs_to_wire(uint8_t* __restrict__ out, const uint8_t* __restrict__ rows, uint64_t n, ProofWire w) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int CB = FieldOps<F>::WORDS * 4, XB = FieldOps<F>::WORDS * 16;
    const uint64_t item = i / w.per;
    const uint32_t q = (uint32_t)(i - item * w.per);
    uint32_t off = w.off[0];
#pragma unroll
    for (int k = 1; k < 6; k++) off = q == (uint32_t)k ? w.off[k] : off;
    const Xyzz<F> p = xyzz_load<F>(rows + (size_t)w.row_stride * item + w.row_first + (size_t)XB * q);
    const bool inf = xyzz_is_inf(p);
    const Aff<F> a = xyzz_to_aff_lockstep(p);
    alignas(16) uint8_t xb[CB];
    wire_encode(xb, a);
    xb[0] |= wire_sign(a) ? 0xA0 : 0x80;
    uint4* dst = reinterpret_cast<uint4*>(out + (size_t)w.wire_stride * item + off);
#pragma unroll
    for (int k = 0; k < CB / 16; k++) {
        const uint4 v = reinterpret_cast<const uint4*>(xb)[k];
        dst[k] = inf ? make_uint4(k == 0 ? 0xC0u : 0u, 0u, 0u, 0u) : v;
    }
}
// zk_selftest_proof_wire: (x, y) in the ABI's uncompressed bytes and a scalar z -> the XYZZ point (x z^2, y z^3, z^2, z^3) as a one-point row of
// k_proofs_to_wire; the all-zero pair -> the identity (zz = 0).  bit 0 of *flag: a coordinate >= p, z = 0 or z >= r.
FF_INLINE bool lift_xy(Aff<Fp>& a, const uint8_t* p) {
    const FpWords x = fpw_from_be(p), y = fpw_from_be(p + 48);
    a = {fp_to_mont(x), fp_to_mont(y)};
    return fpw_canonical(x) && fpw_canonical(y);
}
FF_INLINE bool lift_xy(Aff<Fp2>& a, const uint8_t* p) {
    const FpWords x1 = fpw_from_be(p), x0 = fpw_from_be(p + 48), y1 = fpw_from_be(p + 96), y0 = fpw_from_be(p + 144);
    a = {{fp_to_mont(x0), fp_to_mont(x1)}, {fp_to_mont(y0), fp_to_mont(y1)}};
    return fpw_canonical(x0) && fpw_canonical(x1) && fpw_canonical(y0) && fpw_canonical(y1);
}
FF_INLINE Xyzz<Fp> lift_scale(const Aff<Fp>& a, const FpB<2>& zz, const FpB<2>& zzz) { return {fe_mul(a.x, zz), fe_mul(a.y, zzz), zz, zzz}; }
FF_INLINE Xyzz<Fp2> lift_scale(const Aff<Fp2>& a, const FpB<2>& zz, const FpB<2>& zzz) {
    return {{fe_mul(a.x.c0, zz), fe_mul(a.x.c1, zz)}, {fe_mul(a.y.c0, zzz), fe_mul(a.y.c1, zzz)}, {zz, fp_zero()}, {zzz, fp_zero()}};
}
template <class F> __global__ __launch_bounds__(128) void k_selftest_lift(uint8_t* __restrict__ xyzz, const uint8_t* __restrict__ aff, const uint32_t* __restrict__ z, uint64_t n, int* flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = FieldOps<F>::WORDS * 8;
    const Fr zr = fe_load<FrParams>(z + 8 * i);
    FpWords zw;
#pragma unroll
    for (int k = 0; k < 12; k++) zw.w[k] = k < 8 ? z[8 * i + k] : 0u;
    Aff<F> a;
    const bool ok = lift_xy(a, aff + (size_t)B * i);
    if (!ok || !fe_is_canonical(zr) || fe_is_zero(zr)) atomicOr(flag, 1);
    const FpB<2> zf = fp_to_mont(zw), zz = fe_mul(zf, zf), zzz = fe_mul(zz, zf);
    xyzz_store<F>(xyzz + (size_t)2 * B * i, aff_is_inf(a) ? xyzz_inf<F>() : lift_scale(a, zz, zzz));
}

// zk_selftest_sqrt: the square roots and the sign rule above on bare field elements, one lane per element, as k_decompress_* call them.
// field 0: 48 B big-endian each; field 1: 96 B each, imaginary part | real part (the order of a G2 coordinate on the wire).  root = the root that
// y_is_larger calls the larger one (zeros when a is not a square), is_square = 1 / 0.  An element >= p sets *flag.
__global__ __launch_bounds__(128) void k_selftest_sqrt(uint8_t* __restrict__ root, uint8_t* __restrict__ is_square, const uint8_t* __restrict__ in, uint64_t n,
                                                       int field, int* flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int B = field ? 96 : 48;
    alignas(16) uint8_t ab[96], rb[96];
    for (int k = 0; k < B; k++) { ab[k] = in[B * i + k]; rb[k] = 0; }
    bool sq = false;
    if (!field) {
        const FpWords aw = fpw_from_be(ab);
        if (!fpw_canonical(aw)) atomicOr(flag, 2);
        else {
            FpB<2> y;
            sq = fp_sqrt_dev(y, fp_to_mont(aw));
            if (sq) {
                if (!y_is_larger(y)) y = fp_red2(fe_neg(y));
                fpw_to_be(rb, fp_from_mont(y));
            }
        }
    } else {
        const FpWords a1w = fpw_from_be(ab), a0w = fpw_from_be(ab + 48);
        if (!fpw_canonical(a1w) || !fpw_canonical(a0w)) atomicOr(flag, 2);
        else {
            Fp2B<2> y;
            sq = fp2_sqrt_dev(y, Fp2B<2>{fp_to_mont(a0w), fp_to_mont(a1w)});
            if (sq) {
                if (!y_is_larger(y)) y = {fp_red2(fe_neg(y.c0)), fp_red2(fe_neg(y.c1))};
                fpw_to_be(rb, fp_from_mont(y.c1));
                fpw_to_be(rb + 48, fp_from_mont(y.c0));
            }
        }
    }
    for (int k = 0; k < B; k++) root[B * i + k] = rb[k];
    is_square[i] = sq ? 1 : 0;
}

// ------------------------------------------------------------------ prime-order subgroup membership: two tests, one answer
// The reference's points come from Bls12_381.G1/G2.of_bytes_exn / of_compressed_bytes_exn (curve.ml:199-212), which raise on a point of the curve
// that lies outside the r-torsion; a point uploaded to the library as raw bytes gets the same treatment here.  Each test (SubgroupTest, msm.cuh) is ONE
// device function that takes an affine point of the curve that is not the identity and answers "in the subgroup"; the kernels below add only their way
// of reporting.
// ---- SUBGROUP_ORDER: [r] P = O.  Plain double-and-add over the bits of r (a compile-time constant: the branch is wave-uniform), out-of-line group
// operations: ~255 doublings + 127 additions per point, 0.3 s of a 2^20 key.
__device__ static const uint32_t FR_ORDER_BITS[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
template <class F> FF_INLINE bool in_subgroup_order(const Aff<F>& p) {
    Xyzz<F> acc = xyzz_from_aff(p);                      // the top bit (254) of r
    for (int b = 253; b >= 0; b--) {
        acc = xyzz_dbl(acc);
        if ((FR_ORDER_BITS[b >> 5] >> (b & 31)) & 1u) xyzz_madd(acc, p);
    }
    return xyzz_is_inf(acc);
}
// ---- SUBGROUP_ENDO: the same answer by the curve's endomorphisms (the resident verification keys of verify_resident.hip)
// [r] P = O costs 254 doublings and 127 additions.  Both groups have an endomorphism that acts on the r-torsion as a SHORT scalar, and the curve
// points on which it acts as that scalar are exactly the subgroup (z = -0xd201000000010000, r = z^4 - z^2 + 1):
//   G1:  phi(x, y) = (beta x, y) = [z^2 - 1] P.   phi^2 + phi + 1 = 0 on the whole curve, so phi(P) + P = -phi^2(P) = (beta^2 x, -y):
//        P in G1  <=>  [z^2] P == (beta^2 x, -y).   Two chains over |z|: 2 x (63 doublings + 5 additions).
//   G2:  psi(x, y) = (cx conj x, cy conj y) = [z] Q.   Q in G2  <=>  [|z|] Q == -psi(Q): one chain.  (ENDO_PSI_X[0], ENDO_PSI_Y[0]) of
//        endo_consts.cuh IS -psi: the generator folds the sign of the odd digit terms into the y constant.
// tests/test_subgroup_criterion.py restates both in integers with these constants and holds them to [r] P = O on points of every prime-power order
// the cofactors allow.  The chain is short, so it meets what a 255-bit chain over a point of order r never meets: on a point of order 3 the
// accumulator is +-P at an addition step, on points of order 11, 13 or 23 it passes through the identity mid-chain.  xyzz_dbl and xyzz_madd / xyzz_add
// are the complete operations of ec.cuh (identity operands, P + P, P - P); neither cofactor is even, so no point has y = 0.
// The comparison is projective (X == x' ZZ, Y == y' ZZZ): no inversion.
static constexpr uint64_t BLS_Z_ABS = 0xd201000000010000ull;          // |z|: 64 bits, Hamming weight 6
FF_INLINE FpB<1> endo_const(const uint32_t* __restrict__ c) {
    FpB<1> r;
#pragma unroll
    for (int i = 0; i < FPL; i++) r.v[i] = c[i];
    return r;
}
// [|z|] p, p affine and not the identity
template <class F> FF_INLINE Xyzz<F> mul_z_aff(const Aff<F>& p) {
    Xyzz<F> acc = xyzz_from_aff(p);                      // bit 63
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        acc = xyzz_dbl(acc);
        if ((BLS_Z_ABS >> b) & 1u) xyzz_madd(acc, p);          // a compile-time constant: wave-uniform
    }
    return acc;
}
// [|z|] q, q in XYZZ (the second chain of G1)
template <class F> FF_INLINE Xyzz<F> mul_z_xyzz(const Xyzz<F>& q) {
    Xyzz<F> acc = q;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        acc = xyzz_dbl(acc);
        if ((BLS_Z_ABS >> b) & 1u) xyzz_add(acc, q);
    }
    return acc;
}
FF_INLINE bool in_subgroup_endo(const Aff<Fp>& p) {
    const Xyzz<Fp> t = mul_z_xyzz(mul_z_aff(p));         // [z^2] P
    if (xyzz_is_inf(t)) return false;                    // (beta^2 x, -y) is a point of the curve, never the identity
    const FpB<2> beta2 = fe_sqr(endo_const(ENDO_BETA));
    return fe_eq(t.x, fe_mul(fe_mul(beta2, p.x), t.zz)) && fe_eq(t.y, fe_mul(fe_neg(p.y), t.zzz));
}
FF_INLINE bool in_subgroup_endo(const Aff<Fp2>& q) {
    const Xyzz<Fp2> t = mul_z_aff(q);                    // [|z|] Q
    if (xyzz_is_inf(t)) return false;
    const Fp2B<1> cx = {endo_const(ENDO_PSI_X[0][0]), endo_const(ENDO_PSI_X[0][1])}, cy = {endo_const(ENDO_PSI_Y[0][0]), endo_const(ENDO_PSI_Y[0][1])};
    const Fp2B<128> xc = {q.x.c0, fe_neg(q.x.c1)}, yc = {q.y.c0, fe_neg(q.y.c1)};          // conjugates
    return fe_eq(t.x, fe_mul(fe_mul(cx, xc), t.zz)) && fe_eq(t.y, fe_mul(fe_mul(cy, yc), t.zzz));
}
template <SubgroupTest T, class F> FF_INLINE bool in_subgroup(const Aff<F>& p) {
    static_assert(T == SUBGROUP_ORDER || T == SUBGROUP_ENDO, "SUBGROUP_NONE launches no kernel");
    if constexpr (T == SUBGROUP_ENDO) return in_subgroup_endo(p);
    else return in_subgroup_order(p);
}
// The kernels read `dense` (affine, on the curve; a point the decoder rejected is stored as the identity and skipped) and report in their caller's way:
// one flag word per list, bit 4, plus -- `first` may be null -- the list readers' first-failure word of k_decompress_* ...
template <class F, SubgroupTest T> __global__ __launch_bounds__(128) void k_subgroup_check(const uint8_t* __restrict__ dense, uint64_t n, int* flag, unsigned long long* first) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = FieldOps<F>::WORDS * 8;
    const Aff<F> p = aff_load<F>(dense + B * i);
    if (aff_is_inf(p)) return;
    if (!in_subgroup<T>(p)) {
        atomicOr(flag, 4);
        if (first) atomicMin(first, (unsigned long long)(i << 3) | 4ull);
    }
}
// ... or verdict[i] = 4 next to the decoder's verdict bytes; other verdicts stay
template <class F, SubgroupTest T> __global__ __launch_bounds__(128) void k_subgroup_verdict(const uint8_t* __restrict__ dense, uint64_t n, uint8_t* verdict) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = FieldOps<F>::WORDS * 8;
    const Aff<F> p = aff_load<F>(dense + B * i);
    if (aff_is_inf(p)) return;
    if (!in_subgroup<T>(p)) verdict[i] = 4;
}

// ------------------------------------------------------------------ base tables: table[j*n + i] = 2^(c*j) * P_i, j < nw
// `dense` holds the n base points in the dense affine format (what the key arrived as); the table takes them -- and with nw > 1 their
// multiples by 2^(c j) -- in the 128-byte record layout of ec.cuh (TableLayout).
template <class F> __global__ void k_precompute(uint8_t* table, const uint8_t* __restrict__ dense, uint64_t n, uint32_t c, uint32_t nw) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = FieldOps<F>::WORDS * 8, TB = TableLayout<F>::ENTRY;
    Aff<F> p = aff_load<F>(dense + B * i);
    tab_store(table + TB * i, p);
    for (uint32_t j = 1; j < nw; j++) {
        Xyzz<F> q = xyzz_dbl_aff(p);
        for (uint32_t k = 1; k < c; k++) q = xyzz_dbl(q);
        p = xyzz_to_aff(q);
        tab_store(table + TB * ((uint64_t)j * n + i), p);
    }
}
// window 0 of a table back in the dense affine format (key derivation, re-sharding, zk_*_pool_points): exact -- the records hold canonical limbs
template <class F> __global__ void k_table_to_dense(uint8_t* __restrict__ dense, const uint8_t* __restrict__ table, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = FieldOps<F>::WORDS * 8, TB = TableLayout<F>::ENTRY;
    aff_store<F>(dense + B * i, tab_load((const F*)nullptr, table + TB * i));
}

// flags[i] = 1 iff base i is the identity (its table entries 2^(cj) P are the identity for every window, and only those:
// neither curve has points of even order)
template <class F> __global__ void k_ident_flags(uint8_t* flags, const uint8_t* dense, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = FieldOps<F>::WORDS * 8;
    const uint4* q = reinterpret_cast<const uint4*>(dense + B * i);
    uint32_t o = 0;
    for (int k = 0; k < B / 16; k++) { const uint4 x = q[k]; o |= x.x | x.y | x.z | x.w; }
    flags[i] = o == 0 ? 1 : 0;
}

// acc[i] = sum_j parts[j * npoints + i] on dense XYZZ points: the sum of the ranks' / devices' partial sums of a proof.  One lane per point in G1, a lane PAIR
// in G2 (F = Fp2H), additions expanded in place on the lane's registers: round 3's form (a whole Fp2 point per lane through the out-of-line addition)
// carried 3 KiB of private memory per lane -- 1.6 GiB of scratch reserved on every queue the kernel was dispatched on (DESIGN A.2).
template <class F> __global__ __launch_bounds__(64) void k_xyzz_sum_columns(uint8_t* out, const uint8_t* parts, uint32_t count, uint32_t npoints) {
    constexpr int XB = FieldOps<F>::WORDS * 16;          // dense XYZZ bytes of one point: 192 (G1) / 384 (G2: FieldOps<Fp2H> keeps Fp2's memory layout)
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) / RawLayout<F>::LANES;
    if (i >= npoints) return;          // both lanes of a pair together
    Xyzz<F> acc = xyzz_inf<F>();
    for (uint32_t j = 0; j < count; j++) {
        const Xyzz<F> q = xyzz_load<F>(parts + (uint64_t)XB * ((uint64_t)j * npoints + i));
        xyzz_add_impl(acc, q);
    }
    xyzz_store<F>(out + (uint64_t)XB * i, acc);
}

// ------------------------------------------------------------------ fixed-base: out[i] = s_i * G
// pow2[k] = 2^k * G (affine), 256 entries per curve, built once by 256 lanes.
template <class F> FF_INLINE Aff<F> generator();
template <> FF_INLINE Aff<Fp> generator<Fp>() {
    // canonical generator coordinates as little-endian words, converted to Montgomery
    const FpWords x = {{0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu,
                        0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u}};
    const FpWords y = {{0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu,
                        0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u}};
    return {fp_to_mont(x), fp_to_mont(y)};
}
template <> FF_INLINE Aff<Fp2> generator<Fp2>() {
    const FpWords x0 = {{0xc121bdb8u, 0xd48056c8u, 0xa805bbefu, 0x0bac0326u, 0x7ae3d177u, 0xb4510b64u,
                         0xfa403b02u, 0xc6e47ad4u, 0x2dc51051u, 0x26080527u, 0xf08f0a91u, 0x024aa2b2u}};
    const FpWords x1 = {{0x5d042b7eu, 0xe5ac7d05u, 0x13945d57u, 0x334cf112u, 0xdc7f5049u, 0xb5da61bbu,
                         0x9920b61au, 0x596bd0d0u, 0x88274f65u, 0x7dacd3a0u, 0x52719f60u, 0x13e02b60u}};
    const FpWords y0 = {{0x08b82801u, 0xe1935486u, 0x3baca289u, 0x923ac9ccu, 0x5160d12cu, 0x6d429a69u,
                         0x8cbdd3a7u, 0xadfd9baau, 0xda2e351au, 0x8cc9cdc6u, 0x727d6e11u, 0x0ce5d527u}};
    const FpWords y1 = {{0xf05f79beu, 0xaaa9075fu, 0x5cec1da1u, 0x3f370d27u, 0x572e99abu, 0x267492abu,
                         0x85a763afu, 0xcb3e287eu, 0x2bc28b99u, 0x32acd2b0u, 0x2ea734ccu, 0x0606c4a0u}};
    return {{fp_to_mont(x0), fp_to_mont(x1)}, {fp_to_mont(y0), fp_to_mont(y1)}};
}
template <class F> __global__ void k_gen_pow2_table(uint8_t* table) {
    constexpr int AB = FieldOps<F>::WORDS * 8;
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 256) return;
    Aff<F> g = generator<F>();
    Xyzz<F> q = xyzz_from_aff(g);
    for (uint32_t i = 0; i < k; i++) q = xyzz_dbl(q);
    aff_store<F>(table + AB * k, xyzz_to_aff(q));
}
template <class F>
__global__ __launch_bounds__(128) void k_fixed_base_mul(uint8_t* __restrict__ out, const uint32_t* __restrict__ scalars,
                                                        uint64_t n, const uint8_t* __restrict__ pow2) {
    constexpr int AB = FieldOps<F>::WORDS * 8;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Xyzz<F> acc = xyzz_inf<F>();
    for (uint32_t w = 0; w < 8; w++) {
        uint32_t bits = scalars[8 * i + w];
        while (bits) {
            uint32_t b = __builtin_ctz(bits);
            bits &= bits - 1;
            Aff<F> p = aff_load<F>(pow2 + AB * (32 * w + b));
            xyzz_madd(acc, p);
        }
    }
    aff_store<F>(out + AB * i, xyzz_to_aff(acc));
}
// ================================================================== host side
// THE place a Curve becomes a field type: fn(FieldTag<Fp>{}) for G1, fn(FieldTag<Fp2>{}) for G2, for launches whose two arms differ in the field alone
template <class F> struct FieldTag { using type = F; };
template <class Fn> static void for_curve(Curve curve, Fn&& fn) {
    if (curve == CURVE_G1) fn(FieldTag<Fp>{});
    else fn(FieldTag<Fp2>{});
}
#define FIELD_OF(tag) typename decltype(tag)::type
template <class F> static int bases_finish(MsmBases& b, const void* d_dense, hipStream_t s) {
    // every base set carries its identity flags: the sort never files an identity base into a bucket, so the accumulate loop can take table
    // entries for genuine points (no identity test per addition) in BOTH table modes
    ZKCHK(b.ident.alloc(b.n));
    hipLaunchKernelGGL(k_ident_flags<F>, grid_for(b.n, 256), dim3(256), 0, s, b.ident.as<uint8_t>(), (const uint8_t*)d_dense, b.n);
    ScopedTimer t("msm_precompute", s);
    hipLaunchKernelGGL(k_precompute<F>, grid_for(b.n, 64), dim3(64), 0, s, b.table.as<uint8_t>(), (const uint8_t*)d_dense, b.n, b.c, b.precomp ? b.nw : 1u);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
size_t table_entry_bytes(Curve c) { return c == CURVE_G1 ? TableLayout<Fp>::ENTRY : TableLayout<Fp2>::ENTRY; }
int msm_bases_dense(const MsmBases& b, uint64_t lo, uint64_t count, void* d_dense, hipStream_t s) {
    if (lo + count > b.n) ZK_FAIL(ZK_ERR_ARG, "msm_bases_dense: range outside the base set");
    if (!count) return ZK_OK;
    const uint8_t* src = b.table.as<uint8_t>() + table_entry_bytes(b.curve) * lo;
    for_curve(b.curve, [&](auto f) { hipLaunchKernelGGL(k_table_to_dense<FIELD_OF(f)>, grid_for(count, 128), dim3(128), 0, s, (uint8_t*)d_dense, src, count); });
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
static int bases_setup(MsmBases& b, Curve curve, uint64_t n, uint32_t c, bool precomp, bool in_subgroup) {
    if (n == 0) ZK_FAIL(ZK_ERR_ARG, "msm: empty base set");
    if (c == 0) {
        c = (uint32_t)opt_int(OPT_MSM_WINDOW, (int)msm_auto_window(n, precomp));         // window-size sweeps (BASELINE config 3); key set-up, not a per-proof path
    }
    if (c < 2 || c > 22) ZK_FAIL(ZK_ERR_ARG, "msm: window_bits must be in [2, 22]");
    b.curve = curve; b.n = n; b.c = c; b.precomp = precomp; b.in_subgroup = in_subgroup; b.fold = msm_fold(c, precomp, in_subgroup); b.nw = msm_windows(c, b.fold);
    if ((precomp ? (uint64_t)b.nw : 1) * n >= ((uint64_t)1 << 31)) ZK_FAIL(ZK_ERR_ARG, "msm: too many points for 31-bit references");
    return b.table.alloc(table_entry_bytes(curve) * n * (precomp ? b.nw : 1));
}
int points_bytes_to_affine(Curve curve, void* d_aff, const void* d_bytes, uint64_t n, int* d_flag, hipStream_t s) {
    if (!n) return ZK_OK;
    for_curve(curve, [&](auto f) { hipLaunchKernelGGL(k_bytes_to_affine<FIELD_OF(f)>, grid_for(n, 128), dim3(128), 0, s, (uint8_t*)d_aff, (const uint8_t*)d_bytes, n, d_flag); });
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
int points_subgroup_verdicts(Curve curve, const void* d_aff, uint64_t n, uint8_t* d_verdict, SubgroupTest test, hipStream_t s) {
    if (!n) return ZK_OK;
    for_curve(curve, [&](auto f) {
        using F = FIELD_OF(f);
        const dim3 grid = grid_for(n, 128);
        if (test == SUBGROUP_ORDER) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_subgroup_verdict<F, SUBGROUP_ORDER>), grid, dim3(128), 0, s, (const uint8_t*)d_aff, n, d_verdict);
        if (test == SUBGROUP_ENDO) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_subgroup_verdict<F, SUBGROUP_ENDO>), grid, dim3(128), 0, s, (const uint8_t*)d_aff, n, d_verdict);
    });
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
int points_decode_verdicts(Curve curve, void* d_aff, const void* d_bytes, uint64_t n, uint8_t* d_verdict, SubgroupTest test, hipStream_t s) {
    if (!n) return ZK_OK;
    for_curve(curve, [&](auto f) {
        hipLaunchKernelGGL(k_bytes_to_affine_verdict<FIELD_OF(f)>, grid_for(n, 128), dim3(128), 0, s, (uint8_t*)d_aff, (const uint8_t*)d_bytes, n, d_verdict);
    });
    return points_subgroup_verdicts(curve, d_aff, n, d_verdict, test, s);
}
int points_decompress_verdicts(Curve curve, void* d_aff, const void* d_in, uint64_t items, uint32_t per, uint32_t stride, const uint32_t* off, uint8_t* d_verdict,
                               hipStream_t s) {
    if (!items || !per) return ZK_OK;
    if (per > 6 || stride % 16) ZK_FAIL(ZK_ERR_ARG, "points_decompress_verdicts: at most 6 points per item, at strides of 16 bytes");
    WireSlots w{per, stride, {}};
    for (uint32_t q = 0; q < per; q++) {
        if (off[q] % 16 || off[q] + aff_bytes(curve) / 2 > stride) ZK_FAIL(ZK_ERR_ARG, "points_decompress_verdicts: a point lies outside its item or off a 16-byte boundary");
        w.off[q] = off[q];
    }
    const uint64_t n = items * per;
    for_curve(curve, [&](auto f) {
        hipLaunchKernelGGL(k_decompress_verdict<FIELD_OF(f)>, grid_for(n, 128), dim3(128), 0, s, (uint8_t*)d_aff, (const uint8_t*)d_in, n, w, d_verdict);
    });
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// n1 G1 and n2 G2 points (host bytes) -> dense affine on the device (a1, a2: kept by the caller or dropped) + one verdict each on the host
int points_decode_two_lists(const uint8_t* g1, uint64_t n1, const uint8_t* g2, uint64_t n2, const char* family, SubgroupTest test, DevBuf& a1, DevBuf& a2,
                            std::vector<uint8_t>& v1, std::vector<uint8_t>& v2, hipStream_t s) {
    v1.assign(n1, 0);
    v2.assign(n2, 0);
    DevBuf b1, b2, dv;
    ZKCHK(b1.alloc(96 * n1));
    ZKCHK(b2.alloc(192 * n2));
    ZKCHK(a1.alloc(96 * n1));
    ZKCHK(a2.alloc(192 * n2));
    ZKCHK(dv.alloc(n1 + n2));
    if (n1) HIPCHK(hipMemcpyAsync(b1.p, g1, 96 * n1, hipMemcpyHostToDevice, s));
    if (n2) HIPCHK(hipMemcpyAsync(b2.p, g2, 192 * n2, hipMemcpyHostToDevice, s));
    {
        ScopedTimer t(family, s);
        ZKCHK(points_decode_verdicts(CURVE_G2, a2.p, b2.p, n2, dv.as<uint8_t>() + n1, test, s));
        ZKCHK(points_decode_verdicts(CURVE_G1, a1.p, b1.p, n1, dv.as<uint8_t>(), test, s));
    }
    if (n1) HIPCHK(hipMemcpyAsync(v1.data(), dv.p, n1, hipMemcpyDeviceToHost, s));
    if (n2) HIPCHK(hipMemcpyAsync(v2.data(), dv.as<uint8_t>() + n1, n2, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}
// zk_selftest_subgroup: n encoded points (host) -> n verdicts (host) through the subgroup test asked for
int points_selftest_subgroup(Curve curve, SubgroupTest test, const uint8_t* points, uint64_t n, uint8_t* verdict, hipStream_t s) {
    const size_t ab = aff_bytes(curve);
    DevBuf raw, aff, dv;
    ZKCHK(raw.alloc(ab * n));
    ZKCHK(aff.alloc(ab * n));
    ZKCHK(dv.alloc(n));
    HIPCHK(hipMemcpyAsync(raw.p, points, ab * n, hipMemcpyHostToDevice, s));
    ZKCHK(points_decode_verdicts(curve, aff.p, raw.p, n, dv.as<uint8_t>(), test, s));
    HIPCHK(hipMemcpyAsync(verdict, dv.p, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}
int points_affine_to_bytes(Curve curve, void* d_bytes, const void* d_aff, uint64_t n, hipStream_t s) {
    if (!n) return ZK_OK;
    for_curve(curve, [&](auto f) { hipLaunchKernelGGL(k_affine_to_bytes<FIELD_OF(f)>, grid_for(n, 128), dim3(128), 0, s, (uint8_t*)d_bytes, (const uint8_t*)d_aff, n); });
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
int points_xyzz_to_bytes_dev(Curve curve, const void* d_xyzz, uint64_t count, void* d_bytes, hipStream_t s) {
    for_curve(curve, [&](auto f) { hipLaunchKernelGGL(k_xyzz_to_bytes<FIELD_OF(f)>, grid_for(count, 64), dim3(64), 0, s, (uint8_t*)d_bytes, (const uint8_t*)d_xyzz, count); });
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
int proof_points_to_bytes_dev(const void* d_g1, uint32_t n1, const uint32_t* off1, const void* d_g2, uint32_t n2, const uint32_t* off2, void* d_out, hipStream_t s) {
    if (n1 > 8 || n2 > 4) ZK_FAIL(ZK_ERR_ARG, "proof_points_to_bytes_dev: at most 8 G1 and 4 G2 points");
    ProofOffsets off{};
    for (uint32_t i = 0; i < n1; i++) off.g1[i] = off1[i];
    for (uint32_t i = 0; i < n2; i++) off.g2[i] = off2[i];
    ScopedTimer t("proof_to_bytes", s);
    hipLaunchKernelGGL(k_proof_to_bytes, dim3(n1 + n2), dim3(64), 0, s, (const uint8_t*)d_g1, n1, (const uint8_t*)d_g2, off, (uint8_t*)d_out);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
int points_xyzz_to_bytes(Curve curve, const void* d_xyzz, uint64_t count, uint8_t* host_out, hipStream_t s) {
    DevBuf tmp;
    ZKCHK(tmp.alloc(aff_bytes(curve) * count));
    ZKCHK(points_xyzz_to_bytes_dev(curve, d_xyzz, count, tmp.p, s));
    HIPCHK(hipMemcpyAsync(host_out, tmp.p, aff_bytes(curve) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}
int msm_bases_from_device_affine(MsmBases& b, Curve curve, const void* d_affine, uint64_t n, uint32_t c, bool precomp, hipStream_t s, bool in_subgroup) {
    ZKCHK(bases_setup(b, curve, n, c, precomp, in_subgroup));
    return curve == CURVE_G1 ? bases_finish<Fp>(b, d_affine, s) : bases_finish<Fp2>(b, d_affine, s);
}
static void launch_subgroup_check(Curve curve, const void* d_dense, uint64_t n, int* d_flag, unsigned long long* d_first, hipStream_t s, SubgroupTest test = SUBGROUP_ORDER) {
    for_curve(curve, [&](auto f) {
        using F = FIELD_OF(f);
        const dim3 grid = grid_for(n, 128);
        if (test == SUBGROUP_ENDO) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_subgroup_check<F, SUBGROUP_ENDO>), grid, dim3(128), 0, s, (const uint8_t*)d_dense, n, d_flag, d_first);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_subgroup_check<F, SUBGROUP_ORDER>), grid, dim3(128), 0, s, (const uint8_t*)d_dense, n, d_flag, d_first);
    });
}
// n encoded points (host) -> dense affine (device), checked the way a key upload checks them: encoding, curve, and -- check_subgroup -- [r] P = O.
// The verdict of the list: ZK_ERR_ARG for an encoding, else ZK_ERR_NOT_ON_CURVE for a point off the curve or outside the subgroup.  Synchronises.
int points_from_bytes_checked(Curve curve, const uint8_t* host_bytes, uint64_t n, void* d_dense, bool check_subgroup, hipStream_t s) {
    DevBuf raw, flag;
    ZKCHK(raw.alloc(aff_bytes(curve) * n));
    ZKCHK(flag.alloc(4));
    HIPCHK(hipMemsetAsync(flag.p, 0, 4, s));
    HIPCHK(hipMemcpyAsync(raw.p, host_bytes, aff_bytes(curve) * n, hipMemcpyHostToDevice, s));
    ZKCHK(points_bytes_to_affine(curve, d_dense, raw.p, n, flag.as<int>(), s));
    if (check_subgroup) {
        ScopedTimer t("subgroup_check", s);
        launch_subgroup_check(curve, d_dense, n, flag.as<int>(), nullptr, s);
    }
    int h = 0;
    HIPCHK(hipMemcpyAsync(&h, flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h & 2) ZK_FAIL(ZK_ERR_ARG, "point encoding: compressed flag set or coordinate >= p");
    if (h & 1) ZK_FAIL(ZK_ERR_NOT_ON_CURVE, "a base point is not on the curve");
    if (h & 4) ZK_FAIL(ZK_ERR_NOT_ON_CURVE, "a key point is on the curve but outside the prime-order subgroup (of_bytes_exn, curve.ml:199-212)");
    return ZK_OK;
}
int msm_bases_from_bytes(MsmBases& b, Curve curve, const uint8_t* host_bytes, uint64_t n, uint32_t c, bool precomp, hipStream_t s, bool check_subgroup) {
    ZKCHK(bases_setup(b, curve, n, c, precomp, check_subgroup));      // folded digits only for points the [r] P = O test has passed
    DevBuf dense;
    ZKCHK(dense.alloc(aff_bytes(curve) * n));
    ZKCHK(points_from_bytes_checked(curve, host_bytes, n, dense.p, check_subgroup, s));
    ZKCHK((curve == CURVE_G1 ? bases_finish<Fp>(b, dense.p, s) : bases_finish<Fp2>(b, dense.p, s)));
    HIPCHK(hipStreamSynchronize(s));          // `dense` is released on return: the table build has read it
    return ZK_OK;
}

// ---- key points and MSM bases from their WIRE bytes (zk_*_pk_upload_compressed, zk_bases_upload_compressed): 48 / 96 B per point up, THE decompressor
// straight into the dense list the table build reads, the endomorphism subgroup test, 8 bytes back.  No byte re-encoding, no point travels down.
// *first: index << 3 | kind of the list's first bad point (kind 2 encoding, 1 curve, 4 subgroup), all ones = none.  Synchronises.
int points_from_wire(Curve curve, const uint8_t* host_wire, uint64_t n, void* d_dense, bool check_subgroup, hipStream_t s, unsigned long long* first) {
    *first = ~0ull;
    if (!n) return ZK_OK;
    const size_t cb = aff_bytes(curve) / 2;
    DevBuf din, flag;
    ZKCHK(din.alloc(cb * n));
    ZKCHK(flag.alloc(16));                                  // the subgroup kernel's flag word | the first failure
    HIPCHK(hipMemsetAsync(flag.p, 0, 8, s));
    HIPCHK(hipMemsetAsync(flag.as<uint8_t>() + 8, 0xFF, 8, s));
    unsigned long long* d_first = (unsigned long long*)(flag.as<uint8_t>() + 8);
    HIPCHK(hipMemcpyAsync(din.p, host_wire, cb * n, hipMemcpyHostToDevice, s));
    {
        ScopedTimer t("key_decompress", s);
        for_curve(curve, [&](auto f) { hipLaunchKernelGGL(k_decompress<FIELD_OF(f)>, grid_for(n, 128), dim3(128), 0, s, (uint8_t*)d_dense, (const uint8_t*)din.as<uint8_t>(), n, d_first); });
    }
    if (check_subgroup) {
        ScopedTimer t("subgroup_check", s);
        launch_subgroup_check(curve, d_dense, n, flag.as<int>(), d_first, s, SUBGROUP_ENDO);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(first, d_first, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}
int wire_verdict(unsigned long long first) {
    if (first == ~0ull) return ZK_OK;
    const int kind = (int)(first & 7);
    if (kind == 2) ZK_FAIL(ZK_ERR_ARG, "wire point: the compression flag is not set, a coordinate is >= p, or the infinity bit is set on a string that is not C0 00 .. 00");
    if (kind == 1) ZK_FAIL(ZK_ERR_NOT_ON_CURVE, "wire point: an abscissa is not on the curve");
    ZK_FAIL(ZK_ERR_NOT_ON_CURVE, "wire point: on the curve but outside the prime-order subgroup (of_compressed_bytes_exn, curve.ml:199-212)");
}
int points_wire_check(Curve curve, const uint8_t* host_wire, uint64_t n, bool check_subgroup, hipStream_t s) {
    if (!n) return ZK_OK;
    DevBuf dense;
    unsigned long long first;
    ZKCHK(dense.alloc(aff_bytes(curve) * n));
    ZKCHK(points_from_wire(curve, host_wire, n, dense.p, check_subgroup, s, &first));
    return wire_verdict(first);
}
int msm_bases_from_wire(MsmBases& b, Curve curve, const uint8_t* host_wire, uint64_t n, uint32_t c, bool precomp, hipStream_t s, bool check_subgroup) {
    ZKCHK(bases_setup(b, curve, n, c, precomp, check_subgroup));      // folded digits only for points the subgroup test below has passed
    DevBuf dense;
    unsigned long long first;
    ZKCHK(dense.alloc(aff_bytes(curve) * n));
    ZKCHK(points_from_wire(curve, host_wire, n, dense.p, check_subgroup, s, &first));
    ZKCHK(wire_verdict(first));
    ZKCHK((curve == CURVE_G1 ? bases_finish<Fp>(b, dense.p, s) : bases_finish<Fp2>(b, dense.p, s)));
    HIPCHK(hipStreamSynchronize(s));          // `dense` is released on return: the table build has read it
    return ZK_OK;
}
// n dense affine points (device) -> their wire bytes (host)
int points_affine_to_wire(Curve curve, const void* d_aff, uint64_t n, uint8_t* host_out, hipStream_t s) {
    if (!n) return ZK_OK;
    const size_t cb = aff_bytes(curve) / 2;
    DevBuf dw;
    ZKCHK(dw.alloc(cb * n));
    {
        ScopedTimer t("key_compress", s);
        for_curve(curve, [&](auto f) { hipLaunchKernelGGL(k_compress<FIELD_OF(f)>, grid_for(n, 128), dim3(128), 0, s, dw.as<uint8_t>(), (const uint8_t*)d_aff, n); });
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host_out, dw.p, cb * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}
// the rows of XYZZ sums of `count` proofs (device) -> one group's points in the proofs' wire records (device): msm.cuh, ProofWire
int proofs_to_wire_dev(Curve curve, const void* d_rows, uint64_t count, const ProofWire& w, void* d_wire, hipStream_t s) {
    if (!count || !w.per) return ZK_OK;
    if (w.per > 6) ZK_FAIL(ZK_ERR_ARG, "proofs_to_wire_dev: at most 6 points of a group per proof");
    const uint64_t n = count * w.per;
    ScopedTimer t("prove_to_wire", s);
    for_curve(curve, [&](auto f) { hipLaunchKernelGGL(k_proofs_to_wire<FIELD_OF(f)>, grid_for(n, 128), dim3(128), 0, s, (uint8_t*)d_wire, (const uint8_t*)d_rows, n, w); });
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// zk_selftest_proof_wire: n pairs (affine point, z) (host) -> n XYZZ points on the device -> k_proofs_to_wire as a batch of n one-point proofs -> wire bytes (host)
int points_selftest_proof_wire(Curve curve, const uint8_t* affine, const uint8_t* z, uint64_t n, uint8_t* out, hipStream_t s) {
    const size_t ub = aff_bytes(curve), cb = ub / 2, xb = xyzz_bytes(curve);
    DevBuf din, dz, rows, dw, flag;
    ZKCHK(din.alloc(ub * n));
    ZKCHK(dz.alloc(32 * n));
    ZKCHK(rows.alloc(xb * n));
    ZKCHK(dw.alloc(cb * n));
    ZKCHK(flag.alloc(4));
    HIPCHK(hipMemsetAsync(flag.p, 0, 4, s));
    HIPCHK(hipMemcpyAsync(din.p, affine, ub * n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dz.p, z, 32 * n, hipMemcpyHostToDevice, s));
    for_curve(curve, [&](auto f) {
        hipLaunchKernelGGL(k_selftest_lift<FIELD_OF(f)>, grid_for(n, 128), dim3(128), 0, s, rows.as<uint8_t>(), (const uint8_t*)din.as<uint8_t>(), (const uint32_t*)dz.as<uint32_t>(), n, flag.as<int>());
    });
    HIPCHK(hipGetLastError());
    const ProofWire w{1, (uint32_t)xb, 0, (uint32_t)cb, {0, 0, 0, 0, 0, 0}};
    ZKCHK(proofs_to_wire_dev(curve, rows.p, n, w, dw.p, s));
    int h = 0;
    HIPCHK(hipMemcpyAsync(&h, flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out, dw.p, cb * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_proof_wire: a coordinate is >= p, or a z is 0 or >= r");
    return ZK_OK;
}

int xyzz_sum_columns(Curve curve, void* d_out, const void* d_parts, uint32_t count, uint32_t npoints, hipStream_t s) {
    if (curve == CURVE_G1) hipLaunchKernelGGL(k_xyzz_sum_columns<Fp>, grid_for(npoints, 64), dim3(64), 0, s, (uint8_t*)d_out, (const uint8_t*)d_parts, count, npoints);
    else hipLaunchKernelGGL(k_xyzz_sum_columns<Fp2H>, grid_for(2 * (uint64_t)npoints, 64), dim3(64), 0, s, (uint8_t*)d_out, (const uint8_t*)d_parts, count, npoints);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

// the generator tables 2^k * G live in the context of the device they were built on (zk_common.h: CtxBufs) and die with it

int fixed_base_mul(Curve curve, void* d_out, const void* d_scalars, uint64_t n, hipStream_t s) {
    if (!ctx().bufs) ZK_FAIL(ZK_ERR_HIP, "fixed_base_mul: no device context (zk_init)");
    DevBuf& tab = ctx().bufs->pow2[curve];
    if (!tab.p) {
        ZKCHK(tab.alloc(aff_bytes(curve) * 256));
        for_curve(curve, [&](auto f) { hipLaunchKernelGGL(k_gen_pow2_table<FIELD_OF(f)>, dim3(4), dim3(64), 0, s, tab.as<uint8_t>()); });
        HIPCHK(hipGetLastError());
    }
    if (!n) return ZK_OK;
    ScopedTimer t("fixed_base_mul", s);
    const uint8_t* pow2 = tab.as<uint8_t>();
    for_curve(curve, [&](auto f) { hipLaunchKernelGGL(k_fixed_base_mul<FIELD_OF(f)>, grid_for(n, 128), dim3(128), 0, s, (uint8_t*)d_out, (const uint32_t*)d_scalars, n, pow2); });
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// n compressed points (host) -> n uncompressed points (host), every one decoded, checked (curve, subgroup) and re-encoded on the device
int points_decompress(Curve curve, const uint8_t* in, uint64_t n, uint8_t* out, hipStream_t s) {
    if (!n) return ZK_OK;
    const size_t cb = aff_bytes(curve) / 2, ub = aff_bytes(curve);
    DevBuf din, dense, dout, flag;
    ZKCHK(din.alloc(cb * n));
    ZKCHK(dense.alloc(ub * n));
    ZKCHK(dout.alloc(ub * n));
    ZKCHK(flag.alloc(16));                                  // the subgroup kernel's flag word | the first failure: index << 3 | kind, all ones = none
    HIPCHK(hipMemsetAsync(flag.p, 0, 8, s));
    HIPCHK(hipMemsetAsync(flag.as<uint8_t>() + 8, 0xFF, 8, s));
    unsigned long long* first = (unsigned long long*)(flag.as<uint8_t>() + 8);
    HIPCHK(hipMemcpyAsync(din.p, in, cb * n, hipMemcpyHostToDevice, s));
    for_curve(curve, [&](auto f) { hipLaunchKernelGGL(k_decompress<FIELD_OF(f)>, grid_for(n, 128), dim3(128), 0, s, dense.as<uint8_t>(), (const uint8_t*)din.as<uint8_t>(), n, first); });
    launch_subgroup_check(curve, dense.p, n, flag.as<int>(), first, s);
    HIPCHK(hipGetLastError());
    ZKCHK(points_affine_to_bytes(curve, dout.p, dense.p, n, s));
    unsigned long long h = 0;
    HIPCHK(hipMemcpyAsync(&h, first, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out, dout.p, ub * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h != ~0ull) {          // the verdict of the first bad element of the list
        const int kind = (int)(h & 7);
        if (kind == 2) ZK_FAIL(ZK_ERR_ARG, "decompress: a point's compression flag is not set, a coordinate is >= p, or the infinity bit is set on a string that is not the identity's");
        if (kind == 1) ZK_FAIL(ZK_ERR_NOT_ON_CURVE, "decompress: an abscissa is not on the curve");
        ZK_FAIL(ZK_ERR_NOT_ON_CURVE, "decompress: a point is on the curve but outside the prime-order subgroup");
    }
    return ZK_OK;
}

// zk_selftest_point_decompress: n compressed points (host) through the slab front's two launches -- k_decompress_verdict, then k_subgroup_verdict by
// endomorphism -- -> one verdict each and the decoded point in the ABI's bytes (verdict 0 or 4; zero bytes for a point the decoder rejected)
int points_selftest_decompress(Curve curve, const uint8_t* in, uint64_t n, uint8_t* out, uint8_t* verdict, hipStream_t s) {
    const size_t cb = aff_bytes(curve) / 2, ub = aff_bytes(curve);
    const uint32_t off0 = 0;
    DevBuf din, dense, dout, dv;
    ZKCHK(din.alloc(cb * n));
    ZKCHK(dense.alloc(ub * n));
    ZKCHK(dout.alloc(ub * n));
    ZKCHK(dv.alloc(n));
    HIPCHK(hipMemcpyAsync(din.p, in, cb * n, hipMemcpyHostToDevice, s));
    ZKCHK(points_decompress_verdicts(curve, dense.p, din.p, n, 1, (uint32_t)cb, &off0, dv.as<uint8_t>(), s));
    ZKCHK(points_subgroup_verdicts(curve, dense.p, n, dv.as<uint8_t>(), SUBGROUP_ENDO, s));
    ZKCHK(points_affine_to_bytes(curve, dout.p, dense.p, n, s));
    HIPCHK(hipMemcpyAsync(out, dout.p, ub * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(verdict, dv.p, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < n; i++)
        if (verdict[i] == 1 || verdict[i] == 2) memset(out + ub * i, 0, ub);
    return ZK_OK;
}

int points_selftest_sqrt(int field, const uint8_t* a, uint64_t n, uint8_t* root, uint8_t* is_square, hipStream_t s) {
    const size_t B = field ? 96 : 48;
    DevBuf din, droot, dsq, flag;
    ZKCHK(din.alloc(B * n));
    ZKCHK(droot.alloc(B * n));
    ZKCHK(dsq.alloc(n));
    ZKCHK(flag.alloc(4));
    HIPCHK(hipMemsetAsync(flag.p, 0, 4, s));
    HIPCHK(hipMemcpyAsync(din.p, a, B * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_selftest_sqrt, grid_for(n, 128), dim3(128), 0, s, droot.as<uint8_t>(), dsq.as<uint8_t>(), (const uint8_t*)din.as<uint8_t>(), n, field, flag.as<int>());
    HIPCHK(hipGetLastError());
    int h = 0;
    HIPCHK(hipMemcpyAsync(&h, flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(root, droot.p, B * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(is_square, dsq.p, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_sqrt: an element is >= p");
    return ZK_OK;
}

// ---- may one product read another's sort?  (msm.cuh: msm_accumulate_sorted)
__global__ void k_bytes_differ(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t n, int* flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && a[i] != b[i]) *flag = 1;
}
int msm_bases_same_geometry(const MsmBases& a, const MsmBases& b, bool* same, hipStream_t s) {
    *same = false;
    if (a.n != b.n || a.c != b.c || a.nw != b.nw || a.precomp != b.precomp || a.fold != b.fold) return ZK_OK;
    DevBuf flag;
    ZKCHK(flag.alloc(4));
    HIPCHK(hipMemsetAsync(flag.p, 0, 4, s));
    hipLaunchKernelGGL(k_bytes_differ, grid_for(a.n, 256), dim3(256), 0, s, (const uint8_t*)a.ident.as<uint8_t>(), (const uint8_t*)b.ident.as<uint8_t>(), a.n, flag.as<int>());
    HIPCHK(hipGetLastError());
    int h = 1;
    HIPCHK(hipMemcpyAsync(&h, flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *same = h == 0;
    return ZK_OK;
}

}  // namespace zk
