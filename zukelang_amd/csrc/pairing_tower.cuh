// Fp12 on the device for the batched pairings of pairing_dev.hip (scope row f1: Pairing.pairing, curve.mli:46-54, under Groth16's and
// Pinocchio's verifiers, groth16.ml:163-173 / pinocchio.ml:254-420).
//
// Fp12 = Fp2[w] / (w^6 - xi), xi = 1 + u: the coefficient of v^j w^i of the host tower (pairing_host.hip: Fp6 = Fp2[v] / (v^3 - xi), Fp12 = Fp6[w] /
// (w^2 - v)) is the coefficient of w^(2 j + i) here.  ONE ELEMENT IS SPREAD OVER A GROUP OF 8 LANES: lane s < 6 of the group owns the Fp2 coefficient
// of w^s (lanes 6 and 7 repeat the work of lanes 0 and 1: a wave holds 8 groups, and a group never straddles a wave).  A whole element is 168
// registers before any temporary, so one lane per element would live in scratch memory; spread, a lane carries 28.
//
// The elements of a group live in ITS OWN SLICE OF LDS, as a small register file: NREG elements of 6 x 28 words (14 + 14 limbs of 29 bits, the lazily
// reduced register format of ff.cuh, not the dense memory format) and, for the Miller loop, a handful of single Fp2 cells (the running point, the
// line).  Every operation is an out-of-line function over register NUMBERS: lane k reads the coefficients it needs, computes coefficient k and writes
// it back -- a product is six Fp2 products per lane (c_k = sum_{i+j=k} a_i b_j + xi sum_{i+j=k+6} a_i b_j), a product with a sparse line three, a
// Frobenius map one.  About twice the base-field products of the Karatsuba tower, for lanes that all do the same thing.  Operands cross lanes
// through LDS instead of ds_bpermute: the same exchange, but a function's arguments are a few integers (a by-value Fp2 crosses a call through
// scratch memory, ff.cuh) and nothing but the two accumulators of a product is live in registers, so no kernel here spills.
//
// Rules: workgroups are ONE wave (64 lanes: __syncthreads is the cheap s_barrier that orders the slice's reads and writes), every lane of a workgroup
// calls every function (control flow is uniform: no predicate depends on a value), a destination may alias a source (all reads happen before the
// barrier that precedes the writes).  Bounds: coefficients rest below 256 p (F12C), line coefficients below 1024 p; the types check every formula.
#pragma once
#define ZK_FP_INLINE_MUL          // products expanded in place: the functions below take register numbers, nothing is live across their calls
#include "ec.cuh"
#include "pairing_dev_consts.cuh"

namespace zk {
namespace f12 {

static constexpr uint32_t GROUP = 8, GROUPS_PER_WAVE = 64 / GROUP;
static constexpr uint32_t CW = 2 * FPL;                 // words of one Fp2 cell
static constexpr uint32_t EW = 6 * CW;                  // words of one Fp12 register
static constexpr uint32_t NREG = 6;
// slice of one group: NREG registers, then one cell; the Miller loop's cells (NCELL of them) overlay registers 1.. (it uses register 0 only)
static constexpr uint32_t NCELL = 21;
static constexpr uint32_t CELL_TAIL = NREG * EW;
static constexpr uint32_t SLICE = NREG * EW + CW;
static_assert(EW + NCELL * CW <= SLICE, "the Miller cells overlay registers 1..");
static_assert(SLICE * GROUPS_PER_WAVE * 4 <= 65536, "one workgroup's LDS");

using F12C = Fp2B<256>;          // a coefficient at rest
using LineC = Fp2B<1024>;        // a line coefficient at rest

__shared__ __attribute__((aligned(16))) uint32_t g_lds[SLICE * GROUPS_PER_WAVE];

FF_INLINE uint32_t slot() { return threadIdx.x & (GROUP - 1); }
FF_INLINE uint32_t coef() { const uint32_t s = slot(); return s < 6 ? s : s - 6; }                  // the coefficient this lane computes
FF_INLINE uint32_t* slice() { return g_lds + SLICE * ((threadIdx.x & 63u) / GROUP); }
FF_INLINE uint32_t* reg_cell(uint32_t r, uint32_t k) { return slice() + r * EW + k * CW; }
FF_INLINE uint32_t* cell(uint32_t c) { return slice() + EW + c * CW; }                              // Miller cells
FF_INLINE uint32_t* tail_cell() { return slice() + CELL_TAIL; }

// UNCHECKED bound: the caller names the bound of what was stored there
template <int B> FF_INLINE Fp2B<B> ld(const uint32_t* p) {
    Fp2B<B> r;
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint32_t t[CW];
#pragma unroll
    for (int i = 0; i < (int)CW / 4; i++) { const uint4 x = q[i]; t[4 * i] = x.x; t[4 * i + 1] = x.y; t[4 * i + 2] = x.z; t[4 * i + 3] = x.w; }
#pragma unroll
    for (int i = 0; i < FPL; i++) { r.c0.v[i] = t[i]; r.c1.v[i] = t[FPL + i]; }
    return r;
}
template <int A> FF_INLINE void st(uint32_t* p, const Fp2B<A>& a) {
    uint32_t t[CW];
#pragma unroll
    for (int i = 0; i < FPL; i++) { t[i] = a.c0.v[i]; t[FPL + i] = a.c1.v[i]; }
    uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
    for (int i = 0; i < (int)CW / 4; i++) q[i] = make_uint4(t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]);
}
template <int B> FF_INLINE Fp2B<B> sel(bool take_b, const Fp2B<B>& a, const Fp2B<B>& b) { return {fp_select(take_b, a.c0, b.c0), fp_select(take_b, a.c1, b.c1)}; }
// v_k of six values, widened to the bound B
template <int B, class T0, class T1, class T2, class T3, class T4, class T5>
FF_INLINE Fp2B<B> pick(uint32_t k, const T0& v0, const T1& v1, const T2& v2, const T3& v3, const T4& v4, const T5& v5) {
    Fp2B<B> r = v0;
    r = sel<B>(k == 1, r, v1);
    r = sel<B>(k == 2, r, v2);
    r = sel<B>(k == 3, r, v3);
    r = sel<B>(k == 4, r, v4);
    r = sel<B>(k == 5, r, v5);
    return r;
}
// (a0 + a1 u)(1 + u)
template <int A> FF_INLINE Fp2B<A + fp_ks(A)> mul_xi(const Fp2B<A>& a) { return {fe_sub(a.c0, a.c1), FpB<A + fp_ks(A)>(fe_add(a.c0, a.c1))}; }
template <int A> FF_INLINE Fp2B<2> red2(const Fp2B<A>& a) { return {fe_mul(a.c0, fp_one()), fe_mul(a.c1, fp_one())}; }          // the same value below 2 p

// ------------------------------------------------------------------ the field operations (register numbers in, register number out)
__device__ __noinline__ void set_one(uint32_t dst) {
    const uint32_t k = coef();
    __syncthreads();
    st(reg_cell(dst, k), sel<1>(k == 0, fp2_zero(), fp2_one()));
    __syncthreads();
}
__device__ __noinline__ void copy(uint32_t dst, uint32_t a) {
    const uint32_t k = coef();
    const F12C x = ld<256>(reg_cell(a, k));
    __syncthreads();
    st(reg_cell(dst, k), x);
    __syncthreads();
}
// dst = a b
__device__ __noinline__ void mul(uint32_t dst, uint32_t a, uint32_t b) {
    const uint32_t k = coef();
    Fp2B<60> lo = fp2_zero(), hi = fp2_zero();          // i + j = k | i + j = k + 6
#pragma unroll 1
    for (uint32_t i = 0; i < 6; i++) {
        const bool wrap = i > k;
        const F12C x = ld<256>(reg_cell(a, i)), y = ld<256>(reg_cell(b, wrap ? k + 6 - i : k - i));
        const Fp2B<10> m = fe_mul(x, y), z = fp2_zero();
        // six terms below 10 p each: the loop-carried sums stay below 60 p
        lo = fp_assume<60>(fe_add(fp_assume<50>(lo), sel<10>(wrap, m, z)));
        hi = fp_assume<60>(fe_add(fp_assume<50>(hi), sel<10>(wrap, z, m)));
    }
    const F12C r = fe_add(lo, mul_xi(hi));
    __syncthreads();
    st(reg_cell(dst, k), r);
    __syncthreads();
}
// dst = a (l0 + l3 w^3 + l5 w^5), the line in the Miller cells c0, c0 + 1, c0 + 2
__device__ __noinline__ void mul_line(uint32_t dst, uint32_t a, uint32_t c0) {
    const uint32_t k = coef();
    Fp2B<30> lo = fp2_zero(), hi = fp2_zero();
#pragma unroll 1
    for (uint32_t t = 0; t < 3; t++) {
        const uint32_t j = t == 0 ? 0u : t == 1 ? 3u : 5u;
        const bool wrap = j > k;
        const F12C x = ld<256>(reg_cell(a, wrap ? k + 6 - j : k - j));
        const LineC l = ld<1024>(cell(c0 + t));
        const Fp2B<10> m = fe_mul(x, l), z = fp2_zero();
        lo = fp_assume<30>(fe_add(fp_assume<20>(lo), sel<10>(wrap, m, z)));
        hi = fp_assume<30>(fe_add(fp_assume<20>(hi), sel<10>(wrap, z, m)));
    }
    const F12C r = fe_add(lo, mul_xi(hi));
    __syncthreads();
    st(reg_cell(dst, k), r);
    __syncthreads();
}
// dst = a^(p^6): w -> -w
__device__ __noinline__ void conj(uint32_t dst, uint32_t a) {
    const uint32_t k = coef();
    const F12C x = ld<256>(reg_cell(a, k));
    const F12C r = red2(sel<512>(k & 1, x, fe_neg(x)));
    __syncthreads();
    st(reg_cell(dst, k), r);
    __syncthreads();
}
// dst = a^p: (c w^k)^p = conj(c) g^k w^k
__device__ __noinline__ void frob(uint32_t dst, uint32_t a) {
    const uint32_t k = coef();
    const F12C x = ld<256>(reg_cell(a, k));
    Fp2B<1> g;
#pragma unroll
    for (int i = 0; i < FPL; i++) { g.c0.v[i] = PAIRING_FROB[k][0][i]; g.c1.v[i] = PAIRING_FROB[k][1][i]; }
    const F12C r = fe_mul(Fp2B<512>(x.c0, fe_neg(x.c1)), g);
    __syncthreads();
    st(reg_cell(dst, k), r);
    __syncthreads();
}
// dst = 1 / a (0 for 0).  n = a conj(a) lies in Fp6 = Fp2[w^2]; its norm to Fp2 is n n^(p^2) n^(p^4), so with m = n^(p^2) n^(p^4)
// 1 / a = conj(a) m / (n m) for ONE inversion in Fp2 (every lane inverts the same value).  t1, t2, t3: scratch registers, all distinct from dst and a.
__device__ __noinline__ void inv(uint32_t dst, uint32_t a, uint32_t t1, uint32_t t2, uint32_t t3) {
    conj(t1, a);
    mul(t2, a, t1);          // n
    frob(t3, t2);
    frob(t3, t3);            // n^(p^2)
    frob(dst, t3);
    frob(dst, dst);          // n^(p^4)
    mul(t3, t3, dst);        // m
    mul(dst, t2, t3);        // n m: coefficient 0 holds the norm, the others are 0 mod p
    mul(t1, t1, t3);         // conj(a) m
    const uint32_t k = coef();
    const Fp2B<4> s = fe_inv(ld<256>(reg_cell(dst, 0)));
    const F12C r = fe_mul(ld<256>(reg_cell(t1, k)), s);
    __syncthreads();
    st(reg_cell(dst, k), r);
    __syncthreads();
}
// dst = a^e, e = e_hi 2^64 + e_lo of `bits` bits (a constant of the curve: the branch is uniform); dst != a
__device__ __noinline__ void pow(uint32_t dst, uint32_t a, uint64_t e_lo, uint64_t e_hi, int bits) {
    set_one(dst);
#pragma unroll 1
    for (int i = bits - 1; i >= 0; i--) {
        mul(dst, dst, dst);
        if (((i < 64 ? e_lo >> i : e_hi >> (i - 64)) & 1) != 0) mul(dst, dst, a);
    }
}
static constexpr uint64_t BLS_X = PAIRING_BLS_X, E1_LO = PAIRING_E1_LO, E1_HI = PAIRING_E1_HI;          // scripts/gen_pairing_consts.py
static constexpr int E1_BITS = PAIRING_E1_BITS;
// register 0 <- register 0 ^ ((p^12 - 1) / r), factored as final_exp of pairing_host.hip; uses every register
__device__ __noinline__ void final_exp() {
    conj(1, 0);
    inv(2, 0, 3, 4, 5);
    mul(1, 1, 2);                          // f^(p^6 - 1)
    frob(2, 1);
    frob(2, 2);
    mul(1, 2, 1);                          // m = ^(p^2 + 1)
    pow(2, 1, E1_LO, E1_HI, E1_BITS);      // a = m^e1
    pow(3, 2, BLS_X, 0, 64);
    conj(3, 3);
    frob(4, 2);
    mul(3, 3, 4);                          // b = a^(x + p)
    pow(2, 3, BLS_X, 0, 64);
    pow(4, 2, BLS_X, 0, 64);               // b^(x^2)
    frob(2, 3);
    frob(2, 2);
    mul(4, 4, 2);
    conj(2, 3);
    mul(4, 4, 2);                          // c = b^(x^2 + p^2 - 1)
    mul(0, 4, 1);                          // c m
}

// ------------------------------------------------------------------ registers <-> memory
// raw coefficients (the Miller values between the two kernels): 6 x 28 words per element
FF_INLINE void load_raw(uint32_t dst, const uint32_t* p) {
    const uint32_t k = coef();
    const F12C x = ld<256>(p + k * CW);
    __syncthreads();
    st(reg_cell(dst, k), x);
    __syncthreads();
}
FF_INLINE void store_raw(uint32_t* p, uint32_t a, bool write) {
    const uint32_t k = coef();
    if (write) st(p + k * CW, ld<256>(reg_cell(a, k)));
}
// the GT encoding of pairing_host.hip: 12 x 48 B big-endian, c0.c0.a, c0.c0.b, c0.c1.a, ... c1.c2.b; the coefficient of w^k is block 3 (k & 1) + (k >> 1)
FF_INLINE void fp_be_store(uint8_t* p, const FpWords& a) {
    uint32_t* w = reinterpret_cast<uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < 12; i++) w[11 - i] = __builtin_bswap32(a.w[i]);
}
FF_INLINE FpWords fp_be_load(const uint8_t* p) {
    FpWords r;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < 12; i++) r.w[i] = __builtin_bswap32(w[11 - i]);
    return r;
}
FF_INLINE uint32_t gt_block(uint32_t k) { return 3 * (k & 1) + (k >> 1); }
FF_INLINE void store_gt(uint8_t* out, uint32_t a, bool write) {
    const uint32_t k = coef();
    const F12C x = ld<256>(reg_cell(a, k));
    const FpWords re = fp_from_mont(x.c0), im = fp_from_mont(x.c1);
    if (write) {
        fp_be_store(out + 96 * gt_block(k), re);
        fp_be_store(out + 96 * gt_block(k) + 48, im);
    }
}
// false: a coefficient is >= p
FF_INLINE bool load_gt(uint32_t dst, const uint8_t* in) {
    const uint32_t k = coef();
    const FpWords re = fp_be_load(in + 96 * gt_block(k)), im = fp_be_load(in + 96 * gt_block(k) + 48);
    const bool ok = words_are_canonical<FpParams>(re.w) && words_are_canonical<FpParams>(im.w);
    const Fp2B<2> x = {fp_to_mont(re), fp_to_mont(im)};
    __syncthreads();
    st(reg_cell(dst, k), x);
    __syncthreads();
    return ok;
}

// ------------------------------------------------------------------ the Miller loop of one pair (P in G1, Q on the twist), one group per pair
// T = (X : Y : Z) on the twist y^2 = x^3 + 4 xi in homogeneous coordinates (x = X / Z, y = Y / Z): no inversion.  The host's line at T with slope
// lam is yP + ((lam x_T - y_T) / xi) w^3 - (lam xP / xi) w^5 (pairing_host.hip: miller_product); here every line is that element times xi and
// times the slope's denominator, factors in Fp2 that the power p^6 - 1 of the final exponentiation sends to 1:
//   tangent (x 2 Y Z):     xi yP 2 Y Z + (Y^2 - 3 b' Z^2) w^3 - 3 X^2 xP w^5                (3 X^3 / Z = 3 Y^2 - 3 b' Z^2 on the curve, b' = 4 xi)
//   chord to Q (x v):      xi yP v + (u xQ - v yQ) w^3 - u xP w^5,   u = yQ Z - Y, v = xQ Z - X
// and the point steps are the inversion-free ones of Costello, Lange, Naehrig (PKC 2010) scaled by 4 / the mixed addition add-1998-cmo-2.  The
// products of a step are independent in two (tangent) / four (chord) levels, and the six lanes of the group take one each.
enum : uint32_t { C_X = 0, C_Y, C_Z, C_QX, C_QY, C_PX, C_PY, C_L0, C_L3, C_L5, C_R0, C_S = C_R0 + 6, C_E, C_H, C_BPF, C_BMF, C_U = C_S, C_V, C_A, C_RMA };
static_assert(C_BMF < NCELL, "Miller cells");
using TC = Fp2B<256>;            // a coordinate of T at rest
// Each level: every lane prepares the level's operands (sums and differences: cheap, the same on all lanes) in cells, then lane k multiplies the two
// cells the level assigns to it -- the operands are chosen by ADDRESS, so a lane holds two of them, not all.
FF_INLINE uint32_t tab6(uint32_t k, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t c4, uint32_t c5) {
    return k == 0 ? c0 : k == 1 ? c1 : k == 2 ? c2 : k == 3 ? c3 : k == 4 ? c4 : c5;
}
// cell(out_k) <- cell(l_k) cell(r_k), operands below W p
template <int W> FF_INLINE void level(uint32_t l, uint32_t r, uint32_t out) {
    const Fp2B<10> m = fe_mul(ld<W>(cell(l)), ld<W>(cell(r)));
    __syncthreads();
    st(cell(out), m);
    __syncthreads();
}

__device__ __noinline__ void dbl_step() {
    const uint32_t k = coef();
    {
        const auto S = fe_add(ld<256>(cell(C_Y)), ld<256>(cell(C_Z)));
        static_assert(decltype(S)::BOUND <= 512, "operand bounds");
        st(cell(C_S), S);
        __syncthreads();
    }
    // X Y | Y^2 | Z^2 | (Y + Z)^2 | X^2 | (X^2)
    level<512>(tab6(k, C_X, C_Y, C_Z, C_S, C_X, C_X), tab6(k, C_Y, C_Y, C_Z, C_S, C_X, C_X), C_R0 + k);
    constexpr int W = 10 + fp_ks(936);
    {
        const Fp2B<10> B = ld<10>(cell(C_R0 + 1)), C = ld<10>(cell(C_R0 + 2));
        const auto H = fe_sub(fe_sub(ld<10>(cell(C_R0 + 3)), B), C);                   // 2 Y Z
        st(cell(C_H), H);
        const auto xc = mul_xi(C);
        const auto E = fe_add(fe_dbl(fe_dbl(xc)), fe_dbl(fe_dbl(fe_dbl(xc))));          // 3 b' Z^2 = 12 xi Z^2
        st(cell(C_E), E);
        const auto l3 = fe_sub(B, E);
        static_assert(decltype(l3)::BOUND <= 1024, "line at rest");
        st(cell(C_L3), l3);
        const auto F = fe_add(E, fe_dbl(E));
        static_assert(decltype(F)::BOUND == 936, "operand bounds");
        const auto BpF = fe_add(B, F);
        const auto BmF = fe_sub(B, F);
        static_assert(decltype(BmF)::BOUND == W && decltype(BpF)::BOUND <= W && decltype(E)::BOUND <= W && decltype(H)::BOUND <= W, "operand bounds");
        st(cell(C_BPF), BpF);
        st(cell(C_BMF), BmF);
        __syncthreads();
    }
    // X Y (B - F) | (B + F)^2 | E^2 | B H | X^2 xP | H yP
    level<W>(tab6(k, C_R0, C_BPF, C_E, C_R0 + 1, C_R0 + 4, C_H), tab6(k, C_BMF, C_BPF, C_E, C_H, C_PX, C_PY), C_R0 + k);
    LineC o;
    {
        const auto X3 = fe_dbl(ld<10>(cell(C_R0)));                                  // 4 A (B - F), A = X Y / 2
        const auto Z3 = fe_dbl(fe_dbl(ld<10>(cell(C_R0 + 3))));                      // 4 B H
        static_assert(decltype(X3)::BOUND <= 256 && decltype(Z3)::BOUND <= 256, "T at rest");
        o = sel<1024>(k == 2, X3, Z3);
    }
    {
        const Fp2B<10> r2 = ld<10>(cell(C_R0 + 2));
        const auto Y3 = fe_sub(ld<10>(cell(C_R0 + 1)), fe_add(fe_dbl(fe_dbl(r2)), fe_dbl(fe_dbl(fe_dbl(r2)))));          // 4 G^2 - 12 E^2, G = (B + F) / 2
        static_assert(decltype(Y3)::BOUND <= 256, "T at rest");
        o = sel<1024>(k == 1, o, Y3);
    }
    {
        const Fp2B<10> r4 = ld<10>(cell(C_R0 + 4));
        o = sel<1024>(k == 3, o, mul_xi(ld<10>(cell(C_R0 + 5))));                    // xi yP 2 Y Z
        o = sel<1024>(k == 5, o, fe_neg(fe_add(fe_dbl(r4), r4)));                    // - 3 X^2 xP
    }
    __syncthreads();
    if (k != 4) st(cell(tab6(k, C_X, C_Y, C_Z, C_L0, C_L3, C_L5)), o);               // the w^3 coefficient went out above
    __syncthreads();
}
// T <- T + Q and the chord's line
__device__ __noinline__ void add_step() {
    const uint32_t k = coef();
    level<256>(k & 1 ? C_QX : C_QY, C_Z, C_R0 + (k & 1));          // yQ Z | xQ Z
    constexpr int W = 10 + fp_ks(256);
    {
        const auto u = fe_sub(ld<10>(cell(C_R0)), ld<256>(cell(C_Y))), v = fe_sub(ld<10>(cell(C_R0 + 1)), ld<256>(cell(C_X)));
        static_assert(decltype(u)::BOUND == W, "operand bounds");
        st(cell(C_U), u);
        st(cell(C_V), v);
        __syncthreads();
    }
    // u^2 | v^2 | u xQ | v yQ | u xP | v yP
    level<W>(k & 1 ? C_V : C_U, tab6(k, C_U, C_V, C_QX, C_QY, C_PX, C_PY), C_R0 + k);
    {
        const Fp2B<10> ux = ld<10>(cell(C_R0 + 2)), vy = ld<10>(cell(C_R0 + 3)), up = ld<10>(cell(C_R0 + 4)), vp = ld<10>(cell(C_R0 + 5));
        st(cell(C_L0), mul_xi(vp));
        st(cell(C_L3), fe_sub(ux, vy));
        st(cell(C_L5), fe_neg(up));
        __syncthreads();
    }
    const uint32_t t = k < 3 ? k : k - 3;
    // u^2 Z | v^3 | v^2 X   (v^2, then u^2: the outputs overwrite them in that order only after every lane has read)
    level<W>(tab6(t, C_R0, C_V, C_R0 + 1, 0, 0, 0), tab6(t, C_Z, C_R0 + 1, C_X, 0, 0, 0), C_R0 + 2 + t);
    {
        const Fp2B<10> uuZ = ld<10>(cell(C_R0 + 2)), vvv = ld<10>(cell(C_R0 + 3)), R = ld<10>(cell(C_R0 + 4));
        const auto A = fe_sub_sub_dbl(uuZ, vvv, R);
        const auto RmA = fe_sub(R, A);
        static_assert(decltype(RmA)::BOUND <= W && decltype(A)::BOUND <= W, "operand bounds");
        st(cell(C_A), A);
        st(cell(C_RMA), RmA);
        __syncthreads();
    }
    // v A | u (R - A) | v^3 Y | v^3 Z
    const uint32_t q = k & 3;
    level<W>(tab6(q, C_V, C_U, C_R0 + 3, C_R0 + 3, 0, 0), tab6(q, C_A, C_RMA, C_Y, C_Z, 0, 0), C_S + q);          // over u, v, A, R - A: every lane has read them
    {
        const Fp2B<10> X3 = ld<10>(cell(C_S)), Z3 = ld<10>(cell(C_S + 3));
        const auto Y3 = fe_sub(ld<10>(cell(C_S + 1)), ld<10>(cell(C_S + 2)));
        const TC o = pick<256>(t, X3, Y3, Z3, X3, X3, X3);
        __syncthreads();
        st(cell(C_X + t), o);
        __syncthreads();
    }
}
// register 0 <- f_{|x|, Q}(P) conjugated (x < 0), the loop of miller_product for one pair.  P, Q: genuine points, the same for every lane of the group
FF_INLINE void miller(const Aff<Fp>& P, const Aff<Fp2>& Q) {
    {
        const Fp2B<2> px = {fp_assume<2>(P.x), fp_zero()}, py = {fp_assume<2>(P.y), fp_zero()};
        const Fp2B<2> qx = fp_assume<2>(Q.x), qy = fp_assume<2>(Q.y);
        __syncthreads();
        st(cell(C_PX), px);
        st(cell(C_PY), py);
        st(cell(C_QX), qx);
        st(cell(C_QY), qy);
        st(cell(C_X), qx);
        st(cell(C_Y), qy);
        st(cell(C_Z), fp2_one());
        __syncthreads();
    }
    set_one(0);
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {          // below the top bit of |x|
        mul(0, 0, 0);
        dbl_step();
        mul_line(0, 0, C_L0);
        if ((BLS_X >> i) & 1) {
            add_step();
            mul_line(0, 0, C_L0);
        }
    }
    conj(0, 0);
}

}  // namespace f12
}  // namespace zk
