// zk_selftest_group (include/zkmi355x.h, tests/test_gpu_group_law.py): what the self-test kernels of the group law share.  Every translation unit that
// owns a form of "add two points" defines ONE kernel over these helpers, after its own #define ZK_FP_INLINE_MUL (or without it): the zero test
// fe_is_zero and the field products compile differently under that flag, so a form is only tested where it is built as production builds it.
//
// Device input (group_selftest.hip prepared it on the host): every field element as 12 dense little-endian words of the PLAIN integer (< p, checked
// on the host); a G2 element as c0 | c1.  a[i] = x | y | zz | zzz, an affine b[i] = x | y, a scalar b[i] = 8 words.  Output: dense Montgomery XYZZ
// (ec.cuh: xyzz_store), which points_xyzz_to_bytes encodes.
//
// rep = 1 hands every operand to the form as x + k p with the largest k the operand's TYPE admits (st_lift: built from fe_sub / fe_add, the bounds are
// the types' own), so that the zero tests on ZZ, P and R see multiples of p instead of zeros:
//   at-rest operands (Fp / Fp2H = bound FP_REST: accumulators, XYZZ and raw-layout second operands, the affine q of the raw-point accumulate)  k = FP_REST - 1
//   table entries (madd without the identity test, the parked form): x is FpB<1> and stays canonical, y is FpB<1> or its negation 2p - y: k = 1 on y
//   the affine window table of the scalar multiplication (jac_madd: x is fp_assume<2>, y a cond_neg of bound 4): k = 1 on x, k = 3 on y
//   the scalar multiplication's own table is built inside it: only the multiplicand is lifted.
#pragma once
#include "ec.cuh"
#include "msm.cuh"

namespace zk {

template <class F, int B> struct StBound;
template <int A, int B> struct StBound<FpB<A>, B> { using type = FpB<B>; };
template <int A, int B> struct StBound<Fp2HB<A>, B> { using type = Fp2HB<B>; };

// x + (B - A) p for a value typed FpB<A>: fe_sub(x, 0 typed FpB<K - 1>) adds fp_ks(K - 1) p = K p for a power of two K; the last odd p is FP29_MOD itself
template <int B, int A> FF_INLINE FpB<B> st_lift(const FpB<A>& x) {
    constexpr int room = B - A;
    if constexpr (room >= 2) {
        constexpr int K = fp_ks(room) > room ? fp_ks(room) / 2 : fp_ks(room);          // the largest power of two <= room
        static_assert(K >= 2 && K <= room && fp_ks(K - 1) == K, "lift step");
        return st_lift<B>(fe_sub(x, FpB<K - 1>(fp_zero())));
    } else if constexpr (room == 1) {
        FpB<1> p;
#pragma unroll
        for (int i = 0; i < FPL; i++) p.v[i] = FP29_MOD[i];
        return fe_add(x, p);
    } else {
        return x;
    }
}
template <int B> FF_INLINE FpB<B> st_fp(const uint8_t* p, bool lift) {
    const FpB<1> x = fp_canon(fp_to_mont(fpw_load(p)));
    if (lift) return st_lift<B>(x);
    return FpB<B>(x);
}
static constexpr int ST_REST = FP_REST;
template <int B> FF_INLINE FpB<B> st_coord(const Fp*, const uint8_t* p, bool lift) { return st_fp<B>(p, lift); }
template <int B> FF_INLINE Fp2HB<B> st_coord(const Fp2H*, const uint8_t* p, bool lift) { return {st_fp<B>(p + 48 * pair_comp(), lift)}; }

template <class F> struct StGeom {
    static constexpr int CB = FieldOps<F>::WORDS * 4;          // bytes of one coordinate, in and out
    static constexpr int LANES = RawLayout<F>::LANES;
};
template <class F> FF_INLINE uint64_t st_index() { return ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / StGeom<F>::LANES; }
template <class F> FF_INLINE Xyzz<F> st_load_xyzz(const uint8_t* a, uint64_t i, bool lift) {
    constexpr int CB = StGeom<F>::CB;
    const uint8_t* p = a + (uint64_t)4 * CB * i;
    return {st_coord<ST_REST>((const F*)nullptr, p, lift), st_coord<ST_REST>((const F*)nullptr, p + CB, lift), st_coord<ST_REST>((const F*)nullptr, p + 2 * CB, lift),
            st_coord<ST_REST>((const F*)nullptr, p + 3 * CB, lift)};
}
// BX, BY: the bounds the form's production caller hands the affine coordinates over with
template <class F, int BX, int BY> FF_INLINE Aff<F> st_load_aff(const uint8_t* b, uint64_t i, bool lift) {
    constexpr int CB = StGeom<F>::CB;
    const uint8_t* p = b + (uint64_t)2 * CB * i;
    return {F(st_coord<BX>((const F*)nullptr, p, lift)), F(st_coord<BY>((const F*)nullptr, p + CB, lift))};
}
template <class F> FF_INLINE void st_store_xyzz(uint8_t* out, uint64_t i, const Xyzz<F>& r) { xyzz_store<F>(out + (uint64_t)4 * StGeom<F>::CB * i, r); }

// ---- the mixed additions of the bucket accumulation (msm_acc.cuh), instantiated by msm_acc_g1.hip, msm_acc_g2.hip and msm_acc_g2i.hip
template <class F> FF_INLINE void st_acc_forms(int form, int rep, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t n, uint8_t* __restrict__ out) {
    const uint64_t i = st_index<F>();
    if (i >= n) return;
    const bool lift = rep != 0;
    Xyzz<F> acc = st_load_xyzz<F>(a, i, lift);
    if (form == GROUP_FORM_MADD || form == GROUP_FORM_MADD_INLINE) xyzz_madd_impl<F, true>(acc, st_load_aff<F, ST_REST, ST_REST>(b, i, lift));
    else if (form == GROUP_FORM_MMADD || form == GROUP_FORM_MMADD_INLINE) xyzz_mmadd_impl<F, true>(acc, st_load_aff<F, ST_REST, ST_REST>(b, i, lift));
    else xyzz_madd_impl<F, false>(acc, st_load_aff<F, 1, 2>(b, i, lift));
    st_store_xyzz<F>(out, i, acc);
}

}  // namespace zk
