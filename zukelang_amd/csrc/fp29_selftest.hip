// zk_selftest_fp29 (include/zkmi355x.h; tests/test_gpu_fp29.py): the layer under every Fp product -- the additive forms of ff.cuh with their three tables
// of spread multiples of p, the full reduction fp_canon_call, the zero test, the dense memory format and the lockstep inversion of fp_inv.cuh -- on bare
// limbs.  Operands arrive as 14 register limbs, so the caller chooses the representation: the integer 2^380 reaches fp_inv29_call as 2^380 and not as a
// Montgomery residue, a value of 8191 p reaches the quotient estimate, a non-multiple with a small limb0 / p reaches the slow path of the zero test.  Results
// leave as raw limbs, with no reduction beyond what the function under test does, so that the header's limb claims are visible.  The kernels here and in
// fp29_selftest_inline.hip (the same zero test built the way the units that expand their products in place build it) are the hook's own: no kernel of the
// proving or verifying path is touched.
#include "ff.cuh"
#include "fp29_selftest.cuh"
#include "zk_common.h"

namespace zk {

__global__ __launch_bounds__(64) void k_fp29_selftest(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint32_t n, int op) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* src = in + (uint64_t)FP29_ST_IN_WORDS * i;
    uint32_t* o = out + (uint64_t)fp29_st_out_words(op) * i;
    FpRaw a, b, c;
#pragma unroll
    for (int l = 0; l < FPL; l++) { a.v[l] = src[l]; b.v[l] = src[16 + l]; c.v[l] = src[32 + l]; }
    auto put = [&](uint32_t* dst, const uint32_t* x) {
#pragma unroll
        for (int l = 0; l < FPL; l++) dst[l] = x[l];
    };
    if (op == FP29_OP_CANON) {
        const FpRaw r = fp_canon_call(FP_PASS(a.v));
        put(o, r.v);
    } else if (op == FP29_OP_CARRY) {
        fp_carry(a.v);
        put(o, a.v);
    } else if (op == FP29_OP_ADD) {
        const auto r = fe_add(fp_from_raw<FP_REST>(a), fp_from_raw<FP_REST>(b));
        put(o, r.v);
    } else if (op == FP29_OP_DBL) {
        const auto r = fe_dbl(fp_from_raw<FP_REST>(a));
        put(o, r.v);
    } else if (op == FP29_OP_PACK) {
        FpWords w;
#pragma unroll
        for (int l = 0; l < 12; l++) w.w[l] = src[l];
        const FpB<1> u = fp_unpack(w);
        const FpWords p = fp_pack(u);
        put(o, u.v);
#pragma unroll
        for (int l = 0; l < 12; l++) o[FPL + l] = p.w[l];
    } else if (op == FP29_OP_INV) {
        const FpRaw r = fp_inv29_call(FP_PASS(a.v));
        put(o, r.v);
        const FpB<1> f = fp_canon(fe_inv_fast(fp_from_raw<1>(a)));
        put(o + FPL, f.v);
    } else if (op >= FP29_OP_ZERO && op < FP29_OP_ZERO + 3) {
        // bit 0: fe_is_zero<B> with the fp_canon slow path (this unit does not define ZK_FP_INLINE_MUL); bit 2: fp_is_zero_mod_p_inline called directly;
        // bit 1 is added by k_fp29_zero_inline
        bool z = false;
        if (op == FP29_OP_ZERO) z = fe_is_zero(fp_from_raw<FP29_ZERO_B0>(a));
        else if (op == FP29_OP_ZERO + 1) z = fe_is_zero(fp_from_raw<FP29_ZERO_B1>(a));
        else z = fe_is_zero(fp_from_raw<FP29_ZERO_B2>(a));
        o[0] = (z ? 1u : 0u) | (fp_is_zero_mod_p_inline(a.v) ? 4u : 0u);
    }
}

// one instantiation per reachable table row: the operand bound of row k is 1 (k = 0) or 2^k, so that fp_ki(fp_ks(bound)) = k
template <int ROW> struct RowBound { static constexpr int B = ROW == 0 ? 1 : 1 << ROW; };
template <int ROW> FF_INLINE void fp29_row_op(int fn, uint32_t* __restrict__ o, const FpRaw& a, const FpRaw& b, const FpRaw& c) {
    constexpr int B = RowBound<ROW>::B;
    static_assert(fp_ki(fp_ks(B)) == ROW, "row bound");
    if (fn == 1) {
        const auto r = fe_neg(fp_from_raw<B>(a));
#pragma unroll
        for (int l = 0; l < FPL; l++) o[l] = r.v[l];
    } else if (fn == 2) {
        const auto r = fe_neg_lazy(fp_from_raw<B>(a));
#pragma unroll
        for (int l = 0; l < FPL; l++) o[l] = r.v[l];
    }
    if constexpr (ROW <= 11) {
        if (fn == 0) {
            const auto r = fe_sub(fp_from_raw<FP_REST>(a), fp_from_raw<B>(b));
#pragma unroll
            for (int l = 0; l < FPL; l++) o[l] = r.v[l];
        }
    }
    if constexpr (ROW >= 1 && ROW <= 11) {
        if (fn == 3) {          // b, c < 2^(ROW - 1) p (or p at ROW = 1): fp_ks(3 B') = 2^(ROW + 1)
            constexpr int BS = RowBound<ROW - 1>::B;
            static_assert(fp_ki(fp_ks(3 * BS)) == ROW, "row bound");
            const auto r = fe_sub_sub_dbl(fp_from_raw<FP_REST>(a), fp_from_raw<BS>(b), fp_from_raw<BS>(c));
#pragma unroll
            for (int l = 0; l < FPL; l++) o[l] = r.v[l];
        }
    }
}
__global__ __launch_bounds__(64) void k_fp29_rows(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint32_t n, int fn, int row) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* src = in + (uint64_t)FP29_ST_IN_WORDS * i;
    uint32_t* o = out + (uint64_t)FPL * i;
    FpRaw a, b, c;
#pragma unroll
    for (int l = 0; l < FPL; l++) { a.v[l] = src[l]; b.v[l] = src[16 + l]; c.v[l] = src[32 + l]; }
    switch (row) {
#define ROW_CASE(R) case R: fp29_row_op<R>(fn, o, a, b, c); break;
        ROW_CASE(0) ROW_CASE(1) ROW_CASE(2) ROW_CASE(3) ROW_CASE(4) ROW_CASE(5) ROW_CASE(6) ROW_CASE(7) ROW_CASE(8) ROW_CASE(9) ROW_CASE(10) ROW_CASE(11) ROW_CASE(12)
#undef ROW_CASE
    default: break;
    }
}

namespace {

constexpr uint32_t FP29_WEAK_LIMB = (1u << FP29_W) + 7;
constexpr uint32_t FP29_MOD_HOST[FPL] = {0x1fffaaabu, 0x0ff7ffffu, 0x14ffffeeu, 0x17fffd62u, 0x0f6241eau, 0x09507b58u, 0x0afd9cc3u,
                                         0x109e70a2u, 0x1764774bu, 0x121a5d66u, 0x12c6e9edu, 0x12ffcd34u, 0x00111ea3u, 0x0000000du};
constexpr uint32_t FP_MOD_WORDS_HOST[12] = {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                                            0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
// the top limb of every exact-limb value below bound * p is at most (bound * p) >> 377: p >> 317 is 0xd0088f51cbff34d2, and the 317 bits dropped add
// less than `bound` to the product, which changes the quotient by 2^60 only if its low 60 bits are within `bound` of 2^60 -- they are not for any bound
// the ops use (tests/test_fp29_selftest_surface.py holds every one of them to the integer)
uint32_t top_limb_of(uint32_t bound) { return (uint32_t)(((unsigned __int128)0xd0088f51cbff34d2ull * bound) >> 60); }
bool weak_limbs_ok(const uint32_t* l, uint32_t bound) {
    for (int k = 0; k < FPL - 1; k++)
        if (l[k] > FP29_WEAK_LIMB) return false;
    return l[FPL - 1] <= top_limb_of(bound);
}
bool canonical_limbs(const uint32_t* l) {                            // exact limbs and a value below p
    for (int k = 0; k < FPL - 1; k++)
        if (l[k] > FP29_MASK) return false;
    for (int k = FPL - 1; k >= 0; k--)
        if (l[k] != FP29_MOD_HOST[k]) return l[k] < FP29_MOD_HOST[k];
    return false;
}
bool canonical_words(const uint32_t* w) {
    for (int k = 11; k >= 0; k--)
        if (w[k] != FP_MOD_WORDS_HOST[k]) return w[k] < FP_MOD_WORDS_HOST[k];
    return false;
}
inline dim3 grid64(size_t n) { return dim3((unsigned)((n + 63) / 64)); }
constexpr int row_bound(int row) { return row == 0 ? 1 : 1 << row; }

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" int zk_selftest_fp29(int op, const uint32_t* operands, size_t n, uint32_t* out) {
    const int fn = op >= FP29_OP_ROWS ? (op - FP29_OP_ROWS) / 16 : -1, row = op >= FP29_OP_ROWS ? (op - FP29_OP_ROWS) % 16 : -1;
    const bool plain = op >= 0 && (op <= FP29_OP_INV || (op >= FP29_OP_ZERO && op < FP29_OP_ZERO + 3));
    const bool rows = fn >= 0 && fn <= 3 && ((fn == 0 && row <= 11) || ((fn == 1 || fn == 2) && row <= 12) || (fn == 3 && row >= 1 && row <= 11));
    if (!plain && !rows) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp29: an unknown op");
    if (!operands || !out || !n || n >= ((size_t)1 << 24)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp29: null argument or no operands");
    for (size_t i = 0; i < n; i++) {
        const uint32_t* l = operands + (size_t)FP29_ST_IN_WORDS * i;
        bool ok = true;
        if (op == FP29_OP_CANON) ok = weak_limbs_ok(l, FP_MAX_BOUND);
        else if (op == FP29_OP_CARRY) ok = true;                     // fp_carry's own precondition is limbs below 2^32
        else if (op == FP29_OP_ADD) ok = weak_limbs_ok(l, FP_REST) && weak_limbs_ok(l + 16, FP_REST);
        else if (op == FP29_OP_DBL) ok = weak_limbs_ok(l, FP_REST);
        else if (op == FP29_OP_PACK) ok = canonical_words(l);
        else if (op == FP29_OP_INV) ok = canonical_limbs(l);
        else if (plain) ok = weak_limbs_ok(l, op == FP29_OP_ZERO ? FP29_ZERO_B0 : op == FP29_OP_ZERO + 1 ? FP29_ZERO_B1 : FP29_ZERO_B2);
        else if (fn == 0) ok = weak_limbs_ok(l, FP_REST) && weak_limbs_ok(l + 16, row_bound(row));
        else if (fn == 1 || fn == 2) ok = weak_limbs_ok(l, row_bound(row));
        else ok = weak_limbs_ok(l, FP_REST) && weak_limbs_ok(l + 16, row_bound(row - 1)) && weak_limbs_ok(l + 32, row_bound(row - 1));
        if (!ok) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp29: a limb above 2^29 + 7, a top limb above that of the op's value bound, or an operand that is not canonical");
    }
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    const size_t in_bytes = (size_t)FP29_ST_IN_WORDS * 4 * n, out_bytes = (size_t)fp29_st_out_words(op) * 4 * n;
    DevBuf din, dout;
    ZKCHK(din.alloc(in_bytes));
    ZKCHK(dout.alloc(out_bytes));
    HIPCHK(hipMemcpyAsync(din.p, operands, in_bytes, hipMemcpyHostToDevice, s));
    if (rows) hipLaunchKernelGGL(k_fp29_rows, grid64(n), dim3(64), 0, s, dout.as<uint32_t>(), (const uint32_t*)din.as<uint32_t>(), (uint32_t)n, fn, row);
    else hipLaunchKernelGGL(k_fp29_selftest, grid64(n), dim3(64), 0, s, dout.as<uint32_t>(), (const uint32_t*)din.as<uint32_t>(), (uint32_t)n, op);
    HIPCHK(hipGetLastError());
    if (plain && op >= FP29_OP_ZERO) ZKCHK(fp29_selftest_zero_inline(dout.as<uint32_t>(), (const uint32_t*)din.as<uint32_t>(), (uint32_t)n, op - FP29_OP_ZERO, s));
    HIPCHK(hipMemcpyAsync(out, dout.p, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}
