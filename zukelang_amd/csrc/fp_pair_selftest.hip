// zk_selftest_fp_paired (include/zkmi355x.h, tests/test_gpu_fp_paired.py): the paired field products of fp_pair_gen.cuh on bare limbs, built the way the
// kernels that use them are -- products expanded in place.  Operands arrive as their 14 register limbs, so the caller chooses the representation: any
// value up to the at-rest bound 64 p (top limb at most 64 * 13: below 65 p) in any weakly normalised form, every limb at 2^29 + 7 included.  Results leave fully reduced.
#define ZK_FP_INLINE_MUL 1
#include "ec.cuh"
#include "msm.cuh"

#include <vector>

namespace zk {

static constexpr int FP_PAIR_OUTS = 13, FP_PAIR_IN_WORDS = 4 * 16;          // a | b | c | d, each 14 limbs in a 16-word slot
static constexpr uint32_t FP_WEAK_LIMB = (1u << FP29_W) + 7;

__global__ __launch_bounds__(64) void k_fp_pair_selftest(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    FpB<FP_REST + 1> a, b, c, d;
#pragma unroll
    for (int l = 0; l < FPL; l++) {
        a.v[l] = in[FP_PAIR_IN_WORDS * i + l];
        b.v[l] = in[FP_PAIR_IN_WORDS * i + 16 + l];
        c.v[l] = in[FP_PAIR_IN_WORDS * i + 32 + l];
        d.v[l] = in[FP_PAIR_IN_WORDS * i + 48 + l];
    }
    uint32_t* o = out + (uint64_t)FP_PAIR_OUTS * 12 * i;
    auto put = [&](int k, const FpB<2>& x) {
        const FpWords w = fp_pack(fp_canon(x));
#pragma unroll
        for (int l = 0; l < 12; l++) o[12 * k + l] = w.w[l];
    };
    const auto m = fe_mul2(a, b, c, d);                  // 0, 1: a b | c d
    put(0, m.first);
    put(1, m.second);
    const auto s = fe_sqr2(a, c);                        // 2, 3: a^2 | c^2
    put(2, s.first);
    put(3, s.second);
    const auto same = fe_mul2(a, b, a, b);               // 4, 5: the two products share both operands
    put(4, same.first);
    put(5, same.second);
    const auto cross = fe_mul2(a, b, c, a);              // 6, 7: a is the left factor of one and the right factor of the other
    put(6, cross.first);
    put(7, cross.second);
    {                                                    // 8, 9: each output written over an input of the OTHER product
        FpB<2> x, y;
#pragma unroll
        for (int l = 0; l < FPL; l++) { x.v[l] = a.v[l]; y.v[l] = d.v[l]; }
        fp_mul_pair_limbs(y.v, x.v, b.v, x.v, c.v, y.v);          // y = a b, x = c d
        put(8, y);
        put(9, x);
    }
    const auto t = fe_mul_sub_mul2(a, b, c, d, a, d, c, b);          // 10, 11, 12: a b - c d (c negated lazily: limbs up to 2^30) | a d | c b
    put(10, t.first);
    put(11, t.second);
    put(12, t.third);
}

}  // namespace zk

using namespace zk;

extern "C" int zk_selftest_fp_paired(const uint32_t* operands, size_t n, uint8_t* out) {
    if (!operands || !out || !n || n >= ((size_t)1 << 24)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp_paired: null argument or no operands");
    for (size_t i = 0; i < 4 * n; i++) {
        const uint32_t* l = operands + 16 * i;
        for (int k = 0; k < FPL; k++)
            if (l[k] > FP_WEAK_LIMB) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp_paired: a limb above 2^29 + 7");
        // 64 p - 1 has the top limb 64 * 13; the limbs below hold less than 2^377 (1 + 2^-28) and p > 13 * 2^377, so the value stays below 65 p
        if (l[FPL - 1] > 64u * 13u) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp_paired: a top limb above 64 * 13");
    }
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    DevBuf din, dout;
    ZKCHK(din.alloc((size_t)FP_PAIR_IN_WORDS * 4 * n));
    ZKCHK(dout.alloc((size_t)FP_PAIR_OUTS * 48 * n));
    HIPCHK(hipMemcpyAsync(din.p, operands, (size_t)FP_PAIR_IN_WORDS * 4 * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_fp_pair_selftest, grid_for(n, 64), dim3(64), 0, s, dout.as<uint32_t>(), (const uint32_t*)din.as<uint32_t>(), (uint32_t)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)FP_PAIR_OUTS * 48 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}
