// zk_selftest_fp29, ops 8-10, bit 1: fe_is_zero<B> of ff.cuh as the translation units that expand their products in place compile it -- with
// ZK_FP_INLINE_MUL defined its slow path is fp_is_zero_mod_p_inline instead of fp_canon (the G1 accumulate loop, the batch-affine rounds).  The form is
// chosen by the preprocessor, so it needs a unit of its own; fp29_selftest.hip holds everything else.
#define ZK_FP_INLINE_MUL 1
#include "ff.cuh"
#include "fp29_selftest.cuh"
#include "zk_common.h"

namespace zk {

__global__ __launch_bounds__(64) void k_fp29_zero_inline(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint32_t n, int which) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    FpRaw a;
#pragma unroll
    for (int l = 0; l < FPL; l++) a.v[l] = in[(uint64_t)FP29_ST_IN_WORDS * i + l];
    bool z;
    if (which == 0) z = fe_is_zero(fp_from_raw<FP29_ZERO_B0>(a));
    else if (which == 1) z = fe_is_zero(fp_from_raw<FP29_ZERO_B1>(a));
    else z = fe_is_zero(fp_from_raw<FP29_ZERO_B2>(a));
    out[i] |= z ? 2u : 0u;
}

int fp29_selftest_zero_inline(uint32_t* d_out, const uint32_t* d_in, uint32_t n, int which, hipStream_t s) {
    if (which < 0 || which > 2) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp29: this unit builds ops 8-10");
    hipLaunchKernelGGL(k_fp29_zero_inline, dim3((n + 63) / 64), dim3(64), 0, s, d_out, d_in, n, which);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}

}  // namespace zk
