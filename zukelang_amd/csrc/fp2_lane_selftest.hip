// zk_selftest_fp2_lanewise (include/zkmi355x.h, tests/test_gpu_fp2_lanewise.py): fe_mul2_lanewise and the fused a b - c d of ff.cuh on bare limbs, built
// the way the G2 bucket accumulation builds them -- products expanded in place, one lane pair per quadruple, lane 2k holding the c0 components and
// lane 2k+1 the c1 components.  Operands arrive as register limbs, so the caller chooses the representation: any value up to the at-rest bound 64 p
// in any weakly normalised form.  Results leave fully reduced.
#define ZK_FP_INLINE_MUL 1
#include "ec.cuh"
#include "msm.cuh"

namespace zk {

static constexpr int FP2_LANE_OUTS = 3, FP2_LANE_IN_WORDS = 4 * 2 * 16;          // a | b | c | d, each c0 | c1, each 14 limbs in a 16-word slot
static constexpr uint32_t FP2_LANE_WEAK_LIMB = (1u << FP29_W) + 7;

__global__ __launch_bounds__(128) void k_fp2_lane_selftest(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = t >> 1, comp = pair_comp();
    if (i >= n) return;                                   // pair-uniform
    Fp2HB<FP_REST + 1> v[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int l = 0; l < FPL; l++) v[j].v.v[l] = in[(uint64_t)FP2_LANE_IN_WORDS * i + 32 * j + 16 * comp + l];
    uint32_t* o = out + ((uint64_t)FP2_LANE_OUTS * 2 * i + comp) * 12;
    auto put = [&](int k, const FpB<8>& x) {
        const FpWords w = fp_pack(fp_canon(x));
#pragma unroll
        for (int l = 0; l < 12; l++) o[24 * k + l] = w.w[l];
    };
    const Fp2HPair m = fe_mul2_lanewise(v[0], v[1], v[2], v[3]);          // 0, 1: a b | c d
    put(0, m.first.v);
    put(1, m.second.v);
    put(2, fe_mul2_sub_lanewise(v[0], v[1], v[2], v[3]).v);                // 2: a b - c d
}

}  // namespace zk

using namespace zk;

extern "C" int zk_selftest_fp2_lanewise(const uint32_t* operands, size_t n, uint8_t* out) {
    if (!operands || !out || !n || n >= ((size_t)1 << 24)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp2_lanewise: null argument or no operands");
    for (size_t i = 0; i < 8 * n; i++) {
        const uint32_t* l = operands + 16 * i;
        for (int k = 0; k < FPL; k++)
            if (l[k] > FP2_LANE_WEAK_LIMB) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp2_lanewise: a limb above 2^29 + 7");
        if (l[FPL - 1] > 64u * 13u) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fp2_lanewise: a top limb above 64 * 13");          // below 65 p, as in zk_selftest_fp_paired
    }
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    DevBuf din, dout;
    ZKCHK(din.alloc((size_t)FP2_LANE_IN_WORDS * 4 * n));
    ZKCHK(dout.alloc((size_t)FP2_LANE_OUTS * 96 * n));
    HIPCHK(hipMemcpyAsync(din.p, operands, (size_t)FP2_LANE_IN_WORDS * 4 * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_fp2_lane_selftest, grid_for(2 * n, 128), dim3(128), 0, s, dout.as<uint32_t>(), (const uint32_t*)din.as<uint32_t>(), (uint32_t)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)FP2_LANE_OUTS * 96 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}
