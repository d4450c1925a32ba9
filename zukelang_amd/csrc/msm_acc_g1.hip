// G1 bucket accumulation with the field products expanded in place: no call boundary inside the mixed
// addition, so the gather of the next table entry stays in flight across it (the compiler must drain
// outstanding loads at every call).  ~40 KB of straight-line code per mixed addition: it fits the
// 64 KB instruction cache shared by a CU pair.
#define ZK_FP_INLINE_MUL 1
#include "msm_acc.cuh"
#include "group_selftest.cuh"

#include <stdlib.h>

namespace zk {
int msm_accumulate_launch_g1(uint64_t nthreads, const void* table, const AccJobs& jobs, uint32_t count, uint32_t nb, uint32_t chunk, hipStream_t s) {
    // ZK_ACC_G1_GLDS=0: the register look-ahead (A/B of the LDS-DMA look-ahead).  Cached; per launch only under ZK_TEST_FORMS=1 (zk_options.h).
    const bool glds = opt_on(OPT_ACC_G1_GLDS, true);
    const bool mm = opt_on(OPT_ACC_G1_MMADD, false);      // A/B: the 6-product second step (more code)
    if (glds && !mm) hipLaunchKernelGGL((k_msm_accumulate<Fp, false, true, false>), dim3((unsigned)((nthreads + 127) / 128), count), dim3(128), 0, s, (const uint8_t*)table, jobs, nb, chunk);
    else if (glds) hipLaunchKernelGGL((k_msm_accumulate<Fp, false, true>), dim3((unsigned)((nthreads + 127) / 128), count), dim3(128), 0, s, (const uint8_t*)table, jobs, nb, chunk);
    else hipLaunchKernelGGL((k_msm_accumulate<Fp, false, false>), dim3((unsigned)((nthreads + 127) / 128), count), dim3(128), 0, s, (const uint8_t*)table, jobs, nb, chunk);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// zk_selftest_group, forms 7-9 in G1: the three mixed additions as this unit builds them (products and the zero test's slow path expanded in place),
// one lane per pair of operands.  The equal-x case leaves through xyzz_madd_equal_x, out of line, as in the bucket loop.
__global__ __launch_bounds__(128) void k_group_selftest_acc_g1(int form, int rep, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t n, uint8_t* __restrict__ out) {
    st_acc_forms<Fp>(form, rep, a, b, n, out);
}
int group_selftest_acc_g1(const GroupSelftest& t, hipStream_t s) {
    if (t.curve != CURVE_G1 || t.form < GROUP_FORM_MADD_INLINE || t.form > GROUP_FORM_MMADD_INLINE) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_group: this unit builds forms 7-9 in G1");
    hipLaunchKernelGGL(k_group_selftest_acc_g1, grid_for(t.n, 128), dim3(128), 0, s, t.form, t.rep, t.d_a, t.d_b, t.n, t.d_out);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
}  // namespace zk
