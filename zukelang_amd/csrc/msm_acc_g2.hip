// G2 bucket accumulation on lane pairs (Fp2H: one Fp2 component per lane), field products out of line.
#include "msm_acc.cuh"
#include "group_selftest.cuh"

#include <stdlib.h>

namespace zk {
int msm_accumulate_launch_g1(uint64_t nthreads, const void* table, const AccJobs& jobs, uint32_t count, uint32_t nb, uint32_t chunk, hipStream_t s);
int msm_accumulate_launch_g2_inline(uint64_t nthreads, const void* table, const AccJobs& jobs, uint32_t count, uint32_t nb, uint32_t chunk, hipStream_t s);
int msm_accumulate_launch(Curve curve, uint64_t nthreads, const void* table, const AccJobs& jobs, uint32_t count, uint32_t nb, uint32_t chunk, hipStream_t s, bool raw) {
    if (raw) {
        // the finisher of the batch-affine rounds: a few entries per bucket are left, the products stay out of line for both curves
        if (curve == CURVE_G1) hipLaunchKernelGGL((k_msm_accumulate<Fp, true>), dim3((unsigned)((nthreads + 127) / 128), count), dim3(128), 0, s, (const uint8_t*)table, jobs, nb, chunk);
        else hipLaunchKernelGGL((k_msm_accumulate<Fp2H, true>), dim3((unsigned)((2 * nthreads + 127) / 128), count), dim3(128), 0, s, (const uint8_t*)table, jobs, nb, chunk);
        HIPCHK(hipGetLastError());
        return ZK_OK;
    }
    if (curve == CURVE_G1) return msm_accumulate_launch_g1(nthreads, table, jobs, count, nb, chunk, s);
    const bool g2_inline = opt_on(OPT_ACC_G2_INLINE, true);      // A/B switch (cached; per launch only under ZK_TEST_FORMS=1)
    if (g2_inline) return msm_accumulate_launch_g2_inline(nthreads, table, jobs, count, nb, chunk, s);
    hipLaunchKernelGGL((k_msm_accumulate<Fp2H, false>), dim3((unsigned)((2 * nthreads + 127) / 128), count), dim3(128), 0, s, (const uint8_t*)table, jobs, nb, chunk);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// zk_selftest_group, forms 4-6: the mixed additions with the field products out of line, as the raw-point accumulate of both curves and the G2
// accumulate under ZK_ACC_G2_INLINE=0 run them.  One lane (G1) or lane pair (G2) per pair of operands.
template <class F> __global__ __launch_bounds__(128) void k_group_selftest_acc(int form, int rep, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t n, uint8_t* __restrict__ out) {
    st_acc_forms<F>(form, rep, a, b, n, out);
}
int group_selftest_acc_g2(const GroupSelftest& t, hipStream_t s) {
    if (t.form < GROUP_FORM_MADD || t.form > GROUP_FORM_MMADD) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_group: this unit builds forms 4-6");
    if (t.curve == CURVE_G1) hipLaunchKernelGGL(k_group_selftest_acc<Fp>, grid_for(t.n, 128), dim3(128), 0, s, t.form, t.rep, t.d_a, t.d_b, t.n, t.d_out);
    else hipLaunchKernelGGL(k_group_selftest_acc<Fp2H>, grid_for(2 * t.n, 128), dim3(128), 0, s, t.form, t.rep, t.d_a, t.d_b, t.n, t.d_out);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
}  // namespace zk
