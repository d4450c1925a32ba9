// G2 bucket accumulation on lane pairs with the field products EXPANDED IN PLACE (as msm_acc_g1.hip does for G1): no call inside the mixed
// addition, so the record of the next step can travel HBM -> LDS by LDS-DMA while this step computes -- every function entry drains the
// loads in flight (s_waitcnt 0 is part of the calling convention), which left the out-of-line form (msm_acc_g2.hip) waiting for a full
// random-gather round trip at the top of every step.  One copy of the group law (no 6-product second step): ~68 KB of code.
#define ZK_FP_INLINE_MUL 1
#include "msm_acc.cuh"
#include "group_selftest.cuh"

namespace zk {
int msm_accumulate_launch_g2_inline(uint64_t nthreads, const void* table, const AccJobs& jobs, uint32_t count, uint32_t nb, uint32_t chunk, hipStream_t s) {
    hipLaunchKernelGGL((k_msm_accumulate<Fp2H, false, true, false>), dim3((unsigned)((2 * nthreads + 127) / 128), count), dim3(128), 0, s, (const uint8_t*)table, jobs, nb, chunk);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
// zk_selftest_group, forms 7-10 in G2: the mixed additions on lane pairs with the products expanded in place, and xyzz_madd_parked with ZZ / ZZZ in the
// LDS park buffer of k_msm_accumulate (same layout, same lane index), written and read back around the addition as the bucket loop does.
__global__ __launch_bounds__(128) void k_group_selftest_acc_g2i(int form, int rep, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t n, uint8_t* __restrict__ out) {
    __shared__ uint4 park_buf[2][4][128];
    if (form != GROUP_FORM_MADD_PARKED) {
        st_acc_forms<Fp2H>(form, rep, a, b, n, out);
        return;
    }
    const uint64_t i = st_index<Fp2H>();
    if (i >= n) return;
    const bool lift = rep != 0;
    Xyzz<Fp2H> acc = st_load_xyzz<Fp2H>(a, i, lift);
    ZPark<Fp2H> zpark{&park_buf[0][0][0], threadIdx.x};
    zpark.put(0, acc.zz);
    zpark.put(1, acc.zzz);
    xyzz_madd_parked<Fp2H>(acc.x, acc.y, zpark, st_load_aff<Fp2H, 1, 2>(b, i, lift));
    acc.zz = zpark.get(0);
    acc.zzz = zpark.get(1);
    st_store_xyzz<Fp2H>(out, i, acc);
}
int group_selftest_acc_g2i(const GroupSelftest& t, hipStream_t s) {
    if (t.curve != CURVE_G2 || t.form < GROUP_FORM_MADD_INLINE || t.form > GROUP_FORM_MADD_PARKED) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_group: this unit builds forms 7-10 in G2");
    hipLaunchKernelGGL(k_group_selftest_acc_g2i, grid_for(2 * t.n, 128), dim3(128), 0, s, t.form, t.rep, t.d_a, t.d_b, t.n, t.d_out);
    HIPCHK(hipGetLastError());
    return ZK_OK;
}
}  // namespace zk
