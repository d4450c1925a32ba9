// One scalar times a long list of resident G1 points, affine in and affine out: the tail of zk_groth16_pk_contribute (include/zkmi355x.h).
//
// A phase-2 contribution multiplies delta by delta'.  Of a proving key (src/groth16/groth16.ml:45-108) only d1, d2 and the contiguous tail of the G1 pool
// -- tiztd | ltd_mid, or hl | ltd_mid in Lagrange form -- depend on delta, the tail through 1 / delta: n - 1 + |mids| points times ONE scalar, 1 / delta'.
//
// The multiplication runs on the kernels of the Lagrange derivation (lagrange_derive.hip: points_scale_tabmul = k_aff_to_raw, k_g_tabmul over a table of
// scalars, k_raw_to_aff); this unit adds the table of equal scalars and the slabs.  A kernel of its own was built and measured against that route -- the
// scalar split and recoded once on the host and passed by value, every digit branch wave-uniform, ONE inversion per workgroup on the way back to affine
// (prefix and suffix products of the Z across the workgroup in LDS), one pass over memory instead of three -- and it did not win: 63.0 ms against 62.2 ms
// for the 2 097 151 points of a 2^20 key's tail, best of five (profiles/contribute_kernel_ab.json; DESIGN 2q has the reasons).  The rule was fixed before
// the numbers: the kernel stays only if it beats this route by more than the route's spread.  It does not stay.
#include "groth16_key.cuh"

#include <string.h>

namespace zk {

static constexpr uint32_t SCALE_SLAB = (uint32_t)1 << 18;           // points per chain of launches: 64 MiB of raw points beside the 1 GiB of window tables (DERIVE_SLAB)

// tab[i] = k for i < count: the constant table k_g_tabmul reads its per-point scalars from
__global__ void k_scalar_table(uint32_t* __restrict__ tab, const uint32_t* __restrict__ k, uint64_t count) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
#pragma unroll
    for (int j = 0; j < 8; j++) tab[8 * i + j] = k[j];
}

// pts[i] <- k pts[i] in place for n dense affine G1 points (device); k: canonical, little-endian words; slab: points per chain, 0 = the default
int g1_scale_points(void* d_pts, uint64_t n, const uint64_t k[4], uint32_t slab, hipStream_t s) {
    if (!n) return ZK_OK;
    const uint64_t per = slab ? slab : SCALE_SLAB, most = n < per ? n : per;
    DevBuf dk, table;
    ZKCHK(dk.alloc(32));
    ZKCHK(table.alloc(32 * most));
    HIPCHK(hipMemcpyAsync(dk.p, k, 32, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_scalar_table, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, s, table.as<uint32_t>(), (const uint32_t*)dk.as<uint32_t>(), most);
    HIPCHK(hipGetLastError());
    for (uint64_t i0 = 0; i0 < n; i0 += per) {
        const uint64_t cnt = n - i0 < per ? n - i0 : per;
        uint8_t* p = (uint8_t*)d_pts + 96 * i0;
        ZKCHK(points_scale_tabmul(CURVE_G1, p, p, table.p, cnt, s));          // waits for the stream: `k` and the working arrays of a slab are done with
    }
    // the scalar is a contributor's secret (or its inverse): it does not stay behind in freed device memory
    HIPCHK(hipMemsetAsync(table.p, 0, 32 * most, s));
    HIPCHK(hipMemsetAsync(dk.p, 0, 32, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}

}  // namespace zk

using namespace zk;
// The contribution's tail on a caller's list (include/zkmi355x.h).  Everything that can be refused is refused before the device is touched.
extern "C" int zk_selftest_g1_scale(const uint8_t* pts, size_t n, const uint8_t k[32], uint32_t slab, uint8_t* out) {
    if (!pts || !k || !out || n == 0) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_g1_scale: null argument or an empty list");
    uint64_t kw[4];
    cs_load(kw, k);
    if (!cs_canonical(kw)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_g1_scale: k >= r");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    DevBuf bytes, dense, flag;
    ZKCHK(bytes.alloc(96 * n));
    ZKCHK(dense.alloc(96 * n));
    ZKCHK(flag.alloc(4));
    HIPCHK(hipMemsetAsync(flag.p, 0, 4, s));
    HIPCHK(hipMemcpyAsync(bytes.p, pts, 96 * n, hipMemcpyHostToDevice, s));
    ZKCHK(points_bytes_to_affine(CURVE_G1, dense.p, bytes.p, n, flag.as<int>(), s));
    int h = 0;
    HIPCHK(hipMemcpyAsync(&h, flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h & 2) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_g1_scale: point encoding: compressed flag set or coordinate >= p");
    if (h & 1) ZK_FAIL(ZK_ERR_NOT_ON_CURVE, "zk_selftest_g1_scale: a point is not on the curve");
    ZKCHK(g1_scale_points(dense.p, n, kw, slab, s));
    ZKCHK(points_affine_to_bytes(CURVE_G1, bytes.p, dense.p, n, s));
    HIPCHK(hipMemcpyAsync(out, bytes.p, 96 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}
