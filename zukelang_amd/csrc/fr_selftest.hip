// zk_selftest_fr and zk_selftest_fr29 (include/zkmi355x.h; tests/test_gpu_fr_field.py): the two scalar-field layers on bare operands, through the
// functions of the shipped headers -- the 8 x 32-bit Fe<FrParams> of ff.cuh (k_spmv, k_check_r1cs, the tables, every to/from-Montgomery pass) and the
// lazily reduced 9 x 29-bit integers of fr29.cuh (the NTT butterflies).  The second hook takes raw limbs, so that the caller puts a butterfly at the
// bounds of the stage schedule (ntt_lds.cuh), which no input of zk_fr_ntt can do, and returns raw limbs, so that the header's limb claims are visible.
// The kernels here are the hooks' own: no kernel of the proving path is touched.
#include "fr29.cuh"
#include "zk_common.h"

namespace zk {

static constexpr int FR_OUTS = 14;                                   // op 0 of zk_selftest_fr: 14 x 8 words per pair
static constexpr int FR29_IN_WORDS = 3 * FR29_L;                     // u | v | w
static constexpr uint32_t FR29_WEAK_LIMB = (1u << FR29_W) + 7;
static constexpr uint32_t FR29_TOP_64R = 0x1cfb69d4u;                // (64 r) >> 232: the top limb of every exact-limb value below 64 r is at most this
static constexpr uint32_t FR_MOD_HOST[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
static constexpr uint32_t FR29_MOD_HOST[FR29_L] = {0x00000001u, 0x1ffffff8u, 0x1f96ffbfu, 0x1b4805ffu, 0x1d80553bu, 0x0c0404d0u, 0x1520cce7u, 0x0a6533afu, 0x0073eda7u};

FF_INLINE Fr fr_c32_mont() {                                         // 32 in Montgomery form: x R * 32 = x * 2^261, the factor convention of fr29.cuh
    Fr c;
#pragma unroll
    for (int l = 0; l < 8; l++) c.v[l] = FR29_C32[l];
    return c;
}

__global__ __launch_bounds__(64) void k_fr_selftest(uint32_t* __restrict__ out, const uint32_t* __restrict__ a_in, const uint32_t* __restrict__ b_in, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fr ap = fe_load<FrParams>(a_in + 8 * (uint64_t)i), bp = fe_load<FrParams>(b_in + 8 * (uint64_t)i);
    const Fr a = fe_to_mont(ap), b = fe_to_mont(bp);
    uint32_t* o = out + (uint64_t)FR_OUTS * 8 * i;
    auto put_plain = [&](int k, const Fr& x) { fe_store<FrParams>(o + 8 * k, x); };
    auto put = [&](int k, const Fr& x) { put_plain(k, fe_from_mont(x)); };
    put(0, fe_add(a, b));
    put(1, fe_sub(a, b));
    put(2, fe_sub(b, a));
    put(3, fe_mul(a, b));
    put(4, fe_sqr(a));
    put(5, fe_neg(a));
    put(6, fe_dbl(a));
    put(7, fe_inv(a));
    put_plain(8, fe_from_mont(fe_to_mont(ap)));
    put(9, fe_from_u32<FrParams>(ap.v[0]));
    {                                                                // 10: a row of three terms, accumulated the way k_spmv does
        Fr acc = fe_zero<FrParams>();
        acc = fe_add(acc, fe_mul(a, b));
        acc = fe_add(acc, fe_mul(a, a));
        acc = fe_add(acc, fe_mul(b, b));
        put(10, acc);
    }
    {
        Fr f = fe_zero<FrParams>();
        f.v[0] = (fe_is_zero(a) ? 1u : 0u) | (fe_eq(a, b) ? 2u : 0u);
        put_plain(11, f);
    }
    put(12, fr9_canon_pack(fr9_unpack(a)));
    put(13, fr9_canon_pack(fr9_mul(fr9_unpack(a), fr9_unpack(fe_mul(b, fr_c32_mont())))));
}

__global__ __launch_bounds__(64) void k_fr_canonical_selftest(uint8_t* __restrict__ out, const uint32_t* __restrict__ a_in, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = fe_is_canonical(fe_load<FrParams>(a_in + 8 * (uint64_t)i)) ? 1 : 0;
}

constexpr int fr29_out_words(int op) { return op == 0 || op == 5 ? 8 : op == 3 ? 5 * FR29_L : op == 4 ? 3 * FR29_L : FR29_L; }

__global__ __launch_bounds__(64) void k_fr29_selftest(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint32_t n, int op) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr9 u, v, w;
#pragma unroll
    for (int l = 0; l < FR29_L; l++) {
        u.v[l] = in[(uint64_t)FR29_IN_WORDS * i + l];
        v.v[l] = in[(uint64_t)FR29_IN_WORDS * i + FR29_L + l];
        w.v[l] = in[(uint64_t)FR29_IN_WORDS * i + 2 * FR29_L + l];
    }
    auto put9 = [&](uint32_t* o, const Fr9& x) {
#pragma unroll
        for (int l = 0; l < FR29_L; l++) o[l] = x.v[l];
    };
    auto put8 = [&](uint32_t* o, const Fr& x) {
#pragma unroll
        for (int l = 0; l < 8; l++) o[l] = x.v[l];
    };
    if (op == 0) {
        put8(out + (uint64_t)fr29_out_words(0) * i, fr9_canon_pack(u));
    } else if (op == 1) {
        put9(out + (uint64_t)fr29_out_words(1) * i, fr9_reduce_weak(u));
    } else if (op == 2) {
        put9(out + (uint64_t)fr29_out_words(2) * i, fr9_mul(u, v));
    } else if (op == 3) {                                            // the forward butterfly, in the order of lds_ntt_stages<false>
        uint32_t* o = out + (uint64_t)fr29_out_words(3) * i;
        const Fr9 x = fr9_add(u, v);
        put9(o, x);
        put9(o + FR29_L, fr9_reduce_weak(x));
        put9(o + 2 * FR29_L, fr9_mul(fr9_sub_raw<5>(u, v), w));
        put9(o + 3 * FR29_L, fr9_mul(fr9_sub<5>(u, v), w));
        put9(o + 4 * FR29_L, fr9_sub<5>(u, v));                      // the span-2 stage: no product
    } else if (op == 4) {                                            // the inverse butterfly
        uint32_t* o = out + (uint64_t)fr29_out_words(4) * i;
        const Fr9 t = fr9_mul(v, w);
        put9(o, t);
        put9(o + FR29_L, fr9_add(u, t));
        put9(o + 2 * FR29_L, fr9_sub<2>(u, t));
    } else {
        Fr x;
#pragma unroll
        for (int l = 0; l < 8; l++) x.v[l] = u.v[l];
        put8(out + (uint64_t)fr29_out_words(5) * i, fr9_pack_exact(fr9_unpack(x)));
    }
}

namespace {

bool words_below_r(const uint8_t* s) {                               // 32 little-endian bytes < r ?
    for (int j = 7; j >= 0; j--) {
        const uint32_t v = (uint32_t)s[4 * j] | (uint32_t)s[4 * j + 1] << 8 | (uint32_t)s[4 * j + 2] << 16 | (uint32_t)s[4 * j + 3] << 24;
        if (v != FR_MOD_HOST[j]) return v < FR_MOD_HOST[j];
    }
    return false;
}
bool lazy_limbs_ok(const uint32_t* l) {                              // weakly normalised, top limb at most that of 64 r
    for (int k = 0; k < FR29_L - 1; k++)
        if (l[k] > FR29_WEAK_LIMB) return false;
    return l[FR29_L - 1] <= FR29_TOP_64R;
}
bool factor_limbs_ok(const uint32_t* l) {                            // exact limbs and a value below r: what a factor read from memory is
    for (int k = 0; k < FR29_L - 1; k++)
        if (l[k] > FR29_MASK) return false;
    for (int k = FR29_L - 1; k >= 0; k--)
        if (l[k] != FR29_MOD_HOST[k]) return l[k] < FR29_MOD_HOST[k];
    return false;
}
inline dim3 grid64(size_t n) { return dim3((unsigned)((n + 63) / 64)); }

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" int zk_selftest_fr(int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) {
    if (op != 0 && op != 1) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fr: an op other than 0 / 1");
    if (!a || !out || !n || n >= ((size_t)1 << 24) || (op == 0 && !b)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fr: null argument or no operands");
    if (op == 0)
        for (size_t i = 0; i < n; i++)
            if (!words_below_r(a + 32 * i) || !words_below_r(b + 32 * i)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fr: an operand is >= r");
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    const size_t out_bytes = op == 0 ? (size_t)FR_OUTS * 32 * n : n;
    DevBuf da, db, dout;
    ZKCHK(da.alloc(32 * n));
    ZKCHK(dout.alloc(out_bytes));
    HIPCHK(hipMemcpyAsync(da.p, a, 32 * n, hipMemcpyHostToDevice, s));
    if (op == 0) {
        ZKCHK(db.alloc(32 * n));
        HIPCHK(hipMemcpyAsync(db.p, b, 32 * n, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fr_selftest, grid64(n), dim3(64), 0, s, dout.as<uint32_t>(), (const uint32_t*)da.as<uint32_t>(), (const uint32_t*)db.as<uint32_t>(), (uint32_t)n);
    } else {
        hipLaunchKernelGGL(k_fr_canonical_selftest, grid64(n), dim3(64), 0, s, dout.as<uint8_t>(), (const uint32_t*)da.as<uint32_t>(), (uint32_t)n);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}

extern "C" int zk_selftest_fr29(int op, const uint32_t* operands, size_t n, uint32_t* out) {
    if (op < 0 || op > 5) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fr29: an op other than 0 .. 5");
    if (!operands || !out || !n || n >= ((size_t)1 << 24)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fr29: null argument or no operands");
    if (op != 5)
        for (size_t i = 0; i < n; i++) {
            const uint32_t* l = operands + (size_t)FR29_IN_WORDS * i;
            if (!lazy_limbs_ok(l) || (op >= 2 && !lazy_limbs_ok(l + FR29_L)))
                ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fr29: a limb above 2^29 + 7 or a top limb above that of 64 r");
            if (op >= 3 && !factor_limbs_ok(l + 2 * FR29_L)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_fr29: w has a limb above 2^29 - 1 or a value >= r");
        }
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    const size_t in_bytes = (size_t)FR29_IN_WORDS * 4 * n, out_bytes = (size_t)fr29_out_words(op) * 4 * n;
    DevBuf din, dout;
    ZKCHK(din.alloc(in_bytes));
    ZKCHK(dout.alloc(out_bytes));
    HIPCHK(hipMemcpyAsync(din.p, operands, in_bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_fr29_selftest, grid64(n), dim3(64), 0, s, dout.as<uint32_t>(), (const uint32_t*)din.as<uint32_t>(), (uint32_t)n, op);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZK_OK;
}
