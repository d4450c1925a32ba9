// zk_selftest_group (include/zkmi355x.h): the host half.  Every check of the arguments happens here, on the bytes, before the device is touched; the
// operands then travel as dense little-endian words of the plain integers and the unit that builds the form asked for runs its kernel
// (msm.cuh: GroupForm, group_selftest_*; group_selftest.cuh: what the kernels share).
#include "msm.cuh"
#include "pairing_consts.h"

#include <string.h>
#include <vector>

namespace zk {
namespace {

enum SecondOperand { SECOND_NONE, SECOND_XYZZ, SECOND_AFFINE, SECOND_AFFINE_NO_IDENTITY, SECOND_SCALAR };
SecondOperand second_operand(int form) {
    switch (form) {
    case GROUP_FORM_ADD: case GROUP_FORM_ADD_RAW_MEM: case GROUP_FORM_ADD_SLOTS: case GROUP_FORM_JAC_ADD: return SECOND_XYZZ;
    case GROUP_FORM_DBL: case GROUP_FORM_DBL_AFF: case GROUP_FORM_DBL_SLOTS: case GROUP_FORM_JAC_DBL: return SECOND_NONE;
    case GROUP_FORM_MADD: case GROUP_FORM_MMADD: case GROUP_FORM_MADD_INLINE: case GROUP_FORM_MMADD_INLINE: return SECOND_AFFINE;
    case GROUP_FORM_MUL: return SECOND_SCALAR;
    default: return SECOND_AFFINE_NO_IDENTITY;          // table entries (madd without the identity test, the parked form) and jac_madd
    }
}
// 48 big-endian bytes -> 12 little-endian words; false when the integer is >= p
bool fp_words_from_be(uint32_t* w, const uint8_t* p) {
    for (int j = 0; j < 12; j++) {
        const uint8_t* q = p + 44 - 4 * j;
        w[j] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
    }
    for (int j = 5; j >= 0; j--) {
        const uint64_t v = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
        if (v != HP_P[j]) return v < HP_P[j];
    }
    return false;
}
// `coords` field elements in the wire's order (G2: imaginary part | real part) -> the device's (c0 | c1)
bool coords_from_wire(std::vector<uint32_t>& dst, const uint8_t* src, size_t coords, bool g2) {
    dst.resize(coords * (g2 ? 24 : 12));
    for (size_t c = 0; c < coords; c++) {
        if (!g2) {
            if (!fp_words_from_be(&dst[12 * c], src + 48 * c)) return false;
        } else {
            if (!fp_words_from_be(&dst[24 * c + 12], src + 96 * c)) return false;
            if (!fp_words_from_be(&dst[24 * c], src + 96 * c + 48)) return false;
        }
    }
    return true;
}
bool scalar_is_canonical(const uint8_t* s) {
    for (int j = 3; j >= 0; j--) {
        uint64_t v = 0;
        for (int k = 7; k >= 0; k--) v = (v << 8) | s[8 * j + k];
        if (v != HP_R[j]) return v < HP_R[j];
    }
    return false;
}

}  // namespace
}  // namespace zk

using namespace zk;
extern "C" int zk_selftest_group(int group, int form, int rep, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) {
    if (!a || !out || !n || (group != 0 && group != 1) || form < 0 || form >= GROUP_FORM_COUNT || (rep != 0 && rep != 1))
        ZK_FAIL(ZK_ERR_ARG, "zk_selftest_group: null argument, no operands, a group other than 0 (G1) / 1 (G2), an unknown form, or a rep other than 0 / 1");
    const bool g2 = group == 1;
    if (form == GROUP_FORM_MADD_PARKED && !g2) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_group: the parked mixed addition is built for G2 only");
    const SecondOperand second = second_operand(form);
    if (second != SECOND_NONE && !b) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_group: this form reads b");
    std::vector<uint32_t> wa, wb;
    if (!coords_from_wire(wa, a, 4 * n, g2)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_group: a coordinate of a is >= p");
    if (second == SECOND_XYZZ) {
        if (!coords_from_wire(wb, b, 4 * n, g2)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_group: a coordinate of b is >= p");
    } else if (second == SECOND_AFFINE || second == SECOND_AFFINE_NO_IDENTITY) {
        if (!coords_from_wire(wb, b, 2 * n, g2)) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_group: a coordinate of b is >= p");
        if (second == SECOND_AFFINE_NO_IDENTITY) {
            const size_t pw = g2 ? 48 : 24;
            for (size_t i = 0; i < n; i++) {
                uint32_t o = 0;
                for (size_t k = 0; k < pw; k++) o |= wb[pw * i + k];
                if (!o) ZK_FAIL(ZK_ERR_ARG, "zk_selftest_group: this form's second operand is never the identity");
            }
        }
    } else if (second == SECOND_SCALAR) {
        for (size_t i = 0; i < n; i++)
            if (!scalar_is_canonical(b + 32 * i)) ZK_FAIL(ZK_ERR_SCALAR_RANGE, "zk_selftest_group: a scalar is >= r");
        wb.resize(8 * n);
        memcpy(wb.data(), b, 32 * n);          // canonical scalars are little-endian bytes on the wire: the device's words
    }
    ZKCHK(ensure_init());
    DeviceScope ds(0);
    hipStream_t s = ctx().stream;
    const Curve curve = g2 ? CURVE_G2 : CURVE_G1;
    const size_t raw_xyzz = g2 ? 512 : 256;          // RawLayout<F>::XYZZ
    const size_t scratch = form == GROUP_FORM_MUL ? 16 * raw_xyzz * n : form == GROUP_FORM_ADD_RAW_MEM ? raw_xyzz * n : 0;
    DevBuf da, db, dout, dscratch;
    ZKCHK(da.alloc(wa.size() * 4));
    ZKCHK(db.alloc(wb.size() * 4));
    ZKCHK(dout.alloc(xyzz_bytes(curve) * n));
    ZKCHK(dscratch.alloc(scratch));
    HIPCHK(hipMemcpyAsync(da.p, wa.data(), wa.size() * 4, hipMemcpyHostToDevice, s));
    if (!wb.empty()) HIPCHK(hipMemcpyAsync(db.p, wb.data(), wb.size() * 4, hipMemcpyHostToDevice, s));
    const GroupSelftest t{curve, form, rep, da.as<uint8_t>(), db.as<uint8_t>(), (uint64_t)n, dout.as<uint8_t>(), dscratch.as<uint8_t>()};
    if (form <= GROUP_FORM_ADD_RAW_MEM) ZKCHK(group_selftest_red(t, s));
    else if (form <= GROUP_FORM_MMADD) ZKCHK(group_selftest_acc_g2(t, s));
    else if (form <= GROUP_FORM_MADD_PARKED) ZKCHK(g2 ? group_selftest_acc_g2i(t, s) : group_selftest_acc_g1(t, s));
    else if (form <= GROUP_FORM_DBL_SLOTS) ZKCHK(group_selftest_tail(t, s));
    else ZKCHK(group_selftest_derive(t, s));
    return points_xyzz_to_bytes(curve, dout.p, n, out, s);          // waits for the stream
}
