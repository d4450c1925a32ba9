// The order in which a verifier meets the points of a key and of a proof, written ONCE: the verdict kinds of the point decoders (msm_points.hip) and
// the status each becomes, where a proof's points lie in its bytes, which bad point decides a proof's status, and which bad point of a key fails the
// call -- the order of the host verifiers of pairing_host.hip (Groth16.verify of groth16.ml:163-173, Verify.f of pinocchio.ml:254-420), which the
// batched verifiers (pairing_dev.hip) and the resident keys (verify_resident.hip) reproduce on the host and on the device.  Nothing of HIP here:
// tests/host/verdict_order_main.cpp builds this header with plain g++.
#pragma once
#include "../../include/zkmi355x.h"

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define ZK_HOST_DEVICE __host__ __device__
#else
#define ZK_HOST_DEVICE
#endif

namespace zk {

// one byte per point, and per proof: 0 good, else the first defect met
enum : uint8_t { VERDICT_CURVE = 1, VERDICT_ENCODING = 2, VERDICT_SUBGROUP = 4, VERDICT_SCALAR = 8 };          // 8: a public input >= r
inline int verdict_code(uint8_t v) { return v == 0 ? ZK_OK : v == VERDICT_ENCODING ? ZK_ERR_ARG : v == VERDICT_SCALAR ? ZK_ERR_SCALAR_RANGE : ZK_ERR_NOT_ON_CURVE; }

// where a proof's points lie in its bytes, and the order in which the host verifier meets them (bit 7: a G2 point)
struct VkPlan {
    uint32_t stride, n1, n2, pairs, products;
    uint32_t off1[6], off2[2];
    uint32_t norder;
    uint8_t order[8];
};
static const VkPlan PLAN_GROTH16 = {384, 2, 1, 3, 1, {0, 288, 0, 0, 0, 0}, {96, 0}, 3, {0, 0x80, 1, 0, 0, 0, 0, 0}};                          // A | B | C
static const VkPlan PLAN_PINOCCHIO = {960, 6, 2, 13, 5, {0, 288, 384, 480, 768, 864}, {96, 576}, 8, {0, 0x80, 1, 2, 3, 0x81, 4, 5}};         // vv ww yy h vavv waww yayy bvwy

// The same points where a proof arrives COMPRESSED, as the reference's proof record holds them (48 B per G1 point, 96 B per G2 point, in the order
// above): the proof's stride and the offsets that stand for off1 / off2.  Half of the plan's, every one a multiple of 16.
struct VkWire {
    uint32_t stride;
    uint32_t off1[6], off2[2];
};
static const VkWire WIRE_GROTH16 = {192, {0, 144, 0, 0, 0, 0}, {48, 0}};
static const VkWire WIRE_PINOCCHIO = {480, {0, 144, 192, 240, 384, 432}, {48, 288}};

// Proof i's code: its first bad point's verdict in the plan's order, else 8 when one of its public inputs is >= r (bad[i]), else 0.  The verdict lists
// are laid out per proof: G1 point q of proof i at v1[n1 i + q], G2 point q at v2[n2 i + q].
ZK_HOST_DEVICE inline uint8_t proof_code(const VkPlan& p, const uint8_t* v1, const uint8_t* v2, const uint8_t* bad, uint32_t i) {
    uint8_t c = 0;
    for (uint32_t k = 0; k < p.norder && !c; k++) {
        const uint8_t o = p.order[k];
        c = o & 0x80 ? v2[(size_t)p.n2 * i + (o & 0x7f)] : v1[(size_t)p.n1 * i + o];
    }
    if (!c && bad[i]) c = VERDICT_SCALAR;
    return c;
}

// The first defect of a key in the host verifier's order, with the message that position carries; verdict 0: the key is good.
struct KeyDefect { uint8_t verdict; const char* what; };
// Groth16: gm, d, then ltgm_io[k].   v1 = ltgm_io[n_io], v2 = gm | d
inline KeyDefect groth16_key_defect(const uint8_t* v1, const uint8_t* v2, size_t n_io) {
    for (size_t q = 0; q < 2; q++)
        if (v2[q]) return {v2[q], "verify: bad G2 point"};
    for (size_t k = 0; k < n_io; k++)
        if (v1[k]) return {v1[k], "verify: bad G1 point in the key"};
    return {0, nullptr};
}
// Pinocchio: one aw bgm, then one2 av ay gm2 bgm2 yt, then vv_io[k] yy_io[k] ww_io[k] for every k.
// v1 = one | aw | bgm | vv_io[n_io] | yy_io[n_io], v2 = one2 | av | ay | gm2 | bgm2 | yt | ww_io[n_io]
inline KeyDefect pinocchio_key_defect(const uint8_t* v1, const uint8_t* v2, size_t n_io) {
    for (size_t q = 0; q < 3; q++)
        if (v1[q]) return {v1[q], "verify: bad G1 point"};
    for (size_t q = 0; q < 6; q++)
        if (v2[q]) return {v2[q], "verify: bad G2 point"};
    for (size_t k = 0; k < n_io; k++) {
        const uint8_t v = v1[3 + k] ? v1[3 + k] : v1[3 + n_io + k] ? v1[3 + n_io + k] : v2[6 + k];
        if (v) return {v, "verify: bad point in the key"};
    }
    return {0, nullptr};
}

// the GT encoding of 1: twelve 48-byte big-endian coefficients, the first of them 1
inline void gt_one_bytes(uint8_t out[576]) {
    memset(out, 0, 576);
    out[47] = 1;
}

}  // namespace zk
