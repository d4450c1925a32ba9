// Stand-alone check of csrc/verdict_order.h (tests/test_verdict_order.py builds it with g++ under AddressSanitizer + UBSan and runs it).
// Every expected order is written out here, not derived from the header.  Exit status 0 and "verdict_order ok" on stdout: every check held.
#include "../../zukelang_amd/csrc/verdict_order.h"

#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

using namespace zk;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

// a point of a proof as the host verifier meets it: its group (1: G2), its index among the proof's points of that group, its offset in the proof
struct Pos { int g2; uint32_t q, off; };
static const Pos GROTH16[3] = {{0, 0, 0}, {1, 0, 96}, {0, 1, 288}};                                                                         // A B C
static const Pos PINOCCHIO[8] = {{0, 0, 0}, {1, 0, 96}, {0, 1, 288}, {0, 2, 384}, {0, 3, 480}, {1, 1, 576}, {0, 4, 768}, {0, 5, 864}};     // vv ww yy h vavv waww yayy bvwy

static void check_plan(const VkPlan& p, const Pos* want, uint32_t n, uint32_t stride, uint32_t n1, uint32_t n2) {
    CHECK(p.norder == n && p.stride == stride && p.n1 == n1 && p.n2 == n2);
    for (uint32_t k = 0; k < n; k++) {
        CHECK((p.order[k] & 0x80 ? 1 : 0) == want[k].g2 && (uint32_t)(p.order[k] & 0x7f) == want[k].q);
        CHECK((want[k].g2 ? p.off2[want[k].q] : p.off1[want[k].q]) == want[k].off);
    }
    // proofs 0 and 2 of 3: the strides n1 i + q / n2 i + q.  Proof 1 is bad everywhere, so a wrong stride shows.
    for (uint32_t i = 0; i < 3; i += 2) {
        std::vector<uint8_t> v1(3 * n1, 0), v2(3 * n2, 0), bad(3, 0);
        auto at = [&](uint32_t k) -> uint8_t& { return want[k].g2 ? v2[n2 * i + want[k].q] : v1[n1 * i + want[k].q]; };
        for (uint32_t q = 0; q < n1; q++) v1[n1 * 1 + q] = 2;
        for (uint32_t q = 0; q < n2; q++) v2[n2 * 1 + q] = 2;
        bad[1] = 1;
        CHECK(proof_code(p, v1.data(), v2.data(), bad.data(), i) == 0);          // a clean proof
        CHECK(proof_code(p, v1.data(), v2.data(), bad.data(), 1) == 2);
        bad[i] = 1;
        CHECK(proof_code(p, v1.data(), v2.data(), bad.data(), i) == 8);          // the scalar defect alone
        for (uint32_t k = 0; k < n; k++) {                                       // ... loses to any point defect
            at(k) = 4;
            CHECK(proof_code(p, v1.data(), v2.data(), bad.data(), i) == 4);
            at(k) = 0;
        }
        bad[i] = 0;
        for (uint32_t k = 0; k < n; k++)                                         // two bad verdicts: the earlier position wins, whatever the kinds
            for (uint32_t l = k + 1; l < n; l++) {
                at(k) = 4; at(l) = 2;
                CHECK(proof_code(p, v1.data(), v2.data(), bad.data(), i) == 4);
                at(k) = 1; at(l) = 4;
                CHECK(proof_code(p, v1.data(), v2.data(), bad.data(), i) == 1);
                at(k) = 0; at(l) = 0;
            }
    }
}

// a key position in the host verifier's order: the list (1: the G2 list), the index in it, the message
struct KeyPos { int g2; size_t idx; const char* what; };
typedef KeyDefect (*KeyFn)(const uint8_t*, const uint8_t*, size_t);
static void check_key(KeyFn fn, const std::vector<KeyPos>& want, size_t len1, size_t len2, size_t n_io) {
    std::vector<uint8_t> v1(len1 + 1, 0), v2(len2 + 1, 0);          // one spare byte each: a list of length 0 still has an address
    CHECK(fn(v1.data(), v2.data(), n_io).verdict == 0);
    size_t seen1 = 0, seen2 = 0;
    for (const KeyPos& k : want) (k.g2 ? seen2 : seen1)++;
    CHECK(seen1 == len1 && seen2 == len2);                          // the order visits every point of the key once
    for (size_t a = 0; a < want.size(); a++) {
        auto at = [&](size_t k) -> uint8_t& { return want[k].g2 ? v2[want[k].idx] : v1[want[k].idx]; };
        at(a) = 4;                                                  // alone, as the mildest kind
        KeyDefect d = fn(v1.data(), v2.data(), n_io);
        CHECK(d.verdict == 4 && std::string(d.what) == want[a].what);
        for (size_t b = a + 1; b < want.size(); b++) {              // the later defect of a "stronger" kind (kind priority would pick it) does not win
            at(b) = 2;
            d = fn(v1.data(), v2.data(), n_io);
            CHECK(d.verdict == 4 && std::string(d.what) == want[a].what);
            at(b) = 0;
        }
        at(a) = 0;
    }
}

int main() {
    check_plan(PLAN_GROTH16, GROTH16, 3, 384, 2, 1);
    check_plan(PLAN_PINOCCHIO, PINOCCHIO, 8, 960, 6, 2);
    CHECK(PLAN_GROTH16.pairs == 3 && PLAN_GROTH16.products == 1 && PLAN_PINOCCHIO.pairs == 13 && PLAN_PINOCCHIO.products == 5);

    static const size_t N_IO[3] = {0, 1, 3};
    for (size_t n_io : N_IO) {
        // Groth16: gm, d, then ltgm_io[k].  G1 list = ltgm_io, G2 list = gm | d
        std::vector<KeyPos> g = {{1, 0, "verify: bad G2 point"}, {1, 1, "verify: bad G2 point"}};
        for (size_t k = 0; k < n_io; k++) g.push_back({0, k, "verify: bad G1 point in the key"});
        check_key(groth16_key_defect, g, n_io, 2, n_io);
        // Pinocchio: one aw bgm, then one2 av ay gm2 bgm2 yt, then vv_io[k] yy_io[k] ww_io[k] for every k.
        // G1 list = one aw bgm vv_io[n_io] yy_io[n_io], G2 list = one2 av ay gm2 bgm2 yt ww_io[n_io]
        std::vector<KeyPos> p;
        for (size_t q = 0; q < 3; q++) p.push_back({0, q, "verify: bad G1 point"});
        for (size_t q = 0; q < 6; q++) p.push_back({1, q, "verify: bad G2 point"});
        for (size_t k = 0; k < n_io; k++) {
            p.push_back({0, 3 + k, "verify: bad point in the key"});
            p.push_back({0, 3 + n_io + k, "verify: bad point in the key"});
            p.push_back({1, 6 + k, "verify: bad point in the key"});
        }
        check_key(pinocchio_key_defect, p, 3 + 2 * n_io, 6 + n_io, n_io);
    }

    CHECK(verdict_code(0) == ZK_OK && verdict_code(1) == ZK_ERR_NOT_ON_CURVE && verdict_code(2) == ZK_ERR_ARG);
    CHECK(verdict_code(4) == ZK_ERR_NOT_ON_CURVE && verdict_code(8) == ZK_ERR_SCALAR_RANGE);
    CHECK(VERDICT_CURVE == 1 && VERDICT_ENCODING == 2 && VERDICT_SUBGROUP == 4 && VERDICT_SCALAR == 8);

    uint8_t one[576];
    memset(one, 0xAA, sizeof one);
    gt_one_bytes(one);
    for (int k = 0; k < 576; k++) CHECK(one[k] == (k == 47 ? 1 : 0));

    printf("verdict_order ok\n");
    return 0;
}
