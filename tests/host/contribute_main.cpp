// The host half of zk_groth16_pk_contribute on its own (csrc/contribute_scalar.h: no HIP in it), built by tests/test_contribute_host.py with
// -fsanitize=address,undefined.  For the edge scalars and 1000 random ones: k k^-1 = 1 (mod r) with k^-1 below r, the range test on both sides of r,
// and the byte forms the C-ABI reads.  (The split through the endomorphism and the signed 4-bit digits this program also checked belonged to the
// kernel that was measured and dropped -- DESIGN 2q; the shipped route splits and recodes on the device, where tests/test_gpu_group_law.py holds it.)
// The arithmetic that checks is written here a second time, on unsigned __int128 columns with a bitwise reduction: nothing of the header checks itself.
#include "../../zukelang_amd/csrc/contribute_scalar.h"

#include <stdio.h>
#include <stdlib.h>

using namespace zk;
typedef unsigned __int128 u128;

struct U512 {
    uint64_t w[8];
};
static U512 mul256(const uint64_t a[4], const uint64_t b[4]) {
    U512 r = {{0, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (u128)a[i] * b[j] + r.w[i + j];
            r.w[i + j] = (uint64_t)c;
            c >>= 64;
        }
        r.w[i + 4] = (uint64_t)c;
    }
    return r;
}
// x mod r, bit by bit from the top
static void mod_r(uint64_t out[4], const U512& x) {
    uint64_t rem[4] = {0, 0, 0, 0};
    for (int bit = 511; bit >= 0; bit--) {
        const uint64_t top = rem[3] >> 63;
        for (int i = 3; i > 0; i--) rem[i] = (rem[i] << 1) | (rem[i - 1] >> 63);
        rem[0] = (rem[0] << 1) | ((x.w[bit >> 6] >> (bit & 63)) & 1u);
        bool ge = top != 0;
        if (!ge) {
            ge = true;
            for (int i = 3; i >= 0; i--)
                if (rem[i] != CS_R[i]) { ge = rem[i] > CS_R[i]; break; }
        }
        if (ge) {
            uint64_t borrow = 0;
            for (int i = 0; i < 4; i++) {
                const uint64_t t = rem[i] - CS_R[i], t2 = t - borrow;
                borrow = (rem[i] < CS_R[i]) | (t < borrow);
                rem[i] = t2;
            }
        }
    }
    for (int i = 0; i < 4; i++) out[i] = rem[i];
}
static void mulmod(uint64_t out[4], const uint64_t a[4], const uint64_t b[4]) { mod_r(out, mul256(a, b)); }
static bool eq(const uint64_t a[4], const uint64_t b[4]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; }
static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t splitmix() {
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static int g_fail = 0;
#define EXPECT(c, ...)                          \
    do {                                        \
        if (!(c)) {                             \
            g_fail++;                           \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);       \
            fprintf(stderr, "\n");              \
        }                                       \
    } while (0)

static void check_scalar(const uint64_t k[4], const char* what) {
    EXPECT(cs_canonical(k), "%s is not below r", what);
    if (cs_is_zero(k)) return;
    uint64_t inv[4], one[4], back[4];
    cs_fr_inv(inv, k);
    EXPECT(cs_canonical(inv) && !cs_is_zero(inv), "%s: the inverse is not in [1, r)", what);
    mulmod(one, k, inv);
    EXPECT(cs_is_one(one), "%s: k * k^-1 != 1", what);
    cs_fr_inv(back, inv);
    EXPECT(eq(back, k), "%s: (k^-1)^-1 != k", what);
}

int main() {
    // lambda = z^2 - 1, z = -0xd201000000010000: the scalars around it are where a 128-bit half ends
    const uint64_t lambda[4] = {0x00000000ffffffffull, 0xac45a4010001a402ull, 0, 0};
    const uint64_t one[4] = {1, 0, 0, 0}, two[4] = {2, 0, 0, 0}, zero[4] = {0, 0, 0, 0};
    uint64_t rm1[4], rm2[4], lp1[4], rml[4], half[4];
    (void)cs_sub(rm1, CS_R, one);
    (void)cs_sub(rm2, CS_R, two);
    (void)cs_add(lp1, lambda, one);
    (void)cs_sub(rml, CS_R, lambda);
    memcpy(half, rm1, 32);
    cs_shr1(half);                                   // (r - 1) / 2
    const uint64_t p128m1[4] = {~(uint64_t)0, ~(uint64_t)0, 0, 0}, p128[4] = {0, 0, 1, 0}, p254[4] = {0, 0, 0, (uint64_t)1 << 62};
    struct { const uint64_t* k; const char* name; } edge[] = {
        {zero, "0"}, {one, "1"}, {two, "2"}, {rm1, "r-1"}, {rm2, "r-2"}, {lambda, "lambda"}, {lp1, "lambda+1"}, {p128m1, "2^128-1"}, {p128, "2^128"},
        {rml, "r-lambda"}, {half, "(r-1)/2"}, {p254, "2^254"},
    };
    for (const auto& e : edge) check_scalar(e.k, e.name);
    {
        uint64_t inv[4];
        cs_fr_inv(inv, one);
        EXPECT(cs_is_one(inv), "1^-1 != 1");
        cs_fr_inv(inv, rm1);
        EXPECT(eq(inv, rm1), "(r-1)^-1 != r-1");
        uint64_t rp1[4];
        (void)cs_add(rp1, CS_R, one);
        const uint64_t ones[4] = {~(uint64_t)0, ~(uint64_t)0, ~(uint64_t)0, ~(uint64_t)0};
        EXPECT(!cs_canonical(CS_R) && !cs_canonical(rp1) && !cs_canonical(ones), "r, r + 1 or 2^256 - 1 counts as canonical");
        EXPECT(cs_is_zero(zero) && !cs_is_zero(one) && !cs_is_zero(p254), "zero test");
    }
    for (int i = 0; i < 1000; i++) {
        uint64_t k[4] = {splitmix(), splitmix(), splitmix(), splitmix() >> 1};
        while (!cs_canonical(k)) k[3] >>= 1;
        char name[32];
        snprintf(name, sizeof name, "random %d", i);
        check_scalar(k, name);
    }
    // the byte forms the C-ABI reads
    {
        uint8_t bytes[32];
        uint64_t back[4];
        cs_to_bytes(bytes, rm1);
        cs_load(back, bytes);
        EXPECT(eq(back, rm1) && bytes[0] == 0x00 && bytes[31] == 0x73, "little-endian byte form");
    }
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("contribute_scalar ok\n");
    return 0;
}
