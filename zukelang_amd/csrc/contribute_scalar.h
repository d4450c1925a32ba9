// Host half of zk_groth16_pk_contribute (groth16.hip, contribute.hip): delta' as 256-bit words -- its range checks and its inverse mod r, computed once
// per call on the host.  Plain C++, no HIP: tests/host/contribute_main.cpp runs this file under AddressSanitizer + UBSan.
#pragma once
#include <stdint.h>
#include <string.h>

namespace zk {

// r, little-endian 64-bit words
static const uint64_t CS_R[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};

static inline void cs_load(uint64_t w[4], const uint8_t b[32]) { memcpy(w, b, 32); }          // little-endian hosts only, as everywhere in the library
static inline void cs_to_bytes(uint8_t b[32], const uint64_t w[4]) { memcpy(b, w, 32); }
static inline bool cs_is_zero(const uint64_t a[4]) { return (a[0] | a[1] | a[2] | a[3]) == 0; }
static inline bool cs_is_one(const uint64_t a[4]) { return a[0] == 1 && (a[1] | a[2] | a[3]) == 0; }
static inline int cs_cmp(const uint64_t a[4], const uint64_t b[4]) {
    for (int i = 3; i >= 0; i--)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
static inline bool cs_canonical(const uint64_t a[4]) { return cs_cmp(a, CS_R) < 0; }
static inline uint64_t cs_add(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a[i] + b[i];
        r[i] = (uint64_t)c;
        c >>= 64;
    }
    return (uint64_t)c;
}
static inline uint64_t cs_sub(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {
    uint64_t borrow = 0;
    for (int i = 0; i < 4; i++) {
        const uint64_t t = a[i] - b[i], t2 = t - borrow;
        borrow = (a[i] < b[i]) | (t < borrow);
        r[i] = t2;
    }
    return borrow;
}
static inline void cs_shr1(uint64_t a[4]) {
    for (int i = 0; i < 3; i++) a[i] = (a[i] >> 1) | (a[i + 1] << 63);
    a[3] >>= 1;
}
// x / 2 mod r for x < r: r < 2^255, so x + r fits 256 bits
static inline void cs_half_mod(uint64_t x[4]) {
    if (x[0] & 1) (void)cs_add(x, x, CS_R);
    cs_shr1(x);
}
static inline void cs_sub_mod(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {
    if (cs_sub(r, a, b)) (void)cs_add(r, r, CS_R);
}
// out = a^-1 mod r for 0 < a < r (binary extended Euclid: u = x1 a, v = x2 a mod r throughout)
static inline void cs_fr_inv(uint64_t out[4], const uint64_t a[4]) {
    uint64_t u[4], v[4], x1[4] = {1, 0, 0, 0}, x2[4] = {0, 0, 0, 0};
    memcpy(u, a, 32);
    memcpy(v, CS_R, 32);
    while (!cs_is_one(u) && !cs_is_one(v)) {
        while (!(u[0] & 1)) { cs_shr1(u); cs_half_mod(x1); }
        while (!(v[0] & 1)) { cs_shr1(v); cs_half_mod(x2); }
        if (cs_cmp(u, v) >= 0) { (void)cs_sub(u, u, v); cs_sub_mod(x1, x1, x2); }
        else { (void)cs_sub(v, v, u); cs_sub_mod(x2, x2, x1); }
    }
    memcpy(out, cs_is_one(u) ? x1 : x2, 32);
}

}  // namespace zk
