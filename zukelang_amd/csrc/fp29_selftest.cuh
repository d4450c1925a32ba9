// zk_selftest_fp29: what its two translation units share (fp29_selftest.hip, fp29_selftest_inline.hip).  Op numbers are those of include/zkmi355x.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zk {

static constexpr int FP29_ST_IN_WORDS = 3 * 16;          // a | b | c, each 14 limbs in a 16-word slot
static constexpr int FP29_OP_CANON = 0, FP29_OP_CARRY = 1, FP29_OP_ADD = 2, FP29_OP_DBL = 3, FP29_OP_PACK = 4, FP29_OP_INV = 5;
static constexpr int FP29_OP_ZERO = 8;                   // 8, 9, 10: fe_is_zero<B> for the three bounds below
static constexpr int FP29_OP_ROWS = 16;                  // 16 + 16 * fn + row: fn 0 fe_sub, 1 fe_neg, 2 fe_neg_lazy, 3 fe_sub_sub_dbl
// 2: the smallest bound with a slow path.  64: FP_REST.  192: the largest bound any call site of the shipped kernels instantiates fe_is_zero with
// ("The base field on bare limbs", says how that was found)
static constexpr int FP29_ZERO_B0 = 2, FP29_ZERO_B1 = 64, FP29_ZERO_B2 = 192;

constexpr int fp29_st_out_words(int op) { return op == FP29_OP_PACK ? 14 + 12 : op == FP29_OP_INV ? 2 * 14 : (op >= FP29_OP_ZERO && op < FP29_OP_ZERO + 3) ? 1 : 14; }

// ORs bit 1 of every lane's flag word: fe_is_zero<B> as a unit that defines ZK_FP_INLINE_MUL compiles it (slow path: fp_is_zero_mod_p_inline)
int fp29_selftest_zero_inline(uint32_t* d_out, const uint32_t* d_in, uint32_t n, int which, hipStream_t s);

}  // namespace zk
