#!/usr/bin/env python3
"""Generates zukelang_amd/csrc/ff_mul_gen.cuh: straight-line Montgomery multiplication
(finely integrated product scanning) for gfx950, N = 8 (Fr) 32-bit limbs (gen() also handles N = 12, the
scheme Fp used before it moved to radix 2^29).

Every column of partial products is ONE asm statement (<= 30 operands) made of
    v_mad_u64_u32 acc[0:1], vcc, x, y, acc[0:1]   ; 32x32 product added into the 64-bit pair
    v_addc_co_u32 acc2, vcc, 0, acc2, vcc          ; carry into the third word
so the compiler's per-statement hazard padding (one s_nop) is paid ~4 times per column instead of
once per product, and no zero-extension moves exist at all.  Modulus limbs travel in SGPRs.

It also generates zukelang_amd/csrc/fp_pair_gen.cuh: PAIRED Montgomery products of the base field Fp (14 limbs of
29 bits, R = 2^406, carry-free 64-bit columns; ff.cuh).  Two (at the end of an addition, three) independent products of
a group addition run side by side: every column of each product is ONE chain of v_mad_u64_u32 seeded with the shifted
carry of the column before, and the multiply-adds of the products alternate inside each asm statement, so a dependent
multiply-add is always two or more instructions away from its producer and no 64-bit add ever joins two partial chains
of one column.  The forms are
described by one list of steps (schedule()) that both the emitter and the integer model (model_*) consume: the model
replays the schedule on Python integers, checks the result, and checks that no accumulator reaches 2^64 at the worst
limb values each form admits.
It also generates zukelang_amd/csrc/fp2_lane_gen.cuh: the Montgomery product of Fp2 on ONE lane (lazy Karatsuba, three base
multiplications feeding two running reductions; see "Fp2 on ONE lane" below), with a schedule and an integer model of its own.
Run: python scripts/gen_mont_mul.py            (writes the three headers)
     python scripts/gen_mont_mul.py --check    (runs the integer model only)
"""
import os
import sys

FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FP = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB


def limbs(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def column_asm(pairs, kind):
    """pairs: list of (x_expr, y_expr); kind 'v' (y in VGPR) or 's' (y constant -> SGPR)."""
    lines = []
    ops = []
    for k, (x, y) in enumerate(pairs):
        xi, yi = 2 + 2 * k, 3 + 2 * k
        lines.append("v_mad_u64_u32 %%0, vcc, %%%d, %%%d, %%0" % (xi, yi))
        lines.append("v_addc_co_u32 %1, vcc, 0, %1, vcc")
        ops.append('"v"(%s)' % x)
        ops.append('"%s"(%s)' % (kind, y))
    body = "\\n\\t".join(lines)
    return '    asm("%s" : "+v"(lo), "+v"(hi) : %s : "vcc");' % (body, ", ".join(ops))


def chunks(lst, n):
    for i in range(0, len(lst), n):
        yield lst[i:i + n]


def gen(name, N, mod, inv):
    p = limbs(mod, N)
    out = []
    out.append("// %d-limb Montgomery product, modulus 0x%x" % (N, mod))
    out.append("FF_INLINE void mont_mul_%s(uint32_t* __restrict__ r, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b) {" % name)
    out.append("    uint64_t lo = 0;")
    out.append("    uint32_t hi = 0;")
    out.append("    uint32_t " + ", ".join("m%d" % i for i in range(N)) + ";")
    MAXP = 14   # products per asm statement: 2 + 2*14 = 30 operands
    for i in range(2 * N):
        if i < N:
            ab = [("a[%d]" % j, "b[%d]" % (i - j)) for j in range(i + 1)]
            mp = [("m%d" % j, "0x%08xu" % p[i - j]) for j in range(i)]
        else:
            ab = [("a[%d]" % j, "b[%d]" % (i - j)) for j in range(i - N + 1, N)]
            mp = [("m%d" % j, "0x%08xu" % p[i - j]) for j in range(i - N + 1, N)]
        for c in chunks(ab, MAXP):
            out.append(column_asm(c, "v"))
        for c in chunks(mp, MAXP):
            out.append(column_asm(c, "s"))
        if i < N:
            if inv == 0xFFFFFFFF:
                out.append("    m%d = 0u - (uint32_t)lo;" % i)
            else:
                out.append("    m%d = (uint32_t)lo * 0x%08xu;" % (i, inv))
            out.append(column_asm([("m%d" % i, "0x%08xu" % p[0])], "s"))
        else:
            out.append("    r[%d] = (uint32_t)lo;" % (i - N))
        if i < 2 * N - 1:
            out.append("    lo = (lo >> 32) | ((uint64_t)hi << 32); hi = 0;")
    out.append("}")
    return "\n".join(out)


# ====================================================================== Fp: paired products, radix 2^29
W29, L29 = 29, 14
M29 = (1 << W29) - 1
FP29_MOD = [(FP >> (W29 * i)) & M29 for i in range(L29 - 1)] + [FP >> (W29 * (L29 - 1))]
FP29_NINV = (-pow(FP, -1, 1 << W29)) % (1 << W29)
WEAK = (1 << 29) + 7          # a weakly normalised limb (ff.cuh: one carry pass over limbs < 2^32)
LAZY = 1 << 30                # a limb of K p - a without a carry pass (fe_neg_lazy)
MAX_OPERANDS = 30             # per asm statement, accumulators included


def terms_mul(x, y):
    """Partial products of column k of x * y, as (left, right) operand names."""
    def col(k):
        return [("%s[%d]" % (x, i), "%s[%d]" % (y, k - i)) for i in range(max(0, k - L29 + 1), min(k, L29 - 1) + 1)]
    return col


def terms_sqr(x, d):
    """Column k of x^2: the off-diagonal products once, against the doubled operand d."""
    def col(k):
        t = [("%s[%d]" % (x, i), "%s[%d]" % (d, k - i)) for i in range(max(0, k - L29 + 1), L29) if 2 * i < k]
        if k % 2 == 0:
            t.append(("%s[%d]" % (x, k // 2), "%s[%d]" % (x, k // 2)))
        return t
    return col


# A form = the chains that run side by side.  A chain is (output, [products]): the Montgomery reduction of the SUM of its products (one for a
# product or a square, two for the fused double product); a product is ("mul", x, y) or ("sqr", x) over operand names.
FORMS = {
    "fp_mul_pair_limbs": dict(
        args="uint32_t* r0, const uint32_t* a0, const uint32_t* b0, uint32_t* r1, const uint32_t* a1, const uint32_t* b1",
        chains=[("r0", [("mul", "a0", "b0")]), ("r1", [("mul", "a1", "b1")])],
        limb_max={"a0": WEAK, "b0": WEAK, "a1": WEAK, "b1": WEAK}),
    "fp_sqr_pair_limbs": dict(
        args="uint32_t* r0, const uint32_t* a0, uint32_t* r1, const uint32_t* a1",
        chains=[("r0", [("sqr", "a0")]), ("r1", [("sqr", "a1")])],
        limb_max={"a0": WEAK, "a1": WEAK}),
    # (x1 y1 + x2 y2) / R beside two plain products: the end of a mixed addition (Y3 | ZZ PP | ZZZ PPP).  x2 may be a lazy negation (fe_neg_lazy).
    "fp_mul2_mul_pair_limbs": dict(
        args="uint32_t* r0, const uint32_t* x1, const uint32_t* y1, const uint32_t* x2, const uint32_t* y2, "
             "uint32_t* r1, const uint32_t* a1, const uint32_t* b1, uint32_t* r2, const uint32_t* a2, const uint32_t* b2",
        chains=[("r0", [("mul", "x1", "y1"), ("mul", "x2", "y2")]), ("r1", [("mul", "a1", "b1")]), ("r2", [("mul", "a2", "b2")])],
        limb_max={"x1": WEAK, "y1": WEAK, "x2": LAZY, "y2": WEAK, "a1": WEAK, "b1": WEAK, "a2": WEAK, "b2": WEAK}),
}


def chain_operands(chain):
    return [n for pr in chain[1] for n in pr[1:]]


def column_terms(pr, k):
    return terms_mul(pr[1], pr[2])(k) if pr[0] == "mul" else terms_sqr(pr[1], "d_" + pr[1])(k)


def schedule(form):
    """The straight-line program of a form: ('mads', [(chain, left, right), ...]) with the chains alternating,
    ('digit', chain, k) (quotient digit of column k, its product with p[0], the shift) and ('out', chain, k)."""
    chains = FORMS[form]["chains"]
    prog = []
    for k in range(2 * L29 - 1):
        per = []
        for c, (_, prods) in enumerate(chains):
            t = [x for pr in prods for x in column_terms(pr, k)]
            t += [("m%d[%d]" % (c, i), "P%d" % (k - i)) for i in range(max(0, k - L29 + 1), min(k, L29))]
            per.append([(c, l, r) for l, r in t])
        inter = []
        for j in range(max(len(x) for x in per)):
            for x in per:
                if j < len(x):
                    inter.append(x[j])
        prog.append(("mads", inter))
        for c in range(len(chains)):
            prog.append(("digit", c, k) if k < L29 else ("out", c, k - L29))
    return prog


def squared_operands(form):
    return [pr[1] for ch in FORMS[form]["chains"] for pr in ch[1] if pr[0] == "sqr"]


def statements(mads, nch):
    """Cut one column's multiply-adds into asm statements of at most MAX_OPERANDS distinct operands."""
    out, cur, ops = [], [], []
    for c, l, r in mads:
        need = [x for x in (l, r) if x not in ops]
        if nch + len(ops) + len(set(need)) > MAX_OPERANDS:
            out.append((cur, ops))
            cur, ops = [], []
            need = [l, r]
        for x in need:
            if x not in ops:
                ops.append(x)
        cur.append((c, l, r))
    if cur:
        out.append((cur, ops))
    return out


def emit_form(form):
    f = FORMS[form]
    nch = len(f["chains"])
    o = ["FF_INLINE void %s(%s) {" % (form, f["args"])]
    o.append("    uint64_t " + ", ".join("c%d" % c for c in range(nch)) + ";")
    o.append("    uint32_t " + ", ".join("m%d[%d], t%d[%d]" % (c, L29, c, L29) for c in range(nch)) + ";")
    for a in squared_operands(form):
        o.append("    uint32_t d_%s[%d];" % (a, L29))
        o.append("    _Pragma(\"unroll\") for (int i = 0; i < %d; i++) d_%s[i] = %s[i] << 1;" % (L29, a, a))
    fresh = [True] * nch
    for step in schedule(form):
        if step[0] == "mads":
            for cur, ops in statements(step[1], nch):
                used = sorted(set(c for c, _, _ in cur))          # the accumulators are operands 0 .. len(used) - 1
                first = fresh[used[0]]
                assert all(fresh[c] == first for c in used)
                lines = []
                for c, l, r in cur:
                    li, ri = len(used) + ops.index(l), len(used) + ops.index(r)
                    lines.append("v_mad_u64_u32 %%%d, vcc, %%%d, %%%d, %s" % (used.index(c), li, ri, "0" if fresh[c] else "%%%d" % used.index(c)))
                    fresh[c] = False
                outs = ", ".join(('"=&v"(c%d)' if first else '"+v"(c%d)') % c for c in used)
                ins = ", ".join('"s"(0x%08xu)' % FP29_MOD[int(x[1:])] if x[0] == "P" else '"v"(%s)' % x for x in ops)
                o.append('    asm("%s" : %s : %s : "vcc");' % ("\\n\\t".join(lines), outs, ins))
        elif step[0] == "digit":
            _, c, k = step
            o.append("    m%d[%d] = ((uint32_t)c%d * 0x%08xu) & 0x%08xu; c%d += (uint64_t)m%d[%d] * 0x%08xu; c%d >>= %d;"
                     % (c, k, c, FP29_NINV, M29, c, c, k, FP29_MOD[0], c, W29))
        else:
            _, c, j = step
            if j < L29 - 2:
                o.append("    t%d[%d] = (uint32_t)c%d & 0x%08xu; c%d >>= %d;" % (c, j, c, M29, c, W29))
            else:
                o.append("    t%d[%d] = (uint32_t)c%d & 0x%08xu; t%d[%d] = (uint32_t)(c%d >> %d);" % (c, j, c, M29, c, j + 1, c, W29))
    for c, (r, _) in enumerate(f["chains"]):
        o.append("    _Pragma(\"unroll\") for (int i = 0; i < %d; i++) %s[i] = t%d[i];" % (L29, r, c))
    o.append("}")
    return "\n".join(o)


# ---------------------------------------------------------------------- integer model of the schedules
def model_run(form, vals):
    """Replays schedule(form) on Python integers.  vals: operand name -> 14 limbs.  Returns the output limbs per chain
    and the largest value any accumulator held; asserts the 64-bit and 32-bit ranges on the way."""
    f = FORMS[form]
    nch = len(f["chains"])
    env = dict(vals)
    for a in squared_operands(form):
        env["d_" + a] = [x << 1 for x in env[a]]
        assert all(x < 1 << 32 for x in env["d_" + a])
    for c in range(nch):
        env["m%d" % c] = [None] * L29
    acc, peak, out = [0] * nch, 0, [[0] * L29 for _ in range(nch)]

    def get(name):
        if name[0] == "P":
            return FP29_MOD[int(name[1:])]
        arr, i = name[:-1].split("[")
        return env[arr][int(i)]
    for step in schedule(form):
        if step[0] == "mads":
            for c, l, r in step[1]:
                x, y = get(l), get(r)
                assert x < 1 << 32 and y < 1 << 32
                acc[c] += x * y
                peak = max(peak, acc[c])
        elif step[0] == "digit":
            _, c, k = step
            m = ((acc[c] & 0xFFFFFFFF) * FP29_NINV) & M29
            env["m%d" % c][k] = m
            acc[c] += m * FP29_MOD[0]
            peak = max(peak, acc[c])
            assert acc[c] & M29 == 0
            acc[c] >>= W29
        else:
            _, c, j = step
            out[c][j] = acc[c] & M29
            if j == L29 - 2:
                out[c][j + 1] = acc[c] >> W29
                assert out[c][j + 1] < 1 << 32
            acc[c] >>= W29
        assert peak < 1 << 64, (form, step[:1], "a column accumulator reaches 2^64")
    return out, peak


def limbs_value(l):
    return sum(x << (W29 * i) for i, x in enumerate(l))


def model_expected(form, vals):
    """The value each chain must return: the sum of its products / 2^406 mod p (as a residue)."""
    rinv = pow(1 << (W29 * L29), -1, FP)
    v = {k: limbs_value(x) for k, x in vals.items()}
    return [sum(v[pr[1]] * v[pr[-1]] for pr in ch[1]) * rinv % FP for ch in FORMS[form]["chains"]]


def model_cases(form, samples=0, seed=0x29):
    """The operand sets a form is checked on: every operand at its admitted maximum; all zero; for each chain, that chain all-maximum beside the
    others all-zero and the reverse (nothing may leak between chains); then `samples` sets of random limbs.  The first case is the all-maximum one."""
    import random
    rnd = random.Random(seed)
    f = FORMS[form]
    names = list(f["limb_max"])
    top = {n: [f["limb_max"][n]] * L29 for n in names}
    zero = {n: [0] * L29 for n in names}
    cases = [top, zero]
    if len(f["chains"]) > 1:
        for ch in f["chains"]:
            mine = chain_operands(ch)
            cases.append({n: (top if n in mine else zero)[n] for n in names})
            cases.append({n: (zero if n in mine else top)[n] for n in names})
    for _ in range(samples):
        cases.append({n: [rnd.randrange(f["limb_max"][n] + 1) for _ in range(L29)] for n in names})
    return cases


def model_check(samples=64, seed=0x29):
    """Every form on model_cases: the residues are right, the output limbs exact, no accumulator reaches 2^64 (model_run asserts it step by step).
    Returns {form: log2 of the largest accumulator seen}."""
    import math
    report = {}
    for form in FORMS:
        cases = model_cases(form, samples, seed)
        peak = 0
        for vals in cases:
            out, pk = model_run(form, vals)
            peak = max(peak, pk)
            for o, e in zip(out, model_expected(form, vals)):
                assert limbs_value(o) % FP == e, (form, "wrong residue")
                assert all(x <= M29 for x in o[:-1]), (form, "output limb not exact")
        # the admitted maximum is the worst case of every accumulator (all terms are products of non-negative limbs):
        assert peak == model_run(form, cases[0])[1]
        report[form] = math.log2(peak)
    return report


def gen_fp_pair():
    o = ["// GENERATED by scripts/gen_mont_mul.py -- do not edit.",
         "// Paired Montgomery products of Fp (14 x 29-bit limbs, R = 2^406): two or three independent products side by side, every column of each",
         "// ONE v_mad_u64_u32 chain seeded with the shifted carry, the products' multiply-adds alternating.  Results are those of fp_mul_limbs /",
         "// fp_sqr_limbs / fp_mul2_limbs (ff.cuh) bit for bit; outputs may alias inputs.  Column bounds: the generator's integer model.",
         "#pragma once", "#include <stdint.h>", "", "namespace zk {", ""]
    for form in FORMS:
        o.append(emit_form(form))
        o.append("")
    o.append("}  // namespace zk")
    return "\n".join(o) + "\n"


# ====================================================================== Fp2 on ONE lane: lazy Karatsuba, column-interleaved
# (a0 + a1 u)(b0 + b1 u), u^2 = -1, as three base multiplications feeding TWO running Montgomery reductions.  Column k forms
#     T0 = sum a0_i b0_j        T1 = sum a1_i b1_j        t2 = sum (a0 + a1)_i (b0 + b1)_j          (i + j = k)
# T0 and T1 each in an accumulator of their own starting at zero, t2 on top of the c1 chain's shifted carry; then
#     c0 += T0 - T1             c1 -= T0 + T1
# BEFORE the quotient digits' m p terms go on top (t2 alone is 14 * 2^60: with the m p terms it would pass 2^64), and the two chains reduce like two
# plain products.  No unreduced double-width product is kept.
#   * The sums a0 + a1, b0 + b1 are taken limb by limb WITHOUT a carry pass (limbs <= 2^30 + 14), so t2 - T0 - T1 is the exact column of
#     a0 b1 + a1 b0 and the c1 chain never goes negative.
#   * The c0 chain can: its accumulator is SIGNED (two's complement; v_mad_u64_u32 adds modulo 2^64, the shift is arithmetic).  The high columns
#     add the limbs of p, that is p R to the product, so the value leaves as c0 + p, non-negative with exact limbs: c0 + p < 3p, c1 < 2p for operand
#     bounds 2 A B <= 2^25 (ff.cuh: fe_mul2_lanewise).
# The schedule (fp2_schedule) is one list of steps that the emitter and the integer model both consume, as for the paired forms above.
FP2_FORM = "fp2_mul_lane_limbs"
FP2_OPERANDS = ("a0", "a1", "b0", "b1")
FP2_SUM = 2 * WEAK            # a limb of a0 + a1 (no carry pass)


def fp2_schedule():
    """('mads', [(acc, left, right), ...]): T0, T1 (fresh every column) and C1 (seeded with its carry) alternating, then after ('comb',) the m p terms
    of C0 and C1 alternating; ('digit', chain, k) / ('out', chain, j) as in schedule(); ('addp', j): the c0 chain takes limb j of p; ('addtop',): its top limb."""
    prog = []
    for k in range(2 * L29 - 1):
        idx = range(max(0, k - L29 + 1), min(k, L29 - 1) + 1)
        inter = []
        for i in idx:
            inter += [("T0", "a0[%d]" % i, "b0[%d]" % (k - i)), ("T1", "a1[%d]" % i, "b1[%d]" % (k - i)), ("C1", "sa[%d]" % i, "sb[%d]" % (k - i))]
        prog.append(("mads", inter))
        prog.append(("comb",))
        inter = []
        for i in range(max(0, k - L29 + 1), min(k, L29)):
            inter += [("C0", "m0[%d]" % i, "P%d" % (k - i)), ("C1", "m1[%d]" % i, "P%d" % (k - i))]
        if inter:
            prog.append(("mads", inter))
        if k >= L29:
            prog.append(("addp", k - L29))
        for c in range(2):
            prog.append(("digit", c, k) if k < L29 else ("out", c, k - L29))
    prog.append(("addtop",))          # the top limb of p goes straight onto the top limb of c0: there is no column 27
    return prog


def emit_fp2():
    accs = ("C0", "C1", "T0", "T1")
    o = ["FF_INLINE void %s(uint32_t* r0, uint32_t* r1, const uint32_t* a0, const uint32_t* a1, const uint32_t* b0, const uint32_t* b1) {" % FP2_FORM]
    o.append("    int64_t C0 = 0;")
    o.append("    uint64_t C1 = 0, T0, T1;")
    o.append("    uint32_t sa[%d], sb[%d], m0[%d], m1[%d], t0[%d], t1[%d];" % ((L29,) * 6))
    o.append("    _Pragma(\"unroll\") for (int i = 0; i < %d; i++) { sa[i] = a0[i] + a1[i]; sb[i] = b0[i] + b1[i]; }" % L29)
    for step in fp2_schedule():
        if step[0] == "mads":
            fresh = {"T0": True, "T1": True, "C0": False, "C1": False}
            for cur, ops in statements(step[1], 3):
                used = [a for a in accs if any(c == a for c, _, _ in cur)]
                cons = ", ".join(('"=&v"(%s)' if fresh[a] else '"+v"(%s)') % a for a in used)
                lines = []
                for c, l, r in cur:
                    li, ri = len(used) + ops.index(l), len(used) + ops.index(r)
                    lines.append("v_mad_u64_u32 %%%d, vcc, %%%d, %%%d, %s" % (used.index(c), li, ri, "0" if fresh[c] else "%%%d" % used.index(c)))
                    fresh[c] = False
                ins = ", ".join('"s"(0x%08xu)' % FP29_MOD[int(x[1:])] if x[0] == "P" else '"v"(%s)' % x for x in ops)
                o.append('    asm("%s" : %s : %s : "vcc");' % ("\\n\\t".join(lines), cons, ins))
        elif step[0] == "comb":
            o.append("    C0 += (int64_t)(T0 - T1); C1 -= T0 + T1;")
        elif step[0] == "addp":
            o.append("    C0 += 0x%08x;" % FP29_MOD[step[1]])
        elif step[0] == "addtop":
            o.append("    t0[%d] += 0x%08xu;" % (L29 - 1, FP29_MOD[L29 - 1]))
        elif step[0] == "digit":
            _, c, k = step
            o.append("    m%d[%d] = ((uint32_t)C%d * 0x%08xu) & 0x%08xu; C%d += (uint64_t)m%d[%d] * 0x%08xu; C%d >>= %d;"
                     % (c, k, c, FP29_NINV, M29, c, c, k, FP29_MOD[0], c, W29))
        else:
            _, c, j = step
            if j < L29 - 2:
                o.append("    t%d[%d] = (uint32_t)C%d & 0x%08xu; C%d >>= %d;" % (c, j, c, M29, c, W29))
            else:
                o.append("    t%d[%d] = (uint32_t)C%d & 0x%08xu; t%d[%d] = (uint32_t)(C%d >> %d);" % (c, j, c, M29, c, j + 1, c, W29))
    o.append("    _Pragma(\"unroll\") for (int i = 0; i < %d; i++) { r0[i] = t0[i]; r1[i] = t1[i]; }" % L29)
    o.append("}")
    return "\n".join(o)


def fp2_model_run(vals):
    """Replays fp2_schedule() on Python integers.  vals: a0, a1, b0, b1 -> 14 limbs.  Returns (c0 limbs, c1 limbs) and the ranges seen:
    the largest unsigned accumulator (T0, T1, C1) and the smallest / largest value of the signed one (C0).  Asserts the 64-bit ranges at every step."""
    env = dict(vals)
    env["sa"] = [x + y for x, y in zip(vals["a0"], vals["a1"])]
    env["sb"] = [x + y for x, y in zip(vals["b0"], vals["b1"])]
    assert all(x < 1 << 32 for x in env["sa"] + env["sb"])
    env["m0"], env["m1"] = [None] * L29, [None] * L29
    acc = {"C0": 0, "C1": 0, "T0": 0, "T1": 0}
    out = [[0] * L29, [0] * L29]
    upeak, slo, shi = 0, 0, 0

    def get(name):
        if name[0] == "P":
            return FP29_MOD[int(name[1:])]
        arr, i = name[:-1].split("[")
        return env[arr][int(i)]
    for step in fp2_schedule():
        if step[0] == "mads":
            fresh = {"T0": True, "T1": True}
            for c, l, r in step[1]:
                x, y = get(l), get(r)
                assert x < 1 << 32 and y < 1 << 32
                if fresh.get(c):
                    acc[c], fresh[c] = 0, False
                acc[c] += x * y
        elif step[0] == "comb":
            acc["C0"] += acc["T0"] - acc["T1"]
            acc["C1"] -= acc["T0"] + acc["T1"]
        elif step[0] == "addp":
            acc["C0"] += FP29_MOD[step[1]]
        elif step[0] == "addtop":
            out[0][L29 - 1] += FP29_MOD[L29 - 1]
        elif step[0] == "digit":
            _, c, k = step
            a = "C%d" % c
            m = (((acc[a] & 0xFFFFFFFF) * FP29_NINV) & 0xFFFFFFFF) & M29
            env["m%d" % c][k] = m
            acc[a] += m * FP29_MOD[0]
            assert acc[a] & M29 == 0
            acc[a] >>= W29          # Python's shift of a negative integer is arithmetic
        else:
            _, c, j = step
            a = "C%d" % c
            out[c][j] = acc[a] & M29
            acc[a] >>= W29
            if j == L29 - 2:
                assert -(1 << 31) <= acc[a] < 1 << 31          # the top limb; negative only where c0 + p is (operand bounds beyond the contract)
                out[c][j + 1] = acc[a]
        upeak = max(upeak, acc["C1"], acc["T0"], acc["T1"])
        slo, shi = min(slo, acc["C0"]), max(shi, acc["C0"])
        assert acc["C1"] >= 0 and upeak < 1 << 64, "an unsigned accumulator leaves [0, 2^64)"
        assert -(1 << 63) <= slo and shi < 1 << 63, "the signed accumulator leaves [-2^63, 2^63)"
    return out, (upeak, slo, shi)


def fp2_model_expected(vals):
    """(c0 + p, c1) of the Montgomery product, as integers: exact values, not residues (the reductions are deterministic)."""
    rinv = pow(1 << (W29 * L29), -1, FP)
    a0, a1, b0, b1 = (limbs_value(vals[n]) for n in FP2_OPERANDS)
    return [(a0 * b0 - a1 * b1) * rinv % FP, (a0 * b1 + a1 * b0) * rinv % FP]


def fp2_extreme(bound):
    """The largest weakly normalised operand below bound * p: limbs 0..12 at 2^29 + 7, the top limb as large as the bound lets it be."""
    low = sum(WEAK << (W29 * i) for i in range(L29 - 1))
    return [WEAK] * (L29 - 1) + [(bound * FP - 1 - low) >> (W29 * (L29 - 1))]


def fp2_model_cases(bound, samples=0, seed=0x2F2):
    """The sixteen corner patterns of {extreme, zero} per operand, all-extreme first (a1 b1 extreme beside a0 b0 = 0 is the most negative c0 chain, the
    reverse the most positive); then `samples` sets of random weakly normalised limbs below bound * p."""
    import random
    rnd = random.Random(seed)
    top, zero = fp2_extreme(bound), [0] * L29
    cases = [dict(zip(FP2_OPERANDS, (top if (bits >> i) & 1 else zero for i in range(4)))) for bits in (15,) + tuple(range(15))]
    for _ in range(samples):
        cases.append({n: [rnd.randrange(WEAK + 1) for _ in range(L29 - 1)] + [rnd.randrange(top[-1] + 1)] for n in FP2_OPERANDS})
    return cases


FP2_REST = 64                 # ff.cuh: FP_REST, the bound of values at rest
FP2_TYPE_MAX = 8192           # ff.cuh: FP_MAX_BOUND, the largest bound a register value's type can state


def fp2_model_check(samples=64, seed=0x2F2):
    """The one-lane Fp2 product: (1) at the largest limbs ANY typed operand can have (bound 8192 p, beyond the product's contract) every accumulator stays
    inside its 64-bit range and the residues are right; (2) at the at-rest bound 64 p, and at 4096 p x 4096 p = the contract's limit 2 A B <= 2^25,
    the outputs are moreover non-negative with exact limbs, c0 + p < 3p and c1 < 2p.
    Returns (log2 of the largest unsigned accumulator, log2 of the largest magnitude of the signed one)."""
    import math
    upeak, smag = 0, 0
    for bound, contract in ((FP2_TYPE_MAX, False), (FP2_REST, True), (4096, True)):
        for vals in fp2_model_cases(bound, samples, seed):
            out, (u, lo, hi) = fp2_model_run(vals)
            upeak, smag = max(upeak, u), max(smag, -lo, hi)
            for o, e in zip(out, fp2_model_expected(vals)):
                assert limbs_value(o) % FP == e, (FP2_FORM, "wrong residue")
                assert all(0 <= x <= M29 for x in o[:-1]), (FP2_FORM, "output limb not exact")
            if contract:
                assert 0 <= limbs_value(out[0]) < 3 * FP and 0 <= limbs_value(out[1]) < 2 * FP and out[0][-1] >= 0 and out[1][-1] >= 0
    return math.log2(upeak), math.log2(smag)


def fp2_output_bounds(A, B):
    """Operand values below A p and B p: (c0 + p, c1) lie below these multiples of p.  c0 = (a0 b0 - a1 b1 + m p) / R with m < R, so
    -A B p^2 / R < c0 < A B p^2 / R + p; c1 = (a0 b1 + a1 b0 + m p) / R < 2 A B p^2 / R + p."""
    from fractions import Fraction
    x = Fraction(A * B * FP, 1 << (W29 * L29))
    assert x < 1, "c0 + p could be negative"
    return 2 + x, 1 + 2 * x


def gen_fp2_lane():
    o = ["// GENERATED by scripts/gen_mont_mul.py -- do not edit.",
         "// Montgomery product of Fp2 = Fp[u] / (u^2 + 1) on ONE lane (Fp: 14 x 29-bit limbs, R = 2^406): lazy Karatsuba, three base multiplications",
         "// (a0 b0, a1 b1, (a0 + a1)(b0 + b1)) feeding two running reductions column by column, 5 x 196 multiply-adds.  r0 = c0 + p < 3p, r1 = c1 < 2p,",
         "// exact limbs; the c0 accumulator is signed.  Outputs may alias inputs.  Ranges: the generator's integer model (fp2_model_check).",
         "#pragma once", "#include <stdint.h>", "", "namespace zk {", "", emit_fp2(), "", "}  // namespace zk"]
    return "\n".join(o) + "\n"


def gen_fr_header():
    # the base field Fp no longer uses this scheme: radix 2^29, carry-free columns (ff.cuh, gen_fp29_consts.py)
    return ("// GENERATED by scripts/gen_mont_mul.py -- do not edit.\n#pragma once\n#include <stdint.h>\n\nnamespace zk {\n\n"
            + gen("fr", 8, FR, (-pow(FR, -1, 1 << 32)) % (1 << 32)) + "\n\n}  // namespace zk\n")


def main():
    for form, bits in model_check().items():
        print("model: %s holds, largest column accumulator 2^%.3f" % (form, bits))
    print("model: %s holds, largest unsigned accumulator 2^%.3f, signed accumulator within +-2^%.3f" % ((FP2_FORM,) + fp2_model_check()))
    if "--check" in sys.argv[1:]:
        return
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "zukelang_amd", "csrc", "ff_mul_gen.cuh")
    with open(path, "w") as f:
        f.write(gen_fr_header())
    print("wrote", path)
    path = os.path.join(root, "zukelang_amd", "csrc", "fp_pair_gen.cuh")
    with open(path, "w") as f:
        f.write(gen_fp_pair())
    print("wrote", path)
    path = os.path.join(root, "zukelang_amd", "csrc", "fp2_lane_gen.cuh")
    with open(path, "w") as f:
        f.write(gen_fp2_lane())
    print("wrote", path)


if __name__ == "__main__":
    main()
