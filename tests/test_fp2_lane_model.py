"""The one-lane Fp2 product of the G2 bucket accumulation (scripts/gen_mont_mul.py: fp2_mul_lane_limbs), without a GPU: the generator's integer model
replays the emitted schedule -- the same list of steps the emitter prints -- on Python integers at the extreme limbs, and the committed header is what
the generator writes.

Lazy Karatsuba, column by column: T0 = a0 b0 and T1 = a1 b1 in accumulators of their own, (a0 + a1)(b0 + b1) on top of the c1 chain's carry, then
c0 += T0 - T1 and c1 -= T0 + T1 before the quotient digits' multiples of p.  What can go wrong: an accumulator leaving 64 bits (the Karatsuba column
alone is 14 * 2^60), the SIGNED c0 chain leaving [-2^63, 2^63) or ending below zero, the c1 chain going negative, a limb of p R missing from c0 + p."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_mont_mul", os.path.join(ROOT, "scripts", "gen_mont_mul.py"))
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)

p, L, W = G.FP, G.L29, G.W29
RINV = pow(1 << (W * L), -1, p)


def test_the_schedule_is_five_times_196_multiply_adds_in_the_stated_order():
    mads = [s for s in G.fp2_schedule() if s[0] == "mads"]
    count = lambda acc, pre: sum(1 for s in mads for c, l, _ in s[1] if c == acc and l.startswith(pre))
    assert [count("T0", "a0"), count("T1", "a1"), count("C1", "sa")] == [196] * 3          # three base multiplications
    assert [count("C0", "m0"), count("C1", "m1")] == [14 * 13] * 2                           # two reductions; with the 14 digit products of p[0]: 196 each
    assert sum(len(s[1]) for s in mads) + 2 * 14 == 5 * 196
    # in every column the combination precedes the m p terms, and the three product chains alternate
    prog = G.fp2_schedule()
    for i, s in enumerate(prog):
        if s[0] == "comb":
            assert prog[i - 1][0] == "mads" and all(c in ("T0", "T1", "C1") and not l.startswith("m") for c, l, _ in prog[i - 1][1])
            assert [c for c, _, _ in prog[i - 1][1]] == ["T0", "T1", "C1"] * (len(prog[i - 1][1]) // 3)
        if s[0] == "mads" and s[1][0][1].startswith("m"):
            assert prog[i - 1][0] == "comb" and [c for c, _, _ in s[1]] == ["C0", "C1"] * (len(s[1]) // 2)
    assert sum(1 for s in prog if s[0] == "comb") == 2 * L - 1 and sum(1 for s in prog if s[0] == "addp") == L - 1 and prog[-1] == ("addtop",)


def test_every_accumulator_stays_inside_64_bits_at_the_extreme_limbs():
    """bound 8192 p: the largest limbs any typed register value can have, beyond the product's contract -- ranges and residues only"""
    top = G.fp2_extreme(G.FP2_TYPE_MAX)
    assert top[:-1] == [G.WEAK] * (L - 1) and G.limbs_value(top) < G.FP2_TYPE_MAX * p <= G.limbs_value(top) + (1 << (W * (L - 1)))
    upeak, lo, hi = 0, 0, 0
    for vals in G.fp2_model_cases(G.FP2_TYPE_MAX):
        out, (u, l, h) = G.fp2_model_run(vals)          # asserts the ranges after every step
        upeak, lo, hi = max(upeak, u), min(lo, l), max(hi, h)
        for o, e in zip(out, G.fp2_model_expected(vals)):
            assert G.limbs_value(o) % p == e and all(0 <= x < 1 << W for x in o[:-1])
    assert (1 << 63) < upeak < 1 << 64          # the Karatsuba column: 14 (2^30 + 14)^2 and a carry -- it NEEDS the unsigned range
    assert -(1 << 62) < lo < 0 < hi < 1 << 63   # the c0 chain does go negative; it keeps a bit of room on either side


def test_at_the_contracts_bounds_the_outputs_are_non_negative_and_below_3p_and_2p():
    for bound in (G.FP2_REST, 4096):          # at rest; 4096 x 4096 = 2^24: the limit 2 A B <= 2^25 of fe_mul2_lanewise
        b0, b1 = G.fp2_output_bounds(bound, bound)
        assert b0 <= 3 and b1 <= 2
        for vals in G.fp2_model_cases(bound, samples=16, seed=bound):
            out, _ = G.fp2_model_run(vals)
            a0, a1, c0, c1 = (G.limbs_value(vals[n]) for n in G.FP2_OPERANDS)
            assert max(a0, a1, c0, c1) < bound * p
            v0, v1 = G.limbs_value(out[0]), G.limbs_value(out[1])
            assert 0 <= v0 < b0 * p and 0 <= v1 < b1 * p and out[0][-1] >= 0 and out[1][-1] >= 0
            assert v0 % p == (a0 * c0 - a1 * c1) * RINV % p and v1 % p == (a0 * c1 + a1 * c0) * RINV % p
            assert all(0 <= x < 1 << W for o in out for x in o[:-1])
    worst = dict(zip(G.FP2_OPERANDS, ([0] * L, G.fp2_extreme(4096), [0] * L, G.fp2_extreme(4096))))          # c0 = -a1 b1: the most negative
    out, (_, lo, _) = G.fp2_model_run(worst)
    assert lo < 0 and 0 < G.limbs_value(out[0]) < 2 * p          # c0 + p with -a1 b1 / R < c0 < p: the quotient digits add up to R p


def test_values_one_lane_apart_do_not_mix():
    """a0 b0 = 0 beside a1 b1 extreme and the reverse, each operand alone non-zero: the sixteen corners"""
    cases = G.fp2_model_cases(G.FP2_REST)
    assert len(cases) == 16 and len({tuple(tuple(v[n]) for n in G.FP2_OPERANDS) for v in cases}) == 16
    for vals in cases + G.fp2_model_cases(G.FP2_REST, samples=48, seed=7)[16:]:
        out, _ = G.fp2_model_run(vals)
        assert [G.limbs_value(o) % p for o in out] == G.fp2_model_expected(vals)


def test_the_whole_model_check_and_the_committed_header():
    ubits, sbits = G.fp2_model_check(samples=32)
    assert 63 < ubits < 64 and sbits < 63
    text = open(os.path.join(ROOT, "zukelang_amd", "csrc", "fp2_lane_gen.cuh")).read()
    assert text == G.gen_fp2_lane()
    assert text.count("v_mad_u64_u32") == 5 * 196 - 2 * 14 and "int64_t C0" in text          # the digit products of p[0] are plain C
