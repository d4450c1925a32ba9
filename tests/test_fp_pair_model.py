"""The generator of the paired field products (scripts/gen_mont_mul.py), without a GPU: its integer model replays the schedule of every emitted form --
the same list of steps the emitter prints -- on Python integers at the extreme limb values the form admits, and the committed headers are what the
generator writes."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_mont_mul", os.path.join(ROOT, "scripts", "gen_mont_mul.py"))
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)

WEAK, LAZY = (1 << 29) + 7, 1 << 30


def test_the_forms_the_group_law_uses_are_emitted():
    assert {"fp_mul_pair_limbs", "fp_sqr_pair_limbs", "fp_mul2_mul_pair_limbs"} <= set(G.FORMS)
    for form, f in G.FORMS.items():
        fused = [ch for ch in f["chains"] if len(ch[1]) == 2]
        # weakly normalised limbs everywhere; the lazy negation's 2^30 only as the second left factor of a fused chain
        for name, mx in f["limb_max"].items():
            lazy_ok = any(ch[1][1][1] == name for ch in fused)
            assert mx == (LAZY if lazy_ok else WEAK), (form, name)


@pytest.mark.parametrize("form", sorted(G.FORMS))
def test_no_column_accumulator_reaches_2_64_at_the_extreme_limbs(form):
    cases = G.model_cases(form)          # all-maximum first, all-zero, one chain all-maximum beside the others all-zero and the reverse
    assert len(cases) == 2 + 2 * len(G.FORMS[form]["chains"])
    peaks = []
    for vals in cases:
        out, peak = G.model_run(form, vals)          # asserts < 2^64 after every step
        peaks.append(peak)
        for o, e in zip(out, G.model_expected(form, vals)):
            assert G.limbs_value(o) % G.FP == e
            assert all(x < 1 << 29 for x in o[:-1])
    assert max(peaks) == peaks[0]          # the all-maximum operands are the worst case
    fused = any(len(ch[1]) == 2 for ch in G.FORMS[form]["chains"])
    if fused:
        assert (1 << 63) < peaks[0] < 1 << 64          # 42 terms per column with one factor at 2^30: the tightest bound, 2^63.5
    else:
        assert peaks[0] < 1 << 63                       # 28 terms of weakly normalised limbs: 2^62.05


def test_the_fused_chain_has_42_terms_per_column_and_a_plain_product_28():
    for form, f in G.FORMS.items():
        for c, ch in enumerate(f["chains"]):
            if any(pr[0] == "sqr" for pr in ch[1]):
                continue          # a square takes its off-diagonal products once
            longest = max(sum(1 for cc, _, _ in step[1] if cc == c) for step in G.schedule(form) if step[0] == "mads")
            assert longest + 1 == (42 if len(ch[1]) == 2 else 28), (form, c)          # + the quotient digit's own product


def test_every_chain_is_one_chain_and_the_chains_alternate():
    for form, f in G.FORMS.items():
        n = len(f["chains"])
        for step in G.schedule(form):
            if step[0] != "mads":
                continue
            order = [c for c, _, _ in step[1]]
            if n > 1:
                shortest = min(order.count(c) for c in range(n))
                assert order[:n * shortest] == list(range(n)) * shortest, form          # strictly alternating while every chain has terms left


def test_random_operands_and_the_whole_model_check():
    report = G.model_check(samples=32)
    assert set(report) == set(G.FORMS) and all(bits < 64 for bits in report.values())


def test_the_committed_headers_are_what_the_generator_writes():
    csrc = os.path.join(ROOT, "zukelang_amd", "csrc")
    assert open(os.path.join(csrc, "fp_pair_gen.cuh")).read() == G.gen_fp_pair()
    fr = open(os.path.join(csrc, "ff_mul_gen.cuh")).read()
    assert fr == G.gen_fr_header()
    for text in (fr, G.gen_fp_pair()):
        assert "v_mad_u64_u32" in text
