"""tests/srs_model.py held to the table of tests/srs_cases.py without a GPU: the mask of every crafted string is the one WRITTEN OUT beside it, honest
strings of every length get 0, the degenerate trapdoors their bit, and the contribution is the map the header states -- on honest strings the string
of the product trapdoor, on any string a map that commutes with composition."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import specialize_model as SM
import srs_cases as S
import srs_model as M

R = S.R


@pytest.mark.parametrize("name", sorted(S.CRAFTED))
def test_the_model_gives_the_tables_mask(name):
    assert M.mask(*S.crafted(name)) == S.CRAFTED[name][1], name


def test_the_tables_masks_are_not_all_alike_and_every_bit_stands_alone_somewhere():
    masks = {m for _, m in S.CRAFTED.values()}
    for bit in (M.TAU_G1, M.TAU_G2, M.ALPHA, M.BETA):
        assert bit in masks, M.NAMES[bit]
    assert all(m for m in masks)


def test_honest_strings_of_every_length_hold():
    for n in S.HONEST_N:
        assert M.mask(*SM.honest_string(n, S.ALPHA, S.BETA, S.TAU)) == 0, n
    for lens in S.HONEST_FREE + ((S.N1, S.NAB, S.N2),):
        assert M.lengths_ok(*lens) and M.mask(*M.honest(*lens, S.ALPHA, S.BETA, S.TAU)) == 0, lens
    # the model's free-length string is the specialisation's string at a circuit's sizes
    assert M.honest(*SM.srs_sizes(5), S.ALPHA, S.BETA, S.TAU) == SM.honest_string(5, S.ALPHA, S.BETA, S.TAU)


@pytest.mark.parametrize("name", sorted(S.DEGENERATE))
def test_degenerate_trapdoors(name):
    (a, b, t), want = S.DEGENERATE[name]
    assert M.mask(*M.honest(S.N1, S.NAB, S.N2, a, b, t)) == want
    assert M.mask(*M.honest(2, 1, 2, a, b, t)) == want


def test_the_all_zero_string():
    assert M.mask([0] * 5, [0] * 3, [0] * 3, 0, [0] * 4) == M.GENERATORS | M.TRIVIAL


def test_a_relation_without_an_index_holds():
    t1, a1, b1, b2, t2 = M.honest(4, 1, 2, S.ALPHA, S.BETA, S.TAU)
    assert M.mask(t1, [12345], b1, b2, t2) == 0          # NAB = 1: alpha_tau1[0] is any non-zero alpha


def test_the_specialisations_failing_strings_are_named_by_the_string():
    assert M.mask(*SM.crafted_alpha(8, S.ALPHA, S.BETA, S.TAU)) == M.ALPHA
    assert M.mask(*SM.crafted_high_power(8, S.ALPHA, S.BETA, S.TAU)) == M.TAU_G1


def test_lengths():
    assert M.lengths_ok(2, 1, 2) and M.lengths_ok(1 << 25, 1 << 24, (1 << 24) + 2)
    for bad in ((1, 1, 2), (2, 0, 2), (2, 1, 1), (3, 4, 2), (3, 1, 4), ((1 << 25) + 1, 1, 2)):
        assert not M.lengths_ok(*bad), bad


def test_a_contributed_honest_string_is_the_string_of_the_product_trapdoor():
    am, bm, tm = S.MUL
    for lens in S.HONEST_FREE[:2] + ((S.N1, S.NAB, S.N2),):
        got = M.contributed(*M.honest(*lens, S.ALPHA, S.BETA, S.TAU), am, bm, tm)
        assert got == M.honest(*lens, S.ALPHA * am % R, S.BETA * bm % R, S.TAU * tm % R), lens
        assert M.mask(*got) == 0


def test_the_contribution_is_a_map_of_any_string():
    am, bm, tm = S.MUL
    for name, (_, want) in S.CRAFTED.items():
        s = S.crafted(name)
        assert M.contributed(*s, 1, 1, 1) == tuple([x % R for x in e] if isinstance(e, list) else e % R for e in s), name
        once = M.contributed(*s, am, bm, tm)
        assert M.contributed(*once, 3, 5, 7) == M.contributed(*s, 3 * am % R, 5 * bm % R, 7 * tm % R), name
        # a non-zero scaling of every relation's two sides: the verdict on the string does not change
        assert M.mask(*once) == want, name
    z = M.contributed(*M.honest(S.N1, S.NAB, S.N2, S.ALPHA, S.BETA, 0), am, bm, tm)
    assert z == M.honest(S.N1, S.NAB, S.N2, S.ALPHA * am % R, S.BETA * bm % R, 0)          # a tau = 0 string keeps its zeros
