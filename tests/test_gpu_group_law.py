"""Every form of the device's group law against oracle/pyref.py, byte for byte (zk_selftest_group, include/zkmi355x.h).

The library holds "add two points" in nine near-copies -- XYZZ on one lane, on lane pairs, on four slots, with the second operand affine, in LDS, in
device memory; Jacobian for the key derivation -- built with different flags in different translation units.  Each has its own branches for an
identity operand, P + P and P + (-P), and finds "equal x" with a zero test on a lazily reduced difference.  tests/group_law_cases.py builds the
operands; here every row of its form table runs every class it can take by contract, with the coordinates canonical (rep 0) and lifted to the
largest multiple of p their types admit (rep 1), in one call per (group, form, rep).  No tolerances.

The y = 0 branch of the doublings is unreachable on these curves: a point with y = 0 has order two, and both cofactors are odd, so neither
y^2 = x^3 + 4 nor its twist has one over the field the library works in -- no on-curve operand reaches it, and off-curve points are not fed."""
import ctypes as C
from collections import Counter
from functools import lru_cache

import pytest

import group_law_cases as GL
from oracle import pyref as P
from zukelang_amd import _lib

pytestmark = pytest.mark.gpu

GROUPS = (0, 1)
# (group, form) of every addition; the parked form is built for lane pairs only, so it has no G1 row (the hook refuses it: tests/test_group_law_surface.py)
PAIR_FORMS = [(g, n) for g in GROUPS for n, f in GL.FORMS.items() if f.second in ("xyzz", "affine", "table") and not (f.g2_only and g == 0)]
DBL_FORMS = [n for n, f in GL.FORMS.items() if f.second is None]
CLASSES = {"generic", "P+P", "P-P", "O+P", "P+O", "O+O", "equal y"}


def selftest(group, form, rep, a, b, n):
    out = C.create_string_buffer((192 if group else 96) * n)
    u8 = lambda x: None if x is None else C.cast(C.c_char_p(x), _lib._P8)
    _lib.check(_lib.lib().zk_selftest_group(group, GL.FORMS[form].number, rep, u8(a), u8(b), n, C.cast(out, _lib._P8)))
    size = 192 if group else 96
    return [out.raw[size * i:size * (i + 1)] for i in range(n)]


battery = lru_cache(maxsize=None)(GL.battery)
doublings = lru_cache(maxsize=None)(GL.doublings)
scalar_battery = lru_cache(maxsize=None)(GL.scalar_battery)


def takes(form, pair):
    """the classes a form takes by its contract (tests/group_law_cases.py: FORMS)"""
    f = GL.FORMS[form]
    if f.second == "table" and pair.b_aff is None:
        return False
    if f.needs_affine_a and pair.a_rep not in ("one",) + GL.IDENTITIES:
        return False
    return True


def run_pairs(group, form, rep, g, pairs):
    f = GL.FORMS[form]
    a = b"".join(g.xyzz_bytes(x.a) for x in pairs)
    b = b"".join(g.xyzz_bytes(x.b_xyzz) if f.second == "xyzz" else g.aff_bytes(x.b_aff) for x in pairs)
    got = selftest(group, form, rep, a, b, len(pairs))
    bad = [(i, x.cls, x.a_rep, x.b_rep) for i, (x, y) in enumerate(zip(pairs, got)) if y != x.expected]
    assert not bad, "%s, group %d, rep %d: %d of %d differ from the oracle, first %s" % (form, group, rep, len(bad), len(pairs), bad[:8])


@pytest.mark.parametrize("rep", (0, 1))
@pytest.mark.parametrize("group,form", PAIR_FORMS)
def test_additions_match_the_oracle_in_every_class_and_representation(group, form, rep):
    f = GL.FORMS[form]
    g, pairs, counts = battery(group)
    assert set(counts) == CLASSES and len(pairs) >= 1900
    mine = [x for x in pairs if takes(form, x)]
    seen = Counter((x.cls, x.a_rep, x.b_rep) for x in mine)
    want_classes = CLASSES - ({"P+O", "O+O"} if f.second == "table" else set())
    assert {c for c, _, _ in seen} == want_classes, (form, set(c for c, _, _ in seen))
    a_reps = ("one",) if f.needs_affine_a else GL.REPRS
    b_reps = GL.REPRS if f.second == "xyzz" else ("one",)          # an affine q is the point itself: the three representations of b collapse
    for cls in want_classes:
        for ra in (GL.IDENTITIES if cls in ("O+P", "O+O") else a_reps):
            for rb in (GL.IDENTITIES if cls in ("P+O", "O+O") else b_reps):
                assert seen[(cls, ra, rb)] >= 2, (form, cls, ra, rb)
    run_pairs(group, form, rep, g, mine)


@pytest.mark.parametrize("rep", (0, 1))
@pytest.mark.parametrize("form", DBL_FORMS)
@pytest.mark.parametrize("group", GROUPS)
def test_doublings_match_the_oracle(group, form, rep):
    g, cases = doublings(group)
    if GL.FORMS[form].needs_affine_a:
        cases = [c for c in cases if c[1] in ("one",) + GL.IDENTITIES]
    seen = Counter((c[0], c[1]) for c in cases)
    for r in (("one",) if GL.FORMS[form].needs_affine_a else GL.REPRS):
        assert seen[("P", r)] >= 20
    for r in GL.IDENTITIES:
        assert seen[("O", r)] >= 4
    got = selftest(group, form, rep, b"".join(g.xyzz_bytes(c[2]) for c in cases), None, len(cases))
    bad = [(i, c[0], c[1]) for i, (c, y) in enumerate(zip(cases, got)) if y != c[3]]
    assert not bad, (form, group, rep, bad[:8])


@pytest.mark.parametrize("rep", (0, 1))
@pytest.mark.parametrize("group", GROUPS)
def test_slot_groups_of_one_wave_take_different_branches(group, rep):
    """xyzz_add_slots makes every predicate GROUP-uniform by fetching it from the slot that owns it: consecutive groups of a wave (16 in G1, 8 in G2)
    alternate generic / doubling / cancelling / identity cases, so a predicate that leaked across groups would send a neighbour down the wrong branch"""
    g, pairs, _ = battery(group)
    lanes = {k: [x for x in pairs if x.cls in v] for k, v in
             {"generic": ("generic", "equal y"), "doubling": ("P+P",), "cancelling": ("P-P",), "identity": ("O+P", "P+O", "O+O")}.items()}
    n = min(len(v) for v in lanes.values())
    assert n >= 90
    order = [lanes[k][i] for i in range(n) for k in ("generic", "doubling", "cancelling", "identity")]
    per_wave = 64 // (8 if group else 4)
    for w in range(0, len(order) - per_wave + 1, per_wave):
        kinds = [x.cls for x in order[w:w + per_wave]]
        assert all(kinds[i] != kinds[i + 1] for i in range(per_wave - 1)) and len(set(kinds)) >= 4
    run_pairs(group, "add_slots", rep, g, order)


@pytest.mark.parametrize("rep", (0, 1))
@pytest.mark.parametrize("group", GROUPS)
def test_scalar_multiplication_at_the_edges_of_its_split_and_recoding(group, rep):
    """xyzz_mul_scalar_endo against pt_mul: small scalars and recoding edges, scalars near r, the GLV (G1) / GLS (G2) edges that
    tests/group_law_cases.py: named_scalars asserts from its restatement of the split, and random scalars on top"""
    randoms = 24 if group == 0 else 16
    g, cases = scalar_battery(group, randoms)
    names = Counter(c[0] for c in cases)
    for name in GL.named_scalars(group):
        assert names[name] == 3, name                       # every named scalar, on the point's three representations
    assert sum(1 for n in names if n.startswith("random")) >= randoms and names["identity"] == 2
    for k in GL.SMALL + GL.NEAR_R:
        assert any(c[3] == k for c in cases), hex(k)
    got = selftest(group, "mul", rep, b"".join(g.xyzz_bytes(c[2]) for c in cases), b"".join(P.fr_to_bytes(c[3]) for c in cases), len(cases))
    bad = [(c[0], c[1]) for c, y in zip(cases, got) if y != c[4]]
    assert not bad, (group, rep, bad[:8])
