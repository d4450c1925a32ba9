"""The ends of the MSM window plan on the device, at every width: scalars whose signed digits sit at the top value +2^(c-1) (the top bucket, weight nbw,
the lone member of the last high-digit value of csrc/msm_tail.cuh: digit_plan), at the bottom value -(2^(c-1) - 1), carry out of it, stand alone in
the last window or straddle r / 2 where folded digits change sign -- the scalar families of tests/msm_digit_model.py.  Honest random witnesses
almost never reach them at wide windows: a digit is the top one with probability 2^-c.

The reference throughout is the oracle's naive fold (O.g1_msm_naive / O.g2_msm_naive) or its trapdoor provers on the same bytes, compared bit for bit;
the bases are fixed random points made with the ORACLE's scalar multiplication.  Every case first asserts from the model that its scalars land in the
buckets it is about.

Who folds (held by text in tests/test_msm_digit_model.py): zk_msm_g1 / zk_msm_g2 never run the subgroup test, so they never take folded digits,
with or without ZK_MSM_API_PRECOMP -- they run every width in the PLAIN form, the folded families' scalars included.  Folded digits are reached
where the library takes them: the short products of a resident handle (5 bits, 51 windows) and proving keys at c = 3, 5, 15, 17, whose witness here IS
the family list; a pair s, r - s on two variables with EQUAL key points puts P + (-P) into one bucket of the folded chain."""
import random
from collections import Counter

import numpy as np
import pytest

import msm_digit_model as M
import oracle_lib as O
from oracle import pyref as P
from test_gpu_msm_collisions import SETTINGS
from test_gpu_options import Setup, device_list, frs, options, run_pinocchio
from zukelang_amd import pinocchio as PIN
from zukelang_amd import r1cs as RC
from zukelang_amd.curve import G1, G2
from zukelang_amd.groth16 import Groth16, PKey

pytestmark = pytest.mark.gpu

N_POINTS = 300
LEAD = 5                                 # every product starts with: P0, P0 again, P1, -P1, the identity
GROUPS = ("G1", "G2")


class Curve:
    def __init__(self, G, naive, mul, gen, seed):
        self.G, self.naive, self.mul = G, naive, mul
        rng = random.Random(seed)
        k = lambda: P.fr_to_bytes(rng.randrange(1, P.R))
        self.inf = bytes([0x40]) + bytes(G.POINT_BYTES - 1)
        pts = [mul(gen(), k()) for _ in range(N_POINTS - 3)]
        self.points = [pts[0], pts[0], pts[1], mul(pts[1], P.fr_to_bytes(P.R - 1)), self.inf] + pts[2:]
        self.identity = [False] * 4 + [True] + [False] * (N_POINTS - LEAD)
        assert len(self.points) == N_POINTS and len(set(self.points)) == N_POINTS - 1 and self.points[3] != self.points[2]
        rc, zero = naive(self.points[2] + self.points[3], frs([1, 1]))
        assert rc == 0 and zero == self.inf                       # an exact negation
        self._refs = {}

    def bases(self, n):
        return b"".join(self.points[:n])

    def ref(self, scalars):
        """the oracle's naive fold of `scalars` over the first points, computed once per scalar list"""
        key = tuple(scalars)
        if key not in self._refs:
            rc, out = self.naive(self.bases(len(scalars)), frs(scalars))
            assert rc == 0
            self._refs[key] = out
        return self._refs[key]


_curves = {}


def curve(group):
    if group not in _curves:
        _curves[group] = (Curve(G2, O.g2_msm_naive, O.g2_mul, O.g2_generator, 0xD162) if group else Curve(G1, O.g1_msm_naive, O.g1_mul, O.g1_generator, 0xD161))
    return _curves[group]


def lead(c, fold):
    """the five scalars on P0, P0, P1, -P1, the identity: a pair s, r - s on one point (in a folded form: one bucket per window, opposite signs),
    the all-top scalar on a point and on its negation (P + (-P) in the top bucket of every window it fills), and a scalar that must never be filed"""
    t = M.all_top(c, fold)[1]
    return [t, M.R - t, t, t, M.all_bottom(c, fold)[1]]


def product(c, fold):
    """(names, scalars) of the whole family list of a form as ONE product; in the plain form of a width that can fold, the folded family's own scalars too"""
    fam = M.families(c, fold)
    if not fold and 1 in M.forms(c):
        have = {s for _, s in fam}
        fam = fam + [("folded " + n, s) for n, s in M.families(c, 1) if s not in have]
    scalars = lead(c, fold) + [s for _, s in fam]
    assert len(scalars) <= N_POINTS
    return ["lead"] * LEAD + [n for n, _ in fam], scalars


def assert_lands(c, fold, precomp, scalars, identity, led=True):
    """from the model: the scalars that are filed reach every end of the plan (msm_digit_model.check_coverage), and the buckets at those ends hold them"""
    live = [s for s, i in zip(scalars, identity) if s and not i]
    got = M.check_coverage(c, fold, live)
    nw, nbw = M.msm_windows(c, fold), 1 << (c - 1)
    keys = Counter(M.bucket_keys(scalars, c, precomp, identity, fold))
    assert all(0 <= k < (1 if precomp else nw) * nbw for k in keys)
    for j in got["tops"]:
        assert keys[(0 if precomp else j * nbw) + nbw - 1] >= 1, (c, fold, j)                 # the top bucket (of window j)
    for j in got["bottoms"]:
        assert keys[(0 if precomp else j * nbw) + M.bias(c) - 1] >= 1, (c, fold, j)           # the bottom digit's bucket
    if precomp:
        assert keys[nbw - 1] >= nw - 1
    if led:
        a, b = (M.recode(s, c, fold) for s in scalars[:2])                                     # the pair on P0
        assert scalars[0] + scalars[1] == M.R
        if fold:
            assert [(k, j) for k, _, j in a.keys_precomp] == [(k, j) for k, _, j in b.keys_precomp] and a.digits == [-d for d in b.digits]
        assert M.recode(scalars[2], c, fold).keys_classic == M.recode(scalars[3], c, fold).keys_classic != []    # t on P1 and on -P1
    return got


def run_product(group, c, precomp, settings=None):
    """the family list of (c, plain) through zk_msm_g1 / zk_msm_g2: the entry points never fold"""
    cv = curve(group)
    names, scalars = product(c, 0)
    n = len(scalars)
    assert_lands(c, 0, precomp, scalars, cv.identity[:n])
    with options(dict(settings or {}, **({"ZK_MSM_API_PRECOMP": 1} if precomp else {}))):
        got = bytes(cv.G.apply_powers(frs(scalars), cv.bases(n), c))
    return got == cv.ref(scalars)


# ---- a. every width through the MSM entry points
@pytest.mark.parametrize("c", list(M.WIDTHS))
def test_the_family_list_through_the_window_tables(c):
    """ZK_MSM_API_PRECOMP=1: window tables and ONE bucket set of at most 2^21 buckets, c = 2..22, both groups"""
    bad = [GROUPS[g] for g in (0, 1) if not run_product(g, c, True)]
    assert not bad, (c, "window tables, plain digits", bad)


# Classic widths above 17 are left out on purpose: they run the same reduction kernels as the widths below over nw bucket sets of 2^(c-1) buckets each
# and would allocate several gigabytes on a shared machine for no new code path.
@pytest.mark.parametrize("c", list(range(2, 18)))
def test_the_family_list_in_the_classic_layout(c):
    bad = [GROUPS[g] for g in (0, 1) if not run_product(g, c, False)]
    assert not bad, (c, "classic layout", bad)


def lone_expectation(name, s, c):
    """what the model says about a family member that is the whole product: the buckets of a one-window table it fills"""
    rc = M.recode(s, c, 0)
    nbw = 1 << (c - 1)
    assert rc.keys_precomp and not rc.flipped
    kind, _, at = name.partition("@")
    if kind == "top" and "," not in at:
        assert rc.keys_precomp == [(nbw - 1, False, int(at))]                # one point in the top bucket and nothing else
    if kind == "carry":
        assert rc.keys_precomp == [(M.bias(c) - 1, True, int(at)), (0, False, int(at) + 1)]
    if name == "all top":
        assert {k for k, _, _ in rc.keys_precomp} == {nbw - 1}
    return rc


@pytest.mark.parametrize("group", (0, 1), ids=GROUPS)
@pytest.mark.parametrize("c", [5, 10, 11, 16, 17, 22])
def test_every_family_member_as_a_product_of_its_own(c, group):
    """one scalar on one base: the emptiest shapes the weighting step sees"""
    cv = curve(group)
    base = cv.points[LEAD]
    bad = []
    with options({"ZK_MSM_API_PRECOMP": 1}):
        for name, s in list(zip(*product(c, 0)))[LEAD:]:
            lone_expectation(name, s, c)
            if bytes(cv.G.apply_powers(frs([s]), base, c)) != cv.mul(base, P.fr_to_bytes(s)):
                bad.append(name)
    assert not bad, (GROUPS[group], c, bad)


# ---- b. the top and bottom buckets in every form of the reduction
FORM_WIDTHS = (10, 11, 16, 17, 22)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join("%s=%s" % (k.replace("ZK_", ""), v) for k, v in s.items()) or "defaults")
def test_the_ends_in_every_form_of_the_reduction(setting):
    bad = [(GROUPS[g], c) for c in FORM_WIDTHS for g in (0, 1) if not run_product(g, c, True, setting)]
    assert not bad, (setting, bad)


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("c", [5, 16])
def test_the_ends_after_batch_affine_rounds(c, rounds):
    bad = [GROUPS[g] for g in (0, 1) if not run_product(g, c, True, {"ZK_MSM_BA_ROUNDS": rounds})]
    assert not bad, (c, rounds, bad)


# ---- c. folded signs
@pytest.mark.parametrize("c", [3, 5, 15, 17])
def test_a_scalar_and_its_negative_through_the_entry_points(c):
    """s P + (r - s) P = O, bytes 40 00 .. 00, and s P + (r - s) Q, for the pairs of the folded families; the same bytes under ZK_KEY_SUBGROUP_CHECK=0.  These
    entry points take plain digits either way (the module's docstring): the two scalars of a pair share no bucket here"""
    for group in (0, 1):
        cv = curve(group)
        for name, s, t in M.mirror_pairs(c):
            assert s + t == M.R and M.recode(s, c, 0).keys_precomp and M.recode(t, c, 0).keys_precomp and not M.recode(t, c, 0).flipped
            apart = [s, 0, t]                                       # P0, (P0), P1
            for chk in ({}, {"ZK_KEY_SUBGROUP_CHECK": 0}):
                with options(dict(chk, ZK_MSM_API_PRECOMP=1)):
                    assert bytes(cv.G.apply_powers(frs([s, t]), cv.bases(2), c)) == cv.inf, (GROUPS[group], c, name, chk)
                    assert bytes(cv.G.apply_powers(frs(apart), cv.bases(3), c)) == cv.ref(apart) != cv.inf, (GROUPS[group], c, name, chk)


# ---- d. the resident handle: the short products' own use of the recoding, folded and plain, and the chain
def split(scalars, most):
    """two or more products of at most `most` scalars, each led by the five lead scalars"""
    body = scalars[LEAD:]
    parts = max(2, -(-len(body) // (most - LEAD)))
    size = -(-len(body) // parts)
    out = [scalars[:LEAD] + body[k:k + size] for k in range(0, len(body), size)]
    assert len(out) >= 2 and all(len(p) <= most for p in out) and sum(len(p) - LEAD for p in out) == len(body)
    return out


@pytest.mark.parametrize("checked", [True, False], ids=["folded", "plain"])
@pytest.mark.parametrize("group", (0, 1), ids=GROUPS)
def test_the_ends_on_a_resident_handle(group, checked):
    cv = curve(group)
    c, fold = M.SHORT_C, 1 if checked else 0
    assert M.msm_fold(c, True, checked) == bool(fold) and M.msm_windows(c, fold) == (51 if checked else 52)
    names, scalars = product(c, fold)
    assert_lands(c, fold, True, scalars, cv.identity[:len(scalars)])
    with options({} if checked else {"ZK_KEY_SUBGROUP_CHECK": 0}):
        rb = cv.G.resident(np.frombuffer(cv.bases(N_POINTS), dtype=np.uint8))
    with rb:
        assert rb.short_max == (256, 64)[group] and rb.n == N_POINTS
        parts = split(scalars, min(rb.short_max, 64))
        # pairs s, r - s on ONE point (P0 twice: in the folded form one bucket per window holds P and -P) and on two, as short products of two and three scalars
        pairs = [[s, t] for _, s, t in M.mirror_pairs(c)] + [[s, 0, t] for _, s, t in M.mirror_pairs(c)]
        for s, t in pairs[:3]:
            a, b = M.recode(s, c, fold), M.recode(t, c, fold)
            assert (a.raw == b.raw and a.flipped != b.flipped) if fold else not (a.flipped or b.flipped)
        got = [bytes(x) for x in rb.apply_powers_many([frs(p) for p in parts + pairs])]       # two or more products, none longer than short_max: the short path
        for p, g in zip(parts + pairs, got):
            assert g == cv.ref(p), (GROUPS[group], checked, "short", len(p))
            assert g == bytes(cv.G.apply_powers(frs(p), cv.bases(len(p)))), (GROUPS[group], checked, "zk_msm", len(p))
        assert all(g == cv.inf for g in got[len(parts):len(parts) + 3])
        whole = bytes(rb.apply_powers(frs(scalars)))                                            # a lone product: the chain
        assert whole == cv.ref(scalars) == bytes(cv.G.apply_powers(frs(scalars), cv.bases(len(scalars)))), (GROUPS[group], checked, "chain")


# ---- e. a witness that IS the family list, through a proving key at every width
N_GATES, N_MIRROR = 512, 3
N_PLAIN = N_GATES - N_MIRROR


def free_circuit():
    """512 gates over free variables.  Gate i < 509: v_i * ONE = v_i, the variable in the L row for even i and in the R row for odd i, so in the Lagrange
    form the G1 product of A and the G2 product of B see witness values directly (ltd_mid sees them in every form).  The last three gates are
    (a_k + b_k) * ONE = o_k: a_k and b_k occur in the same row with the same coefficient and nowhere else, so their key points are EQUAL, and a witness
    a_k = s, b_k = r - s, o_k = 0 puts P and -P into one bucket wherever the key's digits fold.  Variables: ONE, v_0 .. v_508, then a_k, b_k, o_k."""
    ONE = 0
    L, R_, O_ = [], [], []
    for i in range(N_PLAIN):
        v = 1 + i
        L.append({v: 1} if i % 2 == 0 else {ONE: 1})
        R_.append({ONE: 1} if i % 2 == 0 else {v: 1})
        O_.append({v: 1})
    for k in range(N_MIRROR):
        a = 1 + N_PLAIN + 3 * k
        L.append({a: 1, a + 1: 1})
        R_.append({ONE: 1})
        O_.append({a + 2: 1})
    m = 1 + N_PLAIN + 3 * N_MIRROR
    mid = np.ones(m, dtype=np.uint8)
    mid[0] = mid[1] = 0                                              # public: ONE and v_0
    return RC.R1CS(N_GATES, m, RC.Matrix.from_rows(L), RC.Matrix.from_rows(R_), RC.Matrix.from_rows(O_), mid)


def family_witness(c, fold):
    """[1], the family list of (c, form) on the free variables, seeded random values behind it; the pairs s, r - s of a folded form on the equal key points"""
    rng = random.Random(0xD163 + c)
    fam = [s for n, s in M.families(c, fold) if not n.startswith("mirror")]
    w = [1] + fam + [rng.randrange(1, M.R) for _ in range(N_PLAIN - len(fam))]
    pairs = [(s, t) for _, s, t in M.mirror_pairs(c)] if fold else [(rng.randrange(1, M.R), rng.randrange(1, M.R)) for _ in range(N_MIRROR)]
    for s, t in pairs:
        w += [s, t, (s + t) % M.R]
    return w


class Keys:
    """the circuit, its Groth16 key (from the oracle's setup exponents) and its Pinocchio key, built once"""
    def __init__(self):
        self.cs = free_circuit()
        self.csr = [O.CSR(X.ptr, X.col, X.val) for X in (self.cs.L, self.cs.R, self.cs.O)]
        st = P.fr_stream(0x5EEDD164)
        self.toxic = [next(st) for _ in range(5)]
        self.rs = (next(st), next(st))
        e1, e2, _ = O.groth16_setup_exponents(self.cs.n, self.cs.m, *self.csr, self.cs.mid, frs(self.toxic))
        self.pk = PKey(G1.of_Fr(e1), G2.of_Fr(e2))
        self.ptoxic = [next(st) for _ in range(8)]
        it = iter(self.ptoxic)
        self.ppk, _ = PIN.ZK.keygen(lambda: next(it), self.cs)
        self.blind = [[next(st) for _ in range(3)] for _ in range(3)] + [[0, 0, 0]]


_keys = []


def keys():
    if not _keys:
        _keys.append(Keys())
    return _keys[0]


def key_form(c):
    """a proving key's points pass the subgroup test at upload: its window tables fold wherever the width allows"""
    return 1 if M.msm_fold(c, True, True) else 0


def witness_for_key(c):
    k, fold = keys(), key_form(c)
    w = family_witness(c, fold)
    assert len(w) == k.cs.m and k.cs.check(w)
    assert_lands(c, fold, True, w[1:], [False] * (k.cs.m - 1), led=False)
    if fold:
        for q in range(N_MIRROR):
            a, b, o = w[1 + N_PLAIN + 3 * q:4 + N_PLAIN + 3 * q]
            ra, rb = M.recode(a, c, fold), M.recode(b, c, fold)
            assert o == 0 and ra.raw == rb.raw and ra.flipped != rb.flipped and ra.keys_precomp           # same buckets, opposite signs, on equal points
    return w


def prove_groth16(c):
    k = keys()
    w = witness_for_key(c)
    r, s = k.rs
    expect = O.groth16_prove_trapdoor(k.cs.n, k.cs.m, *k.csr, k.cs.mid, frs(w), frs(k.toxic), P.fr_to_bytes(r), P.fr_to_bytes(s))
    with options({"ZK_MSM_WINDOW": c}):                              # read when the key's base tables are built
        pr = Groth16(k.cs, k.pk)
        try:
            got = pr.prove_rs(w, r, s)
            assert (got.a, got.b, got.c) == expect, (c, "as uploaded")
            pr.derive_lagrange()
            got = pr.prove_rs(w, r, s)
            assert (got.a, got.b, got.c) == expect, (c, "derived")
        finally:
            pr.close()


@pytest.mark.parametrize("c", list(M.WIDTHS))
def test_a_witness_of_the_family_list_through_a_groth16_key(c):
    prove_groth16(c)


def test_a_witness_of_the_family_list_on_a_device_list():
    with device_list([0, 0]):
        prove_groth16(17)


@pytest.mark.parametrize("c", [5, 16, 17, 22])
def test_a_witness_of_the_family_list_through_a_pinocchio_key(c):
    k = keys()
    w = witness_for_key(c)
    exp = [O.pinocchio_prove_trapdoor(k.cs.n, k.cs.m, *k.csr, k.cs.mid, frs(w), frs(k.ptoxic), *(P.fr_to_bytes(x) for x in d)) for d in k.blind]
    with options({"ZK_MSM_WINDOW": c}):
        run_pinocchio(Setup(k.cs, w, k.csr, k.ptoxic, k.ppk, k.blind, exp), ("window", c))
