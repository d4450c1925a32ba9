"""Degenerate trapdoors and blindings on the device (tests/degenerate_cases.py: the table, the circuits and where each expectation comes from;
tests/test_degenerate_trapdoors.py holds the table and the oracle's shortcuts without a GPU).  tau (Pinocchio: s) inside the domain 0 .. n-1 makes
the tau-power list one generator followed by identities (tau = 0), all one point (tau = 1) or P, -P, P, .. (tau = r-1), the Lagrange pools a unit
vector of points with tiztd / hl all identity; on the shifted points n .. 2n-2 the lambda basis is the unit vector; alpha = beta = 0 makes a, b1,
b2 the identity.  One test per layer, so that a failure names its layer:

  a. making a key: the host keygens and the device keygens in both forms -- key bytes and the handle's pools;
  b. taking a key: upload, wire upload, Lagrange-form upload, the derivation in the exponent (csrc/lagrange_derive.hip) -- pools and proofs;
  c. both key checks: mask 0 on every honest handle of b, and one wrong point in a degenerate key still raises its bit;
  d. a delta contribution on a key whose tail is all identities;
  e. blindings that make A and B the identity, through every prove call and every verifier, for both protocols;
  f. the same keys on the device list [0, 0];
  g. an unsatisfied witness where (v w - y)(tau) = 0 cannot tell.

Every comparison is of exact bytes.  Expected key bytes and proofs: the literal oracle at n <= 64, the trapdoor forms at n = 1025; expected
Lagrange-form pools: the oracle's points of exponents built from degenerate_cases.lagrange_ref.  Measured on an MI355X, the module alone: all 329
cases 210 s, the slowest 2.4 s (making a key at n = 1025, tau = r-1: the oracle multiplies 4400 points for the expected pools)."""
import functools

import numpy as np
import pytest

import degenerate_cases as D
import oracle_lib as O
from zukelang_amd import _lib
from zukelang_amd import pinocchio as PIN
from zukelang_amd.curve import G1, G2, Pairing
from zukelang_amd.groth16 import Groth16, PKey, VKey

pytestmark = pytest.mark.gpu

R = D.R
SEEDS = [bytes(range(32)), bytes([0xA5] * 32)]
ZK_ERR_REMAINDER = -4
arr = lambda b: np.frombuffer(bytes(b), dtype=np.uint8)
abc = lambda p: (p.a, p.b, p.c)
G16_CASES = D.cases(D.CIRCUITS, D.groth16_rows)
PIN_CASES = D.cases(D.CIRCUITS, D.pinocchio_rows)


def _set_option(name, value):
    _lib.check(_lib.lib().zk_set_option(name.encode(), None if value is None else str(value).encode()))


@pytest.fixture(scope="module", autouse=True)
def _init_and_leave_nothing_behind():
    _lib.check(_lib.lib().zk_init(0))
    yield
    _lib.set_device_list([0])          # ZK_ERR_ARG while any key handle is alive


# ---- what is expected, once per row
class G16World:
    def __init__(self, name, tox):
        self.name, self.tox = name, tuple(tox)
        self.cs, self.w = D.circuit(name)
        self.pk1, self.pk2, self.vk1, self.vk2 = D.groth16_key(name, self.tox)
        self.io = [self.w[k] for k in D.public(name)]

    @functools.cached_property
    def lag(self):
        """the Lagrange-form pools: the oracle's points of exponents built from lagrange_ref (made when a test first asks for them)"""
        _e1, _e2, _eio, l1, l2 = D.groth16_exponents_ref(self.name, self.tox)
        return D.points1(tuple(l1)), D.points2(tuple(l2))

    lag1 = property(lambda self: self.lag[0])
    lag2 = property(lambda self: self.lag[1])

    @functools.cached_property
    def pk(self):
        return PKey(arr(self.pk1), arr(self.pk2), arr(self.lag1), arr(self.lag2))

    def pools(self, form):
        return (self.lag1, self.lag2) if form == "lagrange" else (self.pk1, self.pk2)

    def vkey(self):
        v1, v2 = self.vk1, self.vk2
        return VKey(v1[:96], arr(v1[96:]), v2[:192], v2[192:384], v2[384:], Pairing.pairing(self.pk1[:96], self.pk2[:192]))

    def proof(self, r, s):
        return D.groth16_proof(self.name, self.tox, r, s)

    def wire(self, r, s):
        a, b, c = self.proof(r, s)
        return O.g1_compress(a) + O.g2_compress(b) + O.g1_compress(c)


_g16 = {}


def g16_world(name, label, tox=None):
    if (name, label) not in _g16:
        _g16[name, label] = G16World(name, tox or D.row(D.groth16_rows, name, label))
    return _g16[name, label]


class PinWorld:
    def __init__(self, name, tox):
        self.name, self.tox = name, tuple(tox)
        self.cs, self.w = D.circuit(name)
        self.key = D.pinocchio_key(name, self.tox)
        self.pk = PIN.PKey(arr(self.key[0]), arr(self.key[1]))
        self.vk = PIN.VKey(arr(self.key[2]), arr(self.key[3]))
        self.io = [self.w[k] for k in D.public(name)]
        n, m, nm = self.cs.n, self.cs.m, int(np.count_nonzero(self.cs.mid))
        self.si = self.key[0][96 * 5 * nm:96 * (5 * nm + n + 1)]
        self.vw_all = self.key[0][96 * (5 * nm + n + 1):96 * (5 * nm + n + 1 + 2 * m)]
        head = D.pinocchio_h_exponents_ref(name, self.tox, True)
        self.derived_compact = D.points1(tuple(head))                          # lambda (n-1) | Z | 1 | s^(n-1)
        self.derived_full = self.derived_compact[:96 * (n + 1)] + self.vw_all      # lambda | Z | 1 | v_all | w_all
        assert self.derived_compact[96 * (n + 1):] == self.si[96 * (n - 1):96 * n]

    def pool5(self, derived, compact):
        if derived:
            return self.derived_compact if compact else self.derived_full
        return self.si if compact else self.si + self.vw_all

    def proof(self, d):
        return D.pinocchio_proof(self.name, self.tox, tuple(d))


_pin = {}


def pin_world(name, label, tox=None):
    if (name, label) not in _pin:
        _pin[name, label] = PinWorld(name, tox or D.row(D.pinocchio_rows, name, label))
    return _pin[name, label]


def g16_is_key(pr, wd, form, tag, label):
    got = (bytes(pr.pool_points(1)), bytes(pr.pool_points(2)))
    want = wd.pools(form)
    assert got[0] == want[0], (tag, "G1 pool", [i for i in range(len(want[0]) // 96) if got[0][96 * i:96 * i + 96] != want[0][96 * i:96 * i + 96]][:8])
    assert got[1] == want[1], (tag, "G2 pool", [i for i in range(len(want[1]) // 192) if got[1][192 * i:192 * i + 192] != want[1][192 * i:192 * i + 192]][:8])
    for r, s in D.draws(wd.name, label, 2):
        assert abc(pr.prove_rs(wd.w, r, s)) == wd.proof(r, s), (tag, "proof")


def g16_masks(pr, wd, form, tag):
    """c, the honest half: mask 0 with and without the verification key, under two seeds"""
    check = pr.check_lagrange_key if form == "lagrange" else pr.check_key
    vkey = wd.vkey()
    for seed in SEEDS:
        for v in (None, vkey):
            res = check(v, seed=seed)
            assert res.failed == 0, (tag, form, "with vkey" if v else "without", res.names)


def pin_is_key(pr, wd, derived, compact, tag, label):
    n, m = wd.cs.n, wd.cs.m
    assert pr.pool_size(5) == len(wd.pool5(derived, compact)) // 96, (tag, "h pool size")
    got, want = bytes(pr.pool_points(5)), wd.pool5(derived, compact)
    assert got == want, (tag, "h pool", [i for i in range(len(want) // 96) if got[96 * i:96 * i + 96] != want[96 * i:96 * i + 96]][:8])
    for d in D.draws(wd.name, label, 2, 3) + [(0, 0, 0)]:
        assert pr.prove_with(wd.w, *d).to_bytes() == wd.proof(d), (tag, "proof", "ZK" if any(d) else "NonZK")


# ---- a. making a key
@pytest.mark.parametrize("name,label", G16_CASES)
def test_groth16_making_a_key(name, label):
    wd = g16_world(name, label)
    it = iter(wd.tox)
    pk, vk = Groth16.keygen(lambda: next(it), wd.cs, lagrange=True)
    assert bytes(pk.g1) == wd.pk1 and bytes(pk.g2) == wd.pk2, "host keygen, tau powers"
    assert bytes(pk.lag_g1) == wd.lag1, "host keygen, Lagrange-form G1 pool"
    assert bytes(pk.lag_g2) == wd.lag2, "host keygen, Lagrange-form G2 pool"
    assert bytes(vk.one1) + bytes(vk.ltgm_io) == wd.vk1 and bytes(vk.one2) + bytes(vk.gm) + bytes(vk.d) == wd.vk2, "host keygen, vkey"
    assert vk.ab == wd.vkey().ab
    for form in ("lagrange", "tau_powers"):
        it = iter(wd.tox)
        pr, gpk, gvk = Groth16.generate(lambda: next(it), wd.cs, form=form)
        try:
            assert bytes(gpk.g1) == wd.pk1 and bytes(gpk.g2) == wd.pk2, ("device keygen, pkey", form)
            assert bytes(gvk.one1) + bytes(gvk.ltgm_io) == wd.vk1 and bytes(gvk.one2) + bytes(gvk.gm) + bytes(gvk.d) == wd.vk2, ("device keygen, vkey", form)
            g16_is_key(pr, wd, form, "device keygen, " + form, label)
        finally:
            pr.close()


@pytest.mark.parametrize("name,label", PIN_CASES)
def test_pinocchio_making_a_key(name, label):
    wd = pin_world(name, label)
    it = iter(wd.tox)
    pk, vk = PIN.keygen(lambda: next(it), wd.cs)
    assert (bytes(pk.g1), bytes(pk.g2), bytes(vk.g1), bytes(vk.g2)) == wd.key, "host keygen"
    for form in ("lagrange", "tau_powers"):
        it = iter(wd.tox)
        pr, gpk, gvk = PIN.generate(lambda: next(it), wd.cs, form=form)
        try:
            assert (bytes(gpk.g1), bytes(gpk.g2), bytes(gvk.g1), bytes(gvk.g2)) == wd.key, ("device keygen", form)
            pin_is_key(pr, wd, form == "lagrange", True, "device keygen, " + form, label)
        finally:
            pr.close()


# ---- b. taking a key (and c: the honest masks)
@pytest.mark.parametrize("name,label", G16_CASES)
def test_groth16_taking_a_key(name, label):
    wd = g16_world(name, label)
    makers = [("upload", lambda: Groth16(wd.cs, wd.pk)),
              ("wire upload", lambda: Groth16.from_compressed(wd.cs, G1.to_compressed_bytes_many(wd.pk1), G2.to_compressed_bytes_many(wd.pk2)))]
    for tag, make in makers:
        pr = make()
        try:
            g16_is_key(pr, wd, "tau_powers", tag, label)
            g16_masks(pr, wd, "tau_powers", tag)
            pr.derive_lagrange()
            g16_is_key(pr, wd, "lagrange", tag + ", derived", label)
            g16_masks(pr, wd, "lagrange", tag + ", derived")
        finally:
            pr.close()
    pr = Groth16(wd.cs, wd.pk, lagrange=True)
    try:
        g16_is_key(pr, wd, "lagrange", "Lagrange-form upload", label)
        g16_masks(pr, wd, "lagrange", "Lagrange-form upload")
    finally:
        pr.close()


@pytest.mark.parametrize("name,label", PIN_CASES)
def test_pinocchio_taking_a_key(name, label):
    wd = pin_world(name, label)
    n = wd.cs.n
    for compact in (True, False):
        _set_option("ZK_PIN_COMPACT_H", None if compact else "0")
        try:
            pr = PIN.ZK(wd.cs, wd.pk)
        finally:
            _set_option("ZK_PIN_COMPACT_H", None)
        try:
            tag = "compact h pool" if compact else "full h pool"
            pin_is_key(pr, wd, False, compact, tag, label)
            pr.derive_lagrange()
            pin_is_key(pr, wd, True, compact, tag + ", derived", label)
        finally:
            pr.close()
    pr = PIN.ZK.from_lagrange(wd.cs, wd.pk, arr(wd.derived_compact[:96 * n]))
    try:
        pin_is_key(pr, wd, True, True, "zk_pinocchio_pk_upload_lagrange", label)
    finally:
        pr.close()


# ---- c. a degenerate honest key must not blind the check
def _put(points, index, point):
    return points[:96 * index] + point + points[96 * (index + 1):]


@pytest.mark.parametrize("name,label", [("cubic6", "tau=n-1"), ("cubic6", "alpha=beta=0"), ("random24", "tau=0")])
def test_one_wrong_point_in_a_degenerate_key_raises_its_bit(name, label):
    """tau inside the domain: tiztd / hl are all the identity and, for tau in 1 .. n-1, so is l2[0] = [l_0(tau)]_2, which the Lagrange form's h-bases
    relation pairs against.  alpha = beta = 0: a, b1, b2 are the identity, L_k(tau) = y_k(tau).  The mask must be non-zero and hold the named bit;
    further bits may follow what include/zkmi355x.h says a relation also trips."""
    wd = g16_world(name, label)
    n = wd.cs.n
    g = O.g1_generator()
    other = O.g1_mul(g, D.frb(D.draws(name, label, 1, 1)[0][0]))
    vkey = wd.vkey()
    H, L = _lib.KEYCHK_BITS["h_bases"], _lib.KEYCHK_BITS["l"]
    cases = [("tau_powers", "tiztd[0] = g", _put(wd.pk1, 3 + n + 2, g), H),
             ("tau_powers", "ltd_mid[0] = another point", _put(wd.pk1, 3 + n + 2 + n - 1, other), L),
             ("lagrange", "hl[0] = g", _put(wd.lag1, 3 + n, g), H),
             ("lagrange", "ltd_mid[0] = another point", _put(wd.lag1, 3 + n + n - 1, other), L)]
    for form, what, g1, bit in cases:
        assert g1 != wd.pools(form)[0]
        pk = PKey(arr(g1), arr(wd.pk2), arr(g1), arr(wd.lag2))
        pr = Groth16(wd.cs, pk, lagrange=form == "lagrange")
        try:
            check = pr.check_lagrange_key if form == "lagrange" else pr.check_key
            for seed in SEEDS:
                for v in (None, vkey):
                    res = check(v, seed=seed)
                    assert res.failed and res.failed & bit, (form, what, "with vkey" if v else "without", res.names)
        finally:
            pr.close()


# ---- d. contribution
@pytest.mark.parametrize("name,label,form", [(n, l, f) for n, l in (("cubic6", "tau=n-1"), ("random24", "tau=0")) for f in ("tau_powers", "lagrange")])
def test_contribution_to_a_key_whose_tail_is_all_identities(name, label, form):
    wd = g16_world(name, label)
    n = wd.cs.n
    tail = slice(96 * (3 + (n + 2 if form == "tau_powers" else n)), 96 * (3 + (n + 2 if form == "tau_powers" else n) + n - 1))
    assert wd.pools(form)[0][tail] == D.IDENT1 * (n - 1)
    for tag, dmul in (("1", 1), ("r-1", R - 1), ("random", D.draws(name, label, 1, 1)[0][0])):
        tox = list(wd.tox)
        tox[D.G16["delta"]] = tox[D.G16["delta"]] * dmul % R
        new = g16_world(name, label + " delta*" + tag, tox)
        pr = Groth16(wd.cs, wd.pk, lagrange=form == "lagrange")
        try:
            c = pr.contribute(dmul)
            assert c.d1_before == wd.pk1[96:192] and c.d1_after == new.pk1[96:192] and c.vk_d == new.vk2[384:], (tag, "link")
            assert c.dmul_g2 == O.g2_mul(O.g2_generator(), D.frb(dmul)), (tag, "[delta']_2")
            g16_is_key(pr, new, form, "contributed, delta' = " + tag, label)
            assert bytes(pr.pool_points(1))[tail] == D.IDENT1 * (n - 1), (tag, "the identity tail stays the identity")
            g16_masks(pr, new, form, "contributed, delta' = " + tag)
        finally:
            pr.close()


# ---- e. blindings
def _every_groth16_verifier(vkey, ios, proofs, want, tag):
    """host verify, verify_many, the resident key per proof and folded, both again from the compressed wire bytes: each must say `want`"""
    for io, p in zip(ios, proofs):
        assert Groth16.verify(io, vkey, p) == want, (tag, "verify")
    assert Groth16.verify_many(ios, vkey, proofs) == [want] * len(proofs), (tag, "verify_many")
    with vkey.resident() as res:
        for compressed in (False, True):
            assert res.verify_many(ios, proofs, compressed=compressed) == [want] * len(proofs), (tag, "resident", compressed)
            assert res.verify_all(ios, proofs, compressed=compressed) == want, (tag, "folded", compressed)
            assert res.verify_many(ios, proofs, fold_first=True, compressed=compressed) == [want] * len(proofs), (tag, "fold first", compressed)


def _changed_inputs(count, accepted):
    """the first and the last public input, and the first one whose change must be ACCEPTED (its key point is the identity), if there is one"""
    return sorted({0, count - 1} | set([j for j in range(count) if accepted(j)][:1]))


E_CASES = [(name, label) for name in D.CIRCUITS for label in ("base", "tau=" + D.tau_label(name, D.n_of(name) - 1))] + [("random24", "tau=0"), ("cubic6", "alpha=beta=0")]


@pytest.mark.parametrize("name,label", E_CASES)
def test_groth16_blindings_through_every_prove_call_and_every_verifier(name, label):
    wd = g16_world(name, label, D.base_row(name, 5) if label == "base" else None)
    blinds = D.blindings(name, wd.tox)
    rs = [x for _, x in blinds]
    exp = [wd.proof(r, s) for r, s in rs]
    assert exp[0][0] == D.IDENT1 and exp[0][1] == D.IDENT2                      # the oracle's A and B under the first pair
    wire = [wd.wire(r, s) for r, s in rs]
    assert wire[0][:48] == D.IDENT1_WIRE and wire[0][48:144] == D.IDENT2_WIRE
    pr = Groth16(wd.cs, PKey(arr(wd.pk1), arr(wd.pk2)))
    try:
        for form in ("tau_powers", "derived"):          # b holds the derived pools of these keys to the expected Lagrange form
            if form == "derived":
                pr.derive_lagrange()
            proofs = [pr.prove_rs(wd.w, r, s) for r, s in rs]
            assert [abc(p) for p in proofs] == exp, (form, "prove_rs")
            assert proofs[0].a == D.IDENT1 and proofs[0].b == D.IDENT2 and proofs[0].to_compressed() == wire[0]
            pr.set_witness(wd.w)
            for order in ([0, 1], [2, 0]):
                for slot, i in enumerate(order):
                    pr.prove_async(None, *rs[i], slot)
                for slot, i in enumerate(order):
                    assert abc(pr.prove_wait(slot)) == exp[i], (form, "prove_async", blinds[i][0], slot)
            assert pr.prove_many(rs, [wd.w] * len(rs)) == wire, (form, "prove_many")
            assert pr.prove_many(rs, len(rs), in_flight=2) == wire, (form, "prove_many, resident witness")
    finally:
        pr.close()
    vkey = wd.vkey()
    _every_groth16_verifier(vkey, [wd.io] * len(proofs), proofs, True, "as proved")
    for j in _changed_inputs(len(wd.io), lambda j: D.groth16_accepts_changed_input(name, wd.tox, j)):
        io = list(wd.io)
        io[j] = (io[j] + 1) % R
        want = D.groth16_accepts_changed_input(name, wd.tox, j)
        assert want == (wd.vk1[96 * (1 + j):96 * (2 + j)] == D.IDENT1)
        _every_groth16_verifier(vkey, [io] * len(proofs), proofs, want, "public input %d changed" % j)


def _every_pinocchio_verifier(vk, ios, proofs, want, tag):
    for io, p in zip(ios, proofs):
        assert PIN.verify(io, vk, p) == want, (tag, "verify")
    assert PIN.verify_many(ios, vk, proofs) == [want] * len(proofs), (tag, "verify_many")
    with vk.resident() as res:
        for compressed in (False, True):
            assert res.verify_many(ios, proofs, compressed=compressed) == [want] * len(proofs), (tag, "resident", compressed)
            assert res.verify_all(ios, proofs, compressed=compressed) == want, (tag, "folded", compressed)
            assert res.verify_many(ios, proofs, fold_first=True, compressed=compressed) == [want] * len(proofs), (tag, "fold first", compressed)


@pytest.mark.parametrize("name,label", [("gate1", "s=0"), ("readme", "s=2"), ("cubic6", "base"), ("cubic6", "s=0"), ("cubic6", "s=n-1"), ("cubic6", "rv=0"),
                                        ("cubic6", "gm=0"), ("random24", "s=n"), ("cubic64", "s=n-1")])
def test_pinocchio_proofs_through_every_prove_call_and_every_verifier(name, label):
    """Verify.f's equations are identities in the exponent for every trapdoor: with Z(s) = 0 the key's yt and the seven t points are the identity,
    with rv = 0 every v point.  The verdict on a changed public input comes from degenerate_cases.pinocchio_accepts_changed_input."""
    wd = pin_world(name, label, D.base_row(name, 8) if label == "base" else None)
    ds = [(0, 0, 0)] + D.draws(name, label, 2, 3)
    exp = [wd.proof(d) for d in ds]
    c1, c2 = O.g1_compress, O.g2_compress
    wire = [b"".join((c2 if i in (1, 5) else c1)(p) for i, p in enumerate((e[:96], e[96:288], e[288:384], e[384:480], e[480:576], e[576:768], e[768:864], e[864:]))) for e in exp]
    pr = PIN.ZK(wd.cs, wd.pk)
    try:
        for stage in ("as uploaded", "derived"):
            if stage == "derived":
                pr.derive_lagrange()
            proofs = [pr.prove_with(wd.w, *d) for d in ds]
            assert [p.to_bytes() for p in proofs] == exp, (stage, "prove_with")
            pr.set_witness(wd.w)
            for slot in range(2):
                pr.prove_async(*ds[1 + slot], slot)
            for slot in range(2):
                assert pr.prove_wait(slot).to_bytes() == exp[1 + slot], (stage, "prove_async", slot)
            assert pr.prove_many(ds, [wd.w] * len(ds)) == wire, (stage, "prove_many")
    finally:
        pr.close()
    _every_pinocchio_verifier(wd.vk, [wd.io] * len(proofs), proofs, True, "as proved")
    for j in _changed_inputs(len(wd.io), lambda j: D.pinocchio_accepts_changed_input(name, wd.tox, ds[0], j)):
        io = list(wd.io)
        io[j] = (io[j] + 1) % R
        want = {D.pinocchio_accepts_changed_input(name, wd.tox, d, j) for d in ds}
        assert len(want) == 1                                                   # the blinding does not decide it on these rows
        _every_pinocchio_verifier(wd.vk, [io] * len(proofs), proofs, want.pop(), "public input %d changed" % j)


# ---- f. device list
@pytest.mark.parametrize("name", ["readme", "random24"])
def test_the_same_keys_on_two_entries_of_the_device_list(name):
    n = D.n_of(name)
    labels = ["tau=" + D.tau_label(name, v) for v in (0, n - 1, R - 1)]
    worlds = [(label, g16_world(name, label), pin_world(name, label.replace("tau=", "s="))) for label in labels]          # made before the list changes
    _lib.set_device_list([0, 0])
    try:
        for label, wd, pw in worlds:
            pr = Groth16(wd.cs, wd.pk)
            try:
                g16_is_key(pr, wd, "tau_powers", "two entries", label)
                pr.derive_lagrange()
                g16_is_key(pr, wd, "lagrange", "two entries, derived", label)
            finally:
                pr.close()
            pp = PIN.ZK(pw.cs, pw.pk)
            try:
                pin_is_key(pp, pw, False, True, "two entries", label.replace("tau=", "s="))
                pp.derive_lagrange()
                pin_is_key(pp, pw, True, True, "two entries, derived", label.replace("tau=", "s="))
            finally:
                pp.close()
    finally:
        _lib.set_device_list([0])


# ---- g. an unsatisfied witness
@pytest.mark.parametrize("name,label", [("readme", "tau=0"), ("cubic6", "tau=n-1"), ("random24", "tau=0"), ("cubic64", "tau=n-1"), ("random1025", "tau=n-1")])
def test_an_unsatisfied_witness_is_refused_where_tau_is_a_point_of_the_domain(name, label):
    """(v w - y)(tau) is ONE of the n values the witness must make zero: tiztd / hl are the identity, so the proof elements alone could not tell a
    witness that breaks another row.  The remainder check of QAP.ml:134 must."""
    wd = g16_world(name, label)
    bad = D.bad_witness(name)
    (r, s), = D.draws(name, label, 1)
    for form in ("tau_powers", "lagrange"):
        pr = Groth16(wd.cs, wd.pk, lagrange=form == "lagrange")
        try:
            with pytest.raises(AssertionError):
                pr.prove_rs(bad, r, s)
            with pytest.raises(AssertionError):
                pr.qap_eval(bad)
            _, codes = pr.prove_many([(r, s), (r, s)], [bad, wd.w], return_status=True)
            assert codes == [ZK_ERR_REMAINDER, 0], form
            assert abc(pr.prove_rs(wd.w, r, s)) == wd.proof(r, s), (form, "and the good witness afterwards")
        finally:
            pr.close()
    if name in D.LITERAL:
        plabel = label.replace("tau=", "s=")
        pw = pin_world(name, plabel)
        d, = D.draws(name, plabel, 1, 3)
        pp = PIN.ZK(pw.cs, pw.pk)
        try:
            for stage in ("as uploaded", "derived"):
                if stage == "derived":
                    pp.derive_lagrange()
                with pytest.raises(AssertionError):
                    pp.prove_with(bad, *d)
                assert pp.prove_with(pw.w, *d).to_bytes() == pw.proof(d), stage
        finally:
            pp.close()
