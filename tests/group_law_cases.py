"""The form table of zk_selftest_group and the operand battery of tests/test_gpu_group_law.py, importable without a GPU: tests/test_group_law_surface.py
holds the table to the functions csrc/ defines, the GPU test runs every row.  Everything here is oracle/pyref.py arithmetic."""
import random
from collections import Counter, namedtuple

from oracle import pyref as P

# name -> (form number of include/zkmi355x.h, second operand, the device function the row runs).  Second operands: "xyzz" | "affine" (the identity
# allowed) | "table" (affine, never the identity: the form's contract) | None (doublings) | "scalar".  `needs_affine_a`: the accumulator is an affine
# point or the identity, the contract of the 6-product addition and of the doubling of an affine point.
Form = namedtuple("Form", "number second function needs_affine_a g2_only")
FORMS = {
    "add": Form(0, "xyzz", "xyzz_add_impl", False, False),
    "dbl": Form(1, None, "xyzz_dbl_impl", False, False),
    "dbl_aff": Form(2, None, "xyzz_dbl_aff", True, False),
    "add_raw_mem": Form(3, "xyzz", "xyzz_add_raw_mem", False, False),
    "madd": Form(4, "affine", "xyzz_madd_impl", False, False),
    "madd_table": Form(5, "table", "xyzz_madd_impl", False, False),                 # madd<false>: no identity q, its contract
    "mmadd": Form(6, "affine", "xyzz_mmadd_impl", True, False),
    "madd_inline": Form(7, "affine", "xyzz_madd_impl", False, False),
    "madd_table_inline": Form(8, "table", "xyzz_madd_impl", False, False),
    "mmadd_inline": Form(9, "affine", "xyzz_mmadd_impl", True, False),
    "madd_parked": Form(10, "table", "xyzz_madd_parked", False, True),              # the park buffer exists for lane pairs only; q a table entry
    "add_slots": Form(11, "xyzz", "xyzz_add_slots", False, False),
    "dbl_slots": Form(12, None, "xyzz_dbl_slots", False, False),
    "jac_dbl": Form(13, None, "jac_dbl", False, False),
    "jac_madd": Form(14, "table", "jac_madd", False, False),                        # q "an AFFINE point that is not the identity"
    "jac_add": Form(15, "xyzz", "jac_add", False, False),
    "mul": Form(16, "scalar", "xyzz_mul_scalar_endo", False, False),
}
# reached only through a row above: the equal-x exit of every mixed addition, and the table and the conversion inside the scalar multiplication
COVERED_BY = {"xyzz_madd_equal_x": "madd", "xyzz_madd_equal_x_fn": "madd", "window_table_affine": "mul", "jac_to_xyzz": "mul"}

Z = P.BLS_X                      # |z|
Z2 = Z * Z
assert Z ** 4 - Z2 + 1 == P.R


class Group:
    """one of the two groups: field constructor, generator, encoders"""

    def __init__(self, index):
        self.index = index
        self.gen = P.G2 if index else P.G1
        self.to_bytes = P.g2_to_bytes if index else P.g1_to_bytes
        self.b = P.B2 if index else P.B1

    def fe(self, rng, nonzero=True):
        while True:
            v = P.Fp2(rng.randrange(P.P), rng.randrange(P.P)) if self.index else P.Fp1(rng.randrange(P.P))
            if not (nonzero and v.is_zero()):
                return v

    def const(self, c):
        return P.Fp2(c, 0) if self.index else P.Fp1(c)

    def fe_bytes(self, v):
        return (P._fp_be(v.b) + P._fp_be(v.a)) if self.index else P._fp_be(v.a)

    def xyzz_bytes(self, q):
        return b"".join(self.fe_bytes(c) for c in q)

    def aff_bytes(self, pt):
        zero = self.const(0)
        return b"".join(self.fe_bytes(c) for c in (pt if pt is not None else (zero, zero)))


REPRS = ("one", "random", "p-1")
IDENTITIES = ("zeros", "xy00")


def xyzz_of(g, pt, rep, rng):
    """an XYZZ representation of an affine point or None: (x l^2, y l^3, l^2, l^3); the identity as all zeros or as (x, y, 0, 0), x y != 0"""
    zero = g.const(0)
    if pt is None:
        return (zero, zero, zero, zero) if rep == "zeros" else (g.fe(rng), g.fe(rng), zero, zero)
    lam = {"one": g.const(1), "p-1": g.const(P.P - 1)}.get(rep) or g.fe(rng)
    l2 = lam * lam
    l3 = l2 * lam
    return (pt[0] * l2, pt[1] * l3, l2, l3)


Pair = namedtuple("Pair", "cls a_rep b_rep a b_xyzz b_aff expected")


def battery(index, seed=0x6A0B, points=28, generic=136, special=20):
    """(group, pairs, class counts): every class of the issue in every representation of either side; expected values once per pair of group elements"""
    g = Group(index)
    rng = random.Random(seed + index)
    pts = [P.pt_mul_jac(g.gen, rng.randrange(1, P.R)) for _ in range(points)]
    omega = pow(2, (P.P - 1) // 3, P.P)
    assert omega != 1 and pow(omega, 3, P.P) == 1
    cases = []          # (class, P, Q)
    for i in range(generic):
        cases.append(("generic", pts[i % points], pts[(i * 7 + 3) % points]))
    for i in range(special):
        p = pts[i]
        q = (p[0] * omega, p[1])          # (omega x)^3 = x^3: on the curve, same y, another x
        assert P.on_curve(q, g.b) and q[0] != p[0]
        cases += [("P+P", p, p), ("P-P", p, P.pt_neg(p)), ("O+P", None, p), ("P+O", p, None), ("equal y", p, q)]
    cases += [("O+O", None, None)] * 2
    for c in cases:
        assert c[0] != "generic" or c[1][0] != c[2][0]
    pairs = []
    for cls, p, q in cases:
        exp = g.to_bytes(P.pt_add(p, q))
        for ra in (REPRS if p is not None else IDENTITIES):
            for rb in (REPRS if q is not None else IDENTITIES):
                pairs.append(Pair(cls, ra, rb, xyzz_of(g, p, ra, rng), xyzz_of(g, q, rb, rng), q, exp))
    rng.shuffle(pairs)          # the lanes, lane pairs and slot groups of one wave then take different branches
    return g, pairs, Counter(x.cls for x in pairs)


def doublings(index, seed=0xD0B1, points=24):
    """(group, [(class, rep, xyzz, expected)]): P in the three representations, O in its two"""
    g = Group(index)
    rng = random.Random(seed + index)
    out = []
    for _ in range(points):
        p = P.pt_mul_jac(g.gen, rng.randrange(1, P.R))
        exp = g.to_bytes(P.pt_add(p, p))
        out += [("P", r, xyzz_of(g, p, r, rng), exp) for r in REPRS]
    for _ in range(4):
        out += [("O", r, xyzz_of(g, None, r, rng), g.to_bytes(None)) for r in IDENTITIES]
    rng.shuffle(out)
    return g, out


# ---- the scalar multiplication's split and recoding, restated (lagrange_derive.hip: glv_split_g1, gls_split_g2, the signed 4-bit windows)
def glv_model(k):
    """G1: k = q z^2 + t, a = t + q, b = q; 33 signed digits of a and of b from the nibbles of a + 0x88..8"""
    q, t = divmod(k, Z2)
    a, b = t + q, q
    bias = int("8" * 33, 16)
    digits = lambda v: [((v + bias) >> (4 * w) & 15) - 8 for w in range(33)]
    da, db = digits(a), digits(b)
    assert sum(d << (4 * w) for w, d in enumerate(da)) == a and sum(d << (4 * w) for w, d in enumerate(db)) == b and a + bias < 1 << 132
    return dict(q=q, t=t, a=a, da=da, db=db)


def gls_model(k):
    """G2: k = sum k_i |z|^i; 17 signed digits per sub-scalar, nibble 16 = 8 + the carry out of k_i + 0x88..8"""
    sub = []
    for _ in range(3):
        k, r = divmod(k, Z)
        sub.append(r)
    sub.append(k)
    assert all(s < 1 << 64 for s in sub)
    bias = int("8" * 16, 16)
    carry = [(s + bias) >> 64 for s in sub]
    digits = [[(((s + bias) & (2 ** 64 - 1)) >> (4 * w) & 15) - 8 for w in range(16)] + [c] for s, c in zip(sub, carry)]          # nibble 16: 8 + carry - 8
    for s, d in zip(sub, digits):
        assert sum(x << (4 * w) for w, x in enumerate(d)) == s
    return dict(sub=sub, carry=carry, digits=digits)


SMALL = [0, 1, 2, 7, 8, 9, 15, 16, 17, 0x88, 0x78]
NEAR_R = [P.R - 1, P.R - 2, (P.R - 1) // 2]


def named_scalars(index):
    """{name: scalar} with the model's word that each edge is what its name says"""
    named = {"small %#x" % k: k for k in SMALL}
    named.update({"r-1": P.R - 1, "r-2": P.R - 2, "(r-1)/2": (P.R - 1) // 2})
    if index == 0:
        qmax = (P.R - 1) // Z2
        named.update({"z^2": Z2, "z^2+1": Z2 + 1, "z^2-1": Z2 - 1, "qmax z^2": qmax * Z2, "a has bit 128": qmax * Z2 - 1, "8 z^2": 8 * Z2})
        m = {n: glv_model(k) for n, k in named.items()}
        assert m["small 0x1"]["q"] == 0 and m["z^2-1"]["q"] == 0                                  # a zero quotient
        assert m["z^2"]["t"] == 0 and m["qmax z^2"]["t"] == 0 and m["qmax z^2"]["q"] == qmax      # a zero remainder, the largest quotient
        assert m["a has bit 128"]["a"] >> 128 == 1 and m["a has bit 128"]["da"][32] == 1          # the carry into a[4]
        assert all(x["a"] >> 129 == 0 for x in m.values())
        for n in ("small 0x8", "small 0x88", "small 0x78"):
            assert -8 in m[n]["da"], n                                                            # digits of -8
        assert -8 in m["8 z^2"]["db"]                                                             # ... and among the digits of b
    else:
        for i in (1, 2, 3):
            named["|z|^%d" % i] = Z ** i
            named["|z|^%d-1" % i] = Z ** i - 1
        # Every sub-scalar equal to |z| - 1 would be the scalar z^4 - 1 > r, which no canonical scalar is.  The largest canonical one, r - 2, has
        # the sub-scalars (|z|-1, |z|-1, |z|-2, |z|-1): all four overflow the bias.  Beside it: |z| - 1 alone in each position, and in the low three.
        named["(|z|-1)(1+|z|+|z|^2)"] = (Z - 1) * (1 + Z + Z2)
        for i in range(4):
            named["(|z|-1)|z|^%d" % i] = (Z - 1) * Z ** i
            named["0x77..77 |z|^%d" % i] = 0x7777777777777777 * Z ** i
            named["0x77..78 |z|^%d" % i] = 0x7777777777777778 * Z ** i
        m = {n: gls_model(k) for n, k in named.items()}
        assert m["r-2"]["sub"] == [Z - 1, Z - 1, Z - 2, Z - 1] and m["r-2"]["carry"] == [1, 1, 1, 1]
        assert m["(|z|-1)(1+|z|+|z|^2)"]["sub"] == [Z - 1, Z - 1, Z - 1, 0]
        for i in range(4):
            one_hot = lambda s: [s if j == i else 0 for j in range(4)]
            assert m["(|z|-1)|z|^%d" % i]["sub"] == one_hot(Z - 1) and m["(|z|-1)|z|^%d" % i]["carry"][i] == 1
            assert m["0x77..77 |z|^%d" % i]["sub"] == one_hot(0x7777777777777777) and m["0x77..77 |z|^%d" % i]["carry"][i] == 0      # 0xff..ff: no carry
            assert m["0x77..78 |z|^%d" % i]["sub"] == one_hot(0x7777777777777778) and m["0x77..78 |z|^%d" % i]["carry"][i] == 1      # carry into nibble 16
            assert m["0x77..78 |z|^%d" % i]["digits"][i][:16] == [-8] * 16
        for i in (1, 2, 3):
            assert m["|z|^%d" % i]["sub"] == [1 if j == i else 0 for j in range(4)]
            assert m["|z|^%d-1" % i]["sub"] == [Z - 1 if j < i else 0 for j in range(4)]
    assert all(0 <= k < P.R for k in named.values())
    return named


def scalar_battery(index, randoms, seed=0x5CA1):
    """(group, [(name, rep, xyzz, scalar, expected)]): every named scalar and `randoms` random ones, times one point in its three representations"""
    g = Group(index)
    rng = random.Random(seed + index)
    scalars = list(named_scalars(index).items()) + [("random %d" % i, rng.randrange(P.R)) for i in range(randoms)]
    p = P.pt_mul_jac(g.gen, rng.randrange(1, P.R))
    out = []
    for name, k in scalars:
        exp = g.to_bytes(P.pt_mul_jac(p, k) if name.startswith("random") else P.pt_mul(p, k))          # pt_mul_jac: pinned to pt_mul by tests/test_oracle.py
        out += [(name, r, xyzz_of(g, p, r, rng), k, exp) for r in REPRS]
    out += [("identity", r, xyzz_of(g, None, r, rng), 5, g.to_bytes(None)) for r in IDENTITIES]
    return g, out
