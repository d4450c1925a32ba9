"""Generates tests/golden/torsion_points.json: points of BLS12-381 E(Fp) and E'(Fp2) that lie ON the curve and OUTSIDE the subgroup of order r, the
inputs a subgroup check exists for, next to points inside it -- first-principles Python big integers (oracle/pyref.py), a fixed seed.

The cofactors are h1 = (z - 1)^2 / 3 and h2 = (z^8 - 4 z^7 + 5 z^6 - 4 z^4 + 6 z^3 - 4 z^2 - 4 z + 13) / 9 with z = -0xd201000000010000.  For a prime l of a
cofactor h, a point of l-power order is [r h / l^2] Q when l^2 divides h, else [r h / l] Q, for a random curve point Q; it is drawn again when that is
the identity.  ([r h / l] Q alone is almost always the identity: the l-torsion is not cyclic.)

  G1: one l-power-torsion point for every prime l of h1 (3, 11, 10177, 859267, 52437899), each of them plus a random subgroup point, two random curve
      points, three subgroup points (the generator among them), the identity;
  G2: the same over the small primes of h2 (13, 23, 2713, 11953, 262069).

Every record: group, what it is, the uncompressed encoding, and the verdict a decoder owes it (0 good, 4 outside the subgroup -- the kinds of
points_decode_verdicts), decided here by [r] P = O (pyref._in_subgroup).  The short chains of the endomorphism criteria meet special cases on these points
that a chain over a point of order r never meets: on the point of order 3 the accumulator is +-P at an addition step, on points of order 11, 13 or 23 it
passes through the identity.
Run: python tests/golden/make_torsion_points.py"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyref as P  # noqa: E402

Z = -P.BLS_X
H1 = (Z - 1) ** 2 // 3
H2 = (Z ** 8 - 4 * Z ** 7 + 5 * Z ** 6 - 4 * Z ** 4 + 6 * Z ** 3 - 4 * Z ** 2 - 4 * Z + 13) // 9
PRIMES = {0: (3, 11, 10177, 859267, 52437899), 1: (13, 23, 2713, 11953, 262069)}
COFACTOR = {0: H1, 1: H2}
SEED = 0x70125109
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torsion_points.json")


def random_curve_point(group, rnd):
    """a point of the whole curve group: x drawn until x^3 + b is a square, the sign of y drawn too"""
    while True:
        if group == 0:
            x = rnd.randrange(P.P)
            y = P.fp_sqrt(x * x * x + 4)
            if y is None:
                continue
            pt = (P.Fp1(x), P.Fp1(y))
        else:
            x = P.Fp2(rnd.randrange(P.P), rnd.randrange(P.P))
            y = P.fp2_sqrt(x * x * x + P.B2)
            if y is None:
                continue
            pt = (x, y)
        return P.pt_neg(pt) if rnd.getrandbits(1) else pt


def torsion_point(group, ell, rnd):
    h = COFACTOR[group]
    assert h % ell == 0
    k = P.R * h // (ell * ell if h % (ell * ell) == 0 else ell)
    while True:
        t = P.pt_mul_jac(random_curve_point(group, rnd), k)
        if t is not None:
            return t


def build():
    assert (Z - 1) ** 2 % 3 == 0 and H2 * 9 == Z ** 8 - 4 * Z ** 7 + 5 * Z ** 6 - 4 * Z ** 4 + 6 * Z ** 3 - 4 * Z ** 2 - 4 * Z + 13
    rnd = random.Random(SEED)
    out = []
    for group in (0, 1):
        gen = P.G1 if group == 0 else P.G2
        enc = P.g1_to_bytes if group == 0 else P.g2_to_bytes
        b = P.B1 if group == 0 else P.B2
        sub = lambda: P.pt_mul_jac(gen, rnd.randrange(1, P.R))
        pts = []
        for ell in PRIMES[group]:
            t = torsion_point(group, ell, rnd)
            pts.append(("torsion %d" % ell, t))
            pts.append(("torsion %d + subgroup" % ell, P.pt_add(t, sub())))
        pts += [("random curve point", random_curve_point(group, rnd)) for _ in range(2)]
        pts += [("generator", gen), ("subgroup", sub()), ("subgroup", sub()), ("identity", None)]
        for what, pt in pts:
            assert P.on_curve(pt, b), what
            out.append({"group": group, "what": what, "hex": enc(pt).hex(), "verdict": 0 if P._in_subgroup(pt) else 4})
    # what the names promise
    for rec in out:
        inside = rec["what"] in ("generator", "subgroup", "identity")
        assert (rec["verdict"] == 0) == inside, rec["what"]
    return {"how": "python tests/golden/make_torsion_points.py (first-principles Python big integers, oracle/pyref.py)", "seed": hex(SEED), "points": out}


def main():
    doc = build()
    with open(PATH, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote torsion_points.json:", len(doc["points"]), "points,", sum(1 for r in doc["points"] if r["verdict"]), "outside the subgroup")


if __name__ == "__main__":
    main()
