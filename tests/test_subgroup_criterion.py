"""The two subgroup criteria of in_subgroup_endo (zukelang_amd/csrc/msm_points.hip) restated in Python integers, with the constants the kernel
reads (endo_consts.cuh, decoded from their Montgomery limbs), and held to [r] P = O (pyref._in_subgroup):

  G1:  P in G1  <=>  [z^2] P == (beta^2 x, -y)            G2:  Q in G2  <=>  [|z|] Q == (cx conj x, cy' conj y),  (cx, cy') = -psi as stored

on every point of tests/golden/torsion_points.json -- points of every prime-power order the cofactors allow, alone and added to a subgroup point -- and on
freshly drawn curve points.  No GPU: tests/test_gpu_subgroup_endo.py holds the kernel to the same fixture."""
import importlib.util
import json
import os
import random
import re

from oracle import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = json.load(open(os.path.join(GOLDEN, "torsion_points.json")))
CONSTS = open(os.path.join(ROOT, "zukelang_amd", "csrc", "endo_consts.cuh")).read()
Z = P.BLS_X          # |z|


def _limbs(text):
    """14 radix-2^29 Montgomery limbs (R = 2^406) -> the integer"""
    v = sum(int(w, 16) << (29 * i) for i, w in enumerate(re.findall(r"0x([0-9a-f]{8})u", text)))
    return v * pow(1 << 406, -1, P.P) % P.P


def _const_rows(name):
    body = CONSTS[CONSTS.index(name):]
    body = body[body.index("=") + 1:body.index(";")]
    return [_limbs(row) for row in re.findall(r"\{([^{}]*)\}", body)]


BETA = _const_rows("ENDO_BETA[14]")[0]
_px, _py = _const_rows("ENDO_PSI_X[3][2][14]"), _const_rows("ENDO_PSI_Y[3][2][14]")
NEG_PSI = (P.Fp2(_px[0], _px[1]), P.Fp2(_py[0], _py[1]))          # [0][c0 | c1] of each table


def in_g1_by_phi(pt):
    if pt is None:
        return True
    x, y = pt
    return P.pt_mul_jac(pt, Z * Z) == (P.Fp1(BETA * BETA % P.P * x.a), -y)


def in_g2_by_psi(pt):
    if pt is None:
        return True
    x, y = pt
    return P.pt_mul_jac(pt, Z) == (NEG_PSI[0] * x.conj(), NEG_PSI[1] * y.conj())


def _points(group):
    dec = P.g1_from_bytes if group == 0 else P.g2_from_bytes
    return [(r, dec(bytes.fromhex(r["hex"]))) for r in FIXTURE["points"] if r["group"] == group]


def test_constants_are_the_endomorphisms():
    assert pow(BETA, 3, P.P) == 1 and BETA != 1
    lam = Z * Z - 1
    assert (P.Fp1(BETA * P.G1[0].a), P.G1[1]) == P.pt_mul(P.G1, lam)                                          # phi = [z^2 - 1] on G1
    assert (NEG_PSI[0] * P.G2[0].conj(), NEG_PSI[1] * P.G2[1].conj()) == P.pt_mul(P.G2, Z)                    # the stored pair is -psi: [|z|] = [-z]


def test_fixture_holds_what_the_issue_lists():
    for group, primes in ((0, (3, 11, 10177, 859267, 52437899)), (1, (13, 23, 2713, 11953, 262069))):
        what = [r["what"] for r, _ in _points(group)]
        for ell in primes:
            assert "torsion %d" % ell in what and "torsion %d + subgroup" % ell in what
        assert what.count("random curve point") == 2 and what.count("subgroup") + what.count("generator") == 3 and what.count("identity") == 1
        b = P.B1 if group == 0 else P.B2
        for r, pt in _points(group):
            assert P.on_curve(pt, b), r["what"]
            if r["what"].startswith("torsion") and "+" not in r["what"]:          # of l-power order, and not the identity
                ell = int(r["what"].split()[1])
                assert pt is not None and P.pt_mul_jac(pt, ell * ell) is None, r["what"]
    assert sum(1 for r in FIXTURE["points"] if r["verdict"] == 4) == 24


def test_criteria_agree_with_the_order_test_on_the_fixture():
    for group, crit in ((0, in_g1_by_phi), (1, in_g2_by_psi)):
        for r, pt in _points(group):
            inside = P._in_subgroup(pt)
            assert (r["verdict"] == 0) == inside, r["what"]
            assert crit(pt) == inside, (group, r["what"])


def test_criteria_agree_on_fresh_points():
    spec = importlib.util.spec_from_file_location("make_torsion_points", os.path.join(GOLDEN, "make_torsion_points.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rnd = random.Random(0xC0FACE)
    for group, crit, h, g in ((0, in_g1_by_phi, gen.H1, P.G1), (1, in_g2_by_psi, gen.H2, P.G2)):
        for _ in range(6):
            q = gen.random_curve_point(group, rnd)
            assert crit(q) == P._in_subgroup(q)                      # a random curve point is outside, but the order test says so, not this file
            c = P.pt_mul_jac(q, h)                                   # its cofactor-cleared image is inside
            assert P._in_subgroup(c) and crit(c)
            assert crit(P.pt_add(q, P.pt_mul_jac(g, rnd.randrange(1, P.R)))) == P._in_subgroup(q)


def test_fixture_regenerates_from_its_script():
    spec = importlib.util.spec_from_file_location("make_torsion_points", os.path.join(GOLDEN, "make_torsion_points.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.build() == FIXTURE
