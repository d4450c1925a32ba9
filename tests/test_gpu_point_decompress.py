"""zk_selftest_point_decompress -- the two launches a resident key's compressed slab front makes per group, k_decompress_verdict and then
k_subgroup_verdict by endomorphism (csrc/msm_points.hip) -- against oracle/pyref.py: g1_decompress / g2_decompress for the verdicts, fp_sqrt / fp2_sqrt
and the sign rule for the bytes.  One list per group holds every shape the decoder tells apart: oracle points under both sign bits, the identity and
the identity with a sign bit, a cleared compression bit, x = p and x = p - 1, an abscissa whose right-hand side is no square, the torsion points of
tests/golden/torsion_points.json (verdict 4, and still the oracle's root), and in G2 right-hand sides with imaginary part 0 (a real and an imaginary
root) and right-hand sides that take the second branch of the device's root (chi = -1).  The list is cut to n = 1, 127, 128 and 129 points: the
launch's block is 128 lanes."""
import ctypes as C
import functools
import json
import os

import pytest

from oracle import pyref as P
from zukelang_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORSION = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_points.json")))["points"]
VERDICT = {P.OK: 0, P.NOT_ON_CURVE: 1, P.BAD_ENCODING: 2, P.NOT_IN_SUBGROUP: 4}
Pm = P.P
be = lambda v: int(v).to_bytes(48, "big")


def hook(group, strings):
    n, cb = len(strings), 96 if group else 48
    out, verdict = C.create_string_buffer(2 * cb * n), C.create_string_buffer(n)
    rc = _lib.lib().zk_selftest_point_decompress(group, C.cast(C.c_char_p(b"".join(strings)), _lib._P8), n, C.cast(out, _lib._P8), C.cast(verdict, _lib._P8))
    assert rc == 0, _lib.lib().zk_last_error()
    return [out.raw[2 * cb * i:2 * cb * (i + 1)] for i in range(n)], list(verdict.raw)


def g2_x_bytes(x, sign=False):
    b = bytearray(be(x.b) + be(x.a))
    b[0] |= 0x80 | (0x20 if sign else 0)
    return bytes(b)


def oracle(group, s):
    """(verdict, bytes) of one compressed string from pyref alone.  pyref's decoders give the verdict; they return no point outside the subgroup, so the
    bytes are rebuilt from the same pieces: the larger root of fp_sqrt / fp2_sqrt, negated when the sign bit is clear."""
    v, pt = (P.g2_decompress if group else P.g1_decompress)(s)
    if v in (P.BAD_ENCODING, P.NOT_ON_CURVE):
        return VERDICT[v], bytes(192 if group else 96)
    if v == P.OK:
        return 0, (P.g2_to_bytes if group else P.g1_to_bytes)(pt)
    sign = bool(s[0] & 0x20)
    if group:
        x = P.Fp2(int.from_bytes(s[48:], "big"), int.from_bytes(bytes([s[0] & 0x1F]) + s[1:48], "big"))
        y = P.fp2_sqrt(x * x * x + P.B2)
        return 4, P.g2_to_bytes((x, y if sign else -y))
    x = int.from_bytes(bytes([s[0] & 0x1F]) + s[1:], "big")
    y = P.fp_sqrt(x * x * x + 4)
    return 4, P.g1_to_bytes((P.Fp1(x), P.Fp1(y if sign else (Pm - y) % Pm)))


def torsion_strings(group):
    out = []
    for r in TORSION:
        if r["group"] != group:
            continue
        raw = bytes.fromhex(r["hex"])
        if raw[0] & 0x40:
            continue
        out.append((P.g2_compress(P.g2_from_bytes(raw)) if group else P.g1_compress(P.g1_from_bytes(raw)), r["what"]))
    return out


def non_residue_abscissa(group):
    x = 0
    while True:
        x += 1
        s = g2_x_bytes(P.Fp2(x, 1)) if group else bytes([0x80]) + x.to_bytes(47, "big")
        if (P.g2_decompress if group else P.g1_decompress)(s)[0] == P.NOT_ON_CURVE:
            return s


def euler(v):
    return pow(v % Pm, (Pm - 1) // 2, Pm)


def real_rhs_abscissae():
    """G2 abscissae x = x0 + x1 u whose x^3 + 4 + 4u has imaginary part 0: 3 x0^2 x1 - x1^3 + 4 = 0, so x0^2 = (x1^3 - 4) / (3 x1).  Every such x is on
    the curve: a real right-hand side is a square of Fp2 whatever its character in Fp.  -> [(string, 'real' | 'imaginary')]: the kind of its root."""
    got, x1 = {"real": [], "imaginary": []}, 1
    while min(len(v) for v in got.values()) < 2:
        x1 += 1
        x0 = P.fp_sqrt((x1 ** 3 - 4) * pow(3 * x1, -1, Pm) % Pm)
        if x0 is None:
            continue
        x = P.Fp2(x0, x1)
        rhs = x * x * x + P.B2
        assert rhs.b == 0 and rhs.a != 0
        kind = "real" if euler(rhs.a) == 1 else "imaginary"
        if len(got[kind]) < 2:
            got[kind].append(g2_x_bytes(x, sign=len(got[kind]) == 1))
    return [(s, kind) for kind, ss in got.items() for s in ss]


def chi_of_rhs(a):
    """The branch the device's root takes on a = a0 + a1 u, a1 != 0 (csrc/msm_points.hip: fp2_sqrt_dev): s = n^((p + 1) / 4) for the norm n, t = (a0 + s) / 2,
    chi = t^((p - 1) / 2).  None: a is no square."""
    n = (a.a * a.a + a.b * a.b) % Pm
    s = pow(n, (Pm + 1) // 4, Pm)
    if s * s % Pm != n:
        return None
    return euler((a.a + s) * pow(2, -1, Pm))


def chi_abscissae():
    """G2 abscissae on the curve, imaginary part of the right-hand side non-zero, at least two of each branch of the root: chi = 1 and chi = p - 1"""
    got, x0 = {1: [], Pm - 1: []}, 0
    while min(len(v) for v in got.values()) < 2:
        x0 += 1
        x = P.Fp2(x0, 2)
        rhs = x * x * x + P.B2
        c = chi_of_rhs(rhs)
        if rhs.b == 0 or c is None or len(got[c]) >= 2:
            continue
        got[c].append(g2_x_bytes(x, sign=len(got[c]) == 1))
    return got


@functools.lru_cache(maxsize=None)
def cases(group):
    """The group's list, 129 strings, with what pyref says about each: [(string, verdict, bytes, label)].  Computed once."""
    cb = 96 if group else 48
    gen = P.G2 if group else P.G1
    comp = P.g2_compress if group else P.g1_compress
    special = []
    special.append((bytes([0xC0]) + bytes(cb - 1), "identity"))
    special.append((bytes([0xE0]) + bytes(cb - 1), "identity with the sign bit"))
    good = comp(P.pt_mul(gen, 5))
    special.append((bytes([good[0] & 0x7F]) + good[1:], "compression bit cleared"))
    xp = bytearray(be(Pm) + (bytes(48) if group else b"")); xp[0] |= 0x80
    special.append((bytes(xp), "x = p"))
    xm = bytearray((be(0) + be(Pm - 1)) if group else be(Pm - 1)); xm[0] |= 0x80
    special.append((bytes(xm), "x = p - 1"))
    if group:
        x1p = bytearray(be(Pm - 1) + be(Pm)); x1p[0] |= 0x80
        special.append((bytes(x1p), "x0 = p under x1 = p - 1"))
    special.append((non_residue_abscissa(group), "right-hand side no square"))
    special += torsion_strings(group)
    if group:
        special += [(s, "real right-hand side, %s root" % k) for s, k in real_rhs_abscissae()]
        special += [(s, "chi = %s" % ("1" if c == 1 else "-1")) for c, ss in chi_abscissae().items() for s in ss]
    # oracle points under both sign bits: k G and -k G; the specials spread among them so that every cut of the list holds some
    pts, acc = [], None
    while len(pts) + len(special) < 129:
        acc = P.pt_add(acc, gen)
        pts.append((comp(acc), "k G"))
        pts.append((comp(P.pt_neg(acc)), "-k G"))
    rows = pts[:1]
    rest, sp = pts[1:], list(special)
    while rest or sp:
        if sp:
            rows.append(sp.pop(0))
        if rest:
            rows.append(rest.pop(0))
    rows = rows[:129]
    assert len(rows) == 129
    return [(s,) + oracle(group, s) + (label,) for s, label in rows]


@pytest.mark.parametrize("group", [0, 1])
def test_the_lists_hold_every_case_the_decoder_tells_apart(group):
    """pyref alone: all four verdicts, both sign bits on good points, and -- G2 -- both kinds of root of a real right-hand side and both branches chi."""
    rows = cases(group)
    assert {v for _, v, _, _ in rows} == {0, 1, 2, 4}
    assert {bool(s[0] & 0x20) for s, v, _, lab in rows if v == 0 and lab.endswith("k G")} == {True, False}
    assert sum(1 for _, v, _, _ in rows if v == 4) >= 4
    labels = [lab for _, _, _, lab in rows]
    rows_by = {lab: v for _, v, _, lab in rows}
    assert rows_by["identity"] == 0 and rows_by["identity with the sign bit"] == 2
    assert rows_by["compression bit cleared"] == 2 and rows_by["x = p"] == 2 and rows_by["right-hand side no square"] == 1
    assert rows_by["x = p - 1"] in (0, 1, 4)                     # a canonical coordinate: whatever the curve says, not an encoding error
    if group:
        assert "real right-hand side, real root" in labels and "real right-hand side, imaginary root" in labels
        for s, v, pt, lab in rows:
            if lab.startswith("real right-hand side"):
                y = P.g2_from_bytes(pt)[1]
                assert v in (0, 4) and ((y.b == 0) if lab.endswith("real root") else (y.a == 0 and y.b != 0)), lab
        assert labels.count("chi = 1") >= 1 and labels.count("chi = -1") >= 1
        for s, v, pt, lab in rows:
            if lab.startswith("chi"):
                x = P.g2_from_bytes(pt)[0]
                assert v in (0, 4) and chi_of_rhs(x * x * x + P.B2) == (1 if lab == "chi = 1" else Pm - 1)


@pytest.mark.parametrize("n", [1, 127, 128, 129])
@pytest.mark.parametrize("group", [0, 1])
def test_point_decompress_equals_the_oracle(group, n):
    _lib.check(_lib.lib().zk_init(0))
    rows = cases(group)[:n]
    pts, verdicts = hook(group, [s for s, _, _, _ in rows])
    wrong = [(lab, s.hex(), v, got_v) for (s, v, _, lab), got_v in zip(rows, verdicts) if v != got_v]
    assert not wrong, wrong[:4]
    wrong = [(lab, s.hex()) for (s, _, want, lab), got in zip(rows, pts) if want != got]
    assert not wrong, wrong[:4]


def test_the_hook_refuses_what_it_cannot_run():
    lib = _lib.lib()
    s = C.cast(C.c_char_p(bytes([0xC0]) + bytes(95)), _lib._P8)
    out, v = C.cast(C.create_string_buffer(192), _lib._P8), C.cast(C.create_string_buffer(1), _lib._P8)
    for args in ((0, None, 1, out, v), (0, s, 1, None, v), (0, s, 1, out, None), (0, s, 0, out, v), (2, s, 1, out, v), (-1, s, 1, out, v)):
        assert lib.zk_selftest_point_decompress(*args) == -1
