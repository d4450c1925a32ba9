"""k_subgroup_verdict (csrc/msm_points.hip) through zk_selftest_subgroup: the subgroup verdict by endomorphism (method 1) against [r] P = O on the
device (method 0) and against the verdicts tests/golden/torsion_points.json records from Python integers -- points of every prime-power order the
cofactors allow, where the short chains meet P + P, P - P and an identity accumulator (orders 3, 11, 13, 23), those points added to subgroup points,
random curve points, subgroup points and the identity."""
import ctypes as C
import json
import os

import pytest

from oracle import pyref as P
from zukelang_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_points.json")))["points"]
SIZE = {0: 96, 1: 192}


def verdicts(group, method, points):
    n = len(points)
    out = (C.c_uint8 * n)(*([9] * n))
    raw = b"".join(points)
    assert len(raw) == SIZE[group] * n
    _lib.check(_lib.lib().zk_selftest_subgroup(group, method, C.cast(C.c_char_p(raw), _lib._P8), n, C.cast(out, _lib._P8)))
    return list(out)


def fixture(group):
    recs = [r for r in FIXTURE if r["group"] == group]
    return [bytes.fromhex(r["hex"]) for r in recs], [r["verdict"] for r in recs], [r["what"] for r in recs]


@pytest.mark.parametrize("group", [0, 1])
def test_whole_fixture_both_methods(group):
    pts, want, what = fixture(group)
    assert len(pts) == 16 and want.count(4) == 12
    assert verdicts(group, 0, pts) == want, what
    assert verdicts(group, 1, pts) == want, what


@pytest.mark.parametrize("group", [0, 1])
def test_one_point_per_call(group):
    pts, want, what = fixture(group)
    for p, w, name in zip(pts, want, what):
        assert verdicts(group, 1, [p]) == [w], name
    assert verdicts(group, 0, [pts[0]]) == [want[0]]


@pytest.mark.parametrize("group", [0, 1])
def test_one_lane_past_a_full_block(group):
    pts, want, _ = fixture(group)
    idx = [(7 * i + 3) % len(pts) for i in range(129)]          # 129 = 128 + 1: the last point sits alone in the second block
    idx[128] = 0                                                  # ... and is a torsion point, outside the subgroup
    many, exp = [pts[i] for i in idx], [want[i] for i in idx]
    assert exp[128] == 4
    assert verdicts(group, 1, many) == exp
    assert verdicts(group, 0, many) == exp


@pytest.mark.parametrize("group", [0, 1])
def test_other_verdicts_pass_through(group):
    pts, want, _ = fixture(group)
    good = pts[want.index(0)]
    flagged = bytes([good[0] | 0x80]) + good[1:]                                 # compression flag on an uncompressed string: bad encoding
    big = (P.P).to_bytes(48, "big") + good[48:]                                  # a coordinate equal to p: bad encoding
    off = bytearray(good); off[-1] ^= 1                                          # y changed: not on the curve
    zero = bytes(SIZE[group])                                                    # (0, 0) without the infinity bit: not on the curve
    mix = [pts[0], flagged, good, bytes(off), pts[1], big, zero, pts[-1]]
    exp = [want[0], 2, 0, 1, want[1], 2, 1, want[-1]]
    assert verdicts(group, 1, mix) == exp
    assert verdicts(group, 0, mix) == exp
