"""The column sums of zk_groth16_pk_specialize on bare points (zk_selftest_g1_colsum) against the oracle's naive fold, column by column.

out[k] = sum_e coef[e] * pts[row[e]] over the entries of column k, through the call's own stages: the split by coefficient class (0 dropped, 1 and
r - 1 unit, the rest multiplied in one compacted launch), chunks of C = 16 operands per lane, and as many levels as the longest column needs.  Every
case below is a column (or a family of columns) with a property the stages can get wrong; what is expected is O.g1_msm_naive on the column's own
points and coefficients, computed once per battery."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
from oracle import pyref as P
from zukelang_amd import _lib

pytestmark = pytest.mark.gpu

R = P.R
CH = 16          # csrc/specialize.hip: COLSUM_C
IDENT = P.g1_to_bytes(None)
ARG, NOT_ON_CURVE, SCALAR_RANGE = -1, -2, -3


@pytest.fixture(autouse=True)
def _init():
    _lib.check(_lib.lib().zk_init(0))


@functools.lru_cache(maxsize=None)
def battery():
    """300 points: random subgroup points; the identity (both encodings) first, in the middle and last; P and -P side by side; the generator"""
    st = P.fr_stream(0x5EED5C01)
    g = O.g1_generator()
    pts = [O.g1_mul(g, P.fr_to_bytes(next(st))) for _ in range(300)]
    pts[0] = pts[299] = IDENT
    pts[150] = bytes(96)
    pts[64] = P.g1_to_bytes(P.pt_neg(P.g1_from_bytes(pts[63])))
    pts[127] = g
    return pts


def colsum_rc(pts, cols):
    """cols: per column a list of (row, coefficient as an integer, possibly >= r).  Returns (status, m * 96 bytes)."""
    ptr, row, coef = [0], [], b""
    for col in cols:
        for r_, c in col:
            row.append(r_)
            coef += int(c).to_bytes(32, "little")
        ptr.append(len(row))
    a = np.frombuffer(b"".join(pts), dtype=np.uint8)
    ptr = np.array(ptr, dtype=np.uint32)
    row = np.array(row if row else [0], dtype=np.uint32)
    coef = np.frombuffer(coef if coef else bytes(32), dtype=np.uint8)
    out = np.full(96 * len(cols), 0x5A, dtype=np.uint8)
    p8 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint8))
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = _lib.lib().zk_selftest_g1_colsum(p8(a), len(pts), p32(ptr), p32(row), p8(coef), len(cols), p8(out))
    return rc, bytes(out)


def colsum(pts, cols):
    rc, out = colsum_rc(pts, cols)
    _lib.check(rc)
    return [out[96 * k:96 * k + 96] for k in range(len(cols))]


def fold(pts, col):
    """the oracle's sum of one column; the identity in the library's encoding"""
    if not col:
        return IDENT
    bases = b"".join(IDENT if pts[r_] == bytes(96) else pts[r_] for r_, _ in col)
    rc, out = O.g1_msm_naive(bases, b"".join(P.fr_to_bytes(c % R) for _, c in col))
    assert rc == 0
    return out


def held(pts, cols, tag):
    got = colsum(pts, cols)
    bad = [k for k, col in enumerate(cols) if got[k] != fold(pts, col)]
    assert not bad, (tag, bad[:8])


RND = [next(P.fr_stream(0x5EED5C02 + i)) | (1 << 254) for i in range(4)]          # 255-bit
RND = [x % R if x >= R else x for x in RND]


def test_single_columns_of_every_coefficient_class():
    pts = battery()
    cols = [[]]                                                                    # empty: the identity
    cols += [[(7, c)] for c in (0, 1, R - 1, 2, RND[0], RND[1])]                   # one entry
    cols += [[(0, c)] for c in (1, R - 1, RND[0])]                                 # one entry, on the identity
    cols += [[(150, 1), (299, 2), (0, R - 1)]]                                     # identities only
    cols += [[(7, 1), (7, 1)], [(7, R - 1), (7, R - 1)], [(7, 2), (7, 2)], [(7, 1), (7, 2)]]          # the same row twice: doublings
    cols += [[(7, RND[2]), (7, R - RND[2])], [(7, 1), (7, R - 1)], [(63, 1), (64, 1)], [(63, 2), (64, 2)]]          # back to the identity
    cols += [[(7, RND[2]), (7, R - RND[2]), (9, 1), (10, RND[3])], [(7, 1), (7, R - 1), (9, 2), (9, R - 2), (11, R - 1)]]          # ... and on from there
    cols += [[(5, 0), (6, 0)], [(5, 0), (6, 1), (8, 0)]]                           # zeros dropped: an empty column after all, one entry after all
    held(pts, cols, "classes")
    assert colsum(pts, [[]]) == [IDENT]
    assert colsum(pts, [[(7, 1)]]) == [pts[7]]


def _column(length, kind, seed):
    """`length` entries over the battery's rows (rows repeat from 300 entries on)"""
    st = P.fr_stream(seed)
    col = []
    for i in range(length):
        r_ = next(st) % 300
        c = {"unit": (1, R - 1)[i & 1], "general": next(st) % R or 2, "mixed": (1, next(st) % R or 2, R - 1, 2, 0)[next(st) % 5]}[kind]
        col.append((r_, c))
    return col


@pytest.mark.parametrize("kind", ["unit", "general", "mixed"])
def test_column_lengths_around_the_chunk_and_two_and_three_levels(kind):
    """C - 1, C, C + 1: one chunk, one full chunk, two chunks and a second level; 2 C; C^2 + 1: 17 partials, which are two chunks again -- three levels"""
    pts = battery()
    lengths = [CH - 1, CH, CH + 1, 2 * CH, CH * CH + 1]
    cols = [_column(n, kind, 0x5EED5D00 + n) for n in lengths]
    held(pts, cols, kind)
    for col in cols:          # each alone (m = 1: the level loop ends on this column's own length) gives the same point
        assert colsum(pts, [col]) == [fold(pts, col)]


def test_two_hundred_columns_of_unequal_lengths():
    """m = 200: empty columns between long ones, a lane's chunk never depends on its neighbours' lengths"""
    pts = battery()
    st = P.fr_stream(0x5EED5E00)
    lengths = [(0, 1, 3, CH, CH + 1, 40, 2, 0, 5 * CH, 7)[next(st) % 10] for _ in range(200)]
    lengths[0], lengths[199], lengths[100] = 0, CH * CH + 1, 0
    cols = [_column(n, "mixed", 0x5EED5F00 + k) for k, n in enumerate(lengths)]
    held(pts, cols, "m200")


def test_the_hook_refuses_before_the_device_and_points_that_are_not_points():
    pts = battery()[1:9]
    assert colsum_rc(pts, [[(8, 1)]])[0] == ARG                      # row out of range
    assert colsum_rc(pts, [[(1, R)]])[0] == SCALAR_RANGE             # coefficient >= r
    rc, out = colsum_rc(pts, [[(1, R)]])
    assert out == b"\x5a" * 96                                       # a refused call writes nothing
    off = bytearray(pts[1]); off[95] ^= 1
    assert colsum_rc([pts[0], bytes(off)], [[(0, 1)]])[0] == NOT_ON_CURVE
    big = b"\xff" * 48 + pts[1][48:]
    assert colsum_rc([pts[0], big], [[(0, 1)]])[0] == ARG
