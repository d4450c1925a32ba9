"""GPU parity of zk_fr_spmv, the public sparse product of its own: y[g] = sum_e val[e] * x[col[e]] over row g against the integer sum, row by row --
row counts around the 256-thread block, empty rows (first, last, a run), one-entry rows, a row of 2000 entries, a column named several times in one
row, coefficients 0, 1, r - 1, rows whose terms add up to exactly r and to 0, the all-zero matrix, the transposed matrix (the shape key generation
multiplies), and every refusal the header documents."""
import ctypes as C
import random

import numpy as np
import pytest

from zukelang_amd import _lib
from zukelang_amd.groth16 import _csr, _p
from zukelang_amd.r1cs import FR_MODULUS as r, Matrix, fr_bytes, fr_ints

pytestmark = pytest.mark.gpu
ZK_ERR_ARG, ZK_ERR_SCALAR_RANGE = -1, -3
LONG = 2000


def spmv(rows, cols, M, x, status=False):
    """M: Matrix | a ready _lib.CSR; x: uint8 array of cols * 32 bytes"""
    y = np.full(32 * rows, 0xA5, dtype=np.uint8)
    csr = M if isinstance(M, _lib.CSR) else _csr(M)
    rc = _lib.lib().zk_fr_spmv(C.c_uint32(rows), C.c_uint32(cols), C.byref(csr), _p(x), _p(y))
    if status:
        return rc
    _lib.check(rc)
    return fr_ints(y)


def reference(rows, ptr, col, val, x):
    return [sum(val[e] * x[col[e]] for e in range(ptr[g], ptr[g + 1])) % r for g in range(rows)]


def as_matrix(ptr, col, val):
    return Matrix(np.array(ptr, dtype=np.uint32), np.array(col, dtype=np.uint32), fr_bytes(val) if val else np.zeros(0, dtype=np.uint8))


def vector(cols, rnd):
    x = [rnd.randrange(1, r) for _ in range(cols)]
    for k, v in ((1, 0), (2, 1), (3, r - 1)):
        if k < cols:
            x[k] = v
    return x


def special_rows(cols, x, rnd):
    """{kind: [(column, coefficient)]} -- the row shapes and values the kernel can get wrong"""
    c0 = 0                                          # x[0] is never zero
    pick = lambda: rnd.choice([0, 1, r - 1, rnd.randrange(r), rnd.randrange(r)])
    a = rnd.randrange(1, r)
    kinds = {
        "empty": [],
        "one entry": [(rnd.randrange(cols), rnd.randrange(1, r))],
        "one entry, r - 1": [(cols - 1, r - 1)],
        "one entry, 1": [(c0, 1)],
        "one entry, 0": [(c0, 0)],
        "long": [(rnd.randrange(cols), pick()) for _ in range(LONG)],
        "long, all r - 1": [(c0, r - 1)] * LONG,
        "same column several times": [(c0, rnd.randrange(r)) for _ in range(5)] + [(cols - 1, 1), (c0, r - 1), (cols - 1, 1)],
        "terms sum to exactly r": [(c0, a), (c0, r - a)],                      # a x0 mod r + (r - a) x0 mod r = r as integers, x0 != 0
        "terms sum to 0": [(c0, 0), (cols - 1, 0), (c0, 0)],
    }
    t = [v * x[c] % r for c, v in kinds["terms sum to exactly r"]]
    assert sum(t) == r and all(t)
    return kinds


def build(rows, cols, seed):
    """(ptr, col, val ints, x ints, {kind: row index}) with every special row placed while rows last; the rest random short rows"""
    rnd = random.Random(seed)
    x = vector(cols, rnd)
    kinds = special_rows(cols, x, rnd)
    empty = {0, rows - 1} | set(range(100, 120)) if rows >= 255 else {0, rows - 1} if rows >= 16 else set()
    placed, ptr, col, val = {}, [0], [], []
    todo = [k for k in kinds if k != "empty"] + ([] if empty else ["empty"])
    for g in range(rows):
        if g in empty:
            row, kind = [], "empty"
        elif todo and (rows < 16 or g % 3 == 1):
            kind = todo.pop(0)
            row = kinds[kind]
        else:
            kind, row = None, [(rnd.randrange(cols), rnd.choice([1, r - 1, rnd.randrange(r)])) for _ in range(rnd.randrange(0, 6))]
        if kind:
            placed.setdefault(kind, g)
        for c, v in row:
            col.append(c)
            val.append(v)
        ptr.append(len(col))
    return ptr, col, val, x, placed, [k for k in kinds if k not in placed]


@pytest.mark.parametrize("cols", [1, 7, 300])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_spmv_matches_the_integer_sum_row_by_row(rows, cols):
    seed = 0x5B3 + 1000 * rows + cols
    ptr, col, val, x, placed, missing = build(rows, cols, seed)
    if rows >= 255:
        assert not missing and ptr[1] == 0 and ptr[-1] == ptr[-2] and ptr[100] == ptr[120], (placed, missing)
    M = as_matrix(ptr, col, val)
    got = spmv(rows, cols, M, fr_bytes(x))
    ref = reference(rows, ptr, col, val, x)
    for g in range(rows):
        assert got[g] == ref[g], (g, [k for k, i in placed.items() if i == g])
    if "terms sum to exactly r" in placed:
        assert ref[placed["terms sum to exactly r"]] == 0 and ref[placed["terms sum to 0"]] == 0
    # the transposed matrix, the shape of key generation: cols rows over a vector of `rows` elements
    T = M.transposed(cols)
    z = vector(rows, random.Random(seed + 1))
    tptr, tcol = [int(v) for v in T.ptr], [int(v) for v in T.col]
    assert spmv(cols, rows, T, fr_bytes(z)) == reference(cols, tptr, tcol, fr_ints(T.val), z)
    if rows == 1:
        # a matrix of one row holds one special row at a time: the others, each as a matrix of its own
        rnd = random.Random(seed + 2)
        for kind, row in special_rows(cols, x, rnd).items():
            p, c, v = [0, len(row)], [e[0] for e in row], [e[1] for e in row]
            assert spmv(1, cols, as_matrix(p, c, v), fr_bytes(x)) == reference(1, p, c, v, x), kind


def test_the_all_zero_matrix_with_no_entries():
    x = fr_bytes([5, r - 1, 0])
    for rows in (1, 257):
        M = as_matrix([0] * (rows + 1), [], [])
        assert spmv(rows, 3, M, x) == [0] * rows
        bare = _lib.CSR()                     # no col / val arrays at all: nothing is read from them
        bare.row_ptr = M.ptr.ctypes.data_as(C.POINTER(C.c_uint32))
        assert spmv(rows, 3, bare, x) == [0] * rows


def test_refusals_are_the_ones_the_header_documents():
    rnd = random.Random(0x5B4)
    rows, cols = 4, 3
    ptr, col = [0, 2, 2, 3, 5], [0, 2, 1, 0, 1]
    val = [rnd.randrange(r) for _ in col]
    x = [rnd.randrange(r) for _ in range(cols)]
    xb = fr_bytes(x)
    good = as_matrix(ptr, col, val)
    assert spmv(rows, cols, good, xb) == reference(rows, ptr, col, val, x)
    # ZK_ERR_ARG: a malformed matrix (row_ptr not monotone, column >= cols), nothing to do, a null pointer
    assert spmv(rows, cols, as_matrix([0, 2, 1, 3, 5], col, val), xb, status=True) == ZK_ERR_ARG
    assert spmv(rows, cols, as_matrix([0, 2, 2, 5, 3], col, val), xb, status=True) == ZK_ERR_ARG
    assert spmv(rows, cols, as_matrix(ptr, [0, 2, 1, 0, cols], val), xb, status=True) == ZK_ERR_ARG
    assert spmv(rows, cols, as_matrix(ptr, [cols, 2, 1, 0, 1], val), xb, status=True) == ZK_ERR_ARG
    assert spmv(rows, cols, as_matrix(ptr, [0, 2, 0xFFFFFFFF, 0, 1], val), xb, status=True) == ZK_ERR_ARG
    y = np.zeros(32 * rows, dtype=np.uint8)
    call = _lib.lib().zk_fr_spmv
    csr = _csr(good)
    assert call(C.c_uint32(0), C.c_uint32(cols), C.byref(csr), _p(xb), _p(y)) == ZK_ERR_ARG
    assert call(C.c_uint32(rows), C.c_uint32(0), C.byref(csr), _p(xb), _p(y)) == ZK_ERR_ARG
    assert call(C.c_uint32(rows), C.c_uint32(cols), None, _p(xb), _p(y)) == ZK_ERR_ARG
    assert call(C.c_uint32(rows), C.c_uint32(cols), C.byref(csr), None, _p(y)) == ZK_ERR_ARG
    assert call(C.c_uint32(rows), C.c_uint32(cols), C.byref(csr), _p(xb), None) == ZK_ERR_ARG
    for field in ("row_ptr", "col", "val"):
        broken = _csr(good)
        setattr(broken, field, None)
        assert call(C.c_uint32(rows), C.c_uint32(cols), C.byref(broken), _p(xb), _p(y)) == ZK_ERR_ARG, field
    # row_ptr[0] != 0 is not among the header's refusals: the rows are what row_ptr says, y[g] = the sum over row_ptr[g] .. row_ptr[g + 1]
    shifted = [1, 2, 2, 3, 5]
    assert spmv(rows, cols, as_matrix(shifted, col, val), xb) == reference(rows, shifted, col, val, x)
    # ZK_ERR_SCALAR_RANGE: a coefficient = r, a vector element = r (fr_bytes reduces: write the bytes)
    rb = np.frombuffer(int(r).to_bytes(32, "little"), dtype=np.uint8)
    for e in (0, len(col) - 1):
        bad = as_matrix(ptr, col, val)
        bad.val[32 * e:32 * e + 32] = rb
        assert spmv(rows, cols, bad, xb, status=True) == ZK_ERR_SCALAR_RANGE, e
    for k in (0, cols - 1):
        bad = xb.copy()
        bad[32 * k:32 * k + 32] = rb
        assert spmv(rows, cols, good, bad, status=True) == ZK_ERR_SCALAR_RANGE, k
    bad = as_matrix(ptr, col, val)
    bad.val[:32] = 0xFF                       # 2^256 - 1
    assert spmv(rows, cols, bad, xb, status=True) == ZK_ERR_SCALAR_RANGE
    assert spmv(rows, cols, good, xb) == reference(rows, ptr, col, val, x)          # and the library goes on working
