"""Circuits and strings the specialisation tests share (tests/test_specialize_model.py on the CPU, tests/test_gpu_specialize*.py on the GPU) -- helpers
only.  What is expected of the device never comes from the library under test: strings are [exponent] G through the oracle's point multiplication,
keys the oracle's setup for the trapdoor (alpha, beta, 1, 1, tau), crafted strings the integer model of tests/specialize_model.py."""
import functools

import numpy as np

import oracle_lib as O
import specialize_model as SM
from oracle import pyref as P
from zukelang_amd import r1cs as RC
from zukelang_amd.groth16 import SRS

R = RC.FR_MODULUS
ALPHA, BETA, TAU = (0x5EC1A11 + 7919 * i + (i << 201) for i in range(1, 4))
frs = lambda xs: b"".join(P.fr_to_bytes(x % R) for x in xs)
csrs = lambda cs: [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]


def _cut_rows(M, n):
    e = int(M.ptr[n])
    return RC.Matrix(M.ptr[:n + 1].copy(), M.col[:e].copy(), M.val[:32 * e].copy())


def cubic(n, x=0xC0B1C):
    """RC.iterated_cubic cut to its first n gates (the family itself has an even number of them): same variables, the ones of the dropped gate stay
    behind as a variable of fewer rows; n = 1 is the lone gate t_0 = u_0 * u_0 with two variables that occur in no row"""
    full, w = RC.iterated_cubic(n + (n & 1), x)
    if n == full.n:
        return full, w
    cs = RC.R1CS(n, full.m, _cut_rows(full.L, n), _cut_rows(full.R, n), _cut_rows(full.O, n), full.mid)
    assert cs.check(w)
    return cs, w


def matrix(rows):
    """rows of [(column, coefficient), ...] in the order given: a (row, column) pair may repeat, which RC.Matrix.from_rows cannot say"""
    ptr, col, val = [0], [], []
    for row in rows:
        for k, c in row:
            col.append(k)
            val.append(c % R)
        ptr.append(len(col))
    return RC.Matrix(np.array(ptr, dtype=np.uint32), np.array(col, dtype=np.uint32), RC.fr_bytes(val))


def handbuilt():
    """5 gates, 7 variables: gate 1 is an all-zero row in all three matrices; variable 6 (a mid) occurs in no row; L holds (gate 2, variable 3) twice
    (2 and r - 2: the pair sums to zero) and (gate 3, variable 1) twice (1 and 1); the coefficients are 0 (stored), 1, r - 1, 2 and full-width ones.
    No witness: a key is a function of the matrices alone."""
    big = next(P.fr_stream(0x5EC1A112))
    L = matrix([[(3, 1)], [], [(3, 2), (0, 3), (3, R - 2), (2, 0)], [(1, 1), (1, 1), (4, big)], [(2, R - 1), (5, 1)]])
    Rm = matrix([[(3, 1)], [], [(0, 1)], [(0, R - 1), (4, 0)], [(5, big + 1), (0, 2)]])
    Om = matrix([[(1, 1)], [], [(4, 1)], [(2, 1), (2, R - 1)], [(5, 2), (1, R - 1)]])
    return RC.R1CS(5, 7, L, Rm, Om, np.array([0, 1, 1, 1, 0, 0, 1], dtype=np.uint8)), None


_MAKERS = {"readme": lambda: RC.readme_circuit(3), "handbuilt": handbuilt,
           # 8 entries per row, m < n: the column of `one` and others meet far more than one chunk of rows
           "random256": lambda: RC.random_r1cs(256, 200, 0x5EC256, nnz=(8, 8))}


@functools.lru_cache(maxsize=None)
def circuit(name):
    if name.startswith("cubic"):
        cs, w = cubic(int(name[5:]))
    else:
        cs, w = _MAKERS[name]()
    if name == "random256":          # the column of `one` is longer than a chunk of the summing kernel (16): its sum takes a second level
        assert sum(int(np.count_nonzero(M.col == 0)) for M in (cs.L, cs.R, cs.O)) > 16
    return cs, (None if w is None else [int(x) % R for x in w])


def toxic(alpha=ALPHA, beta=BETA, tau=TAU, delta=1):
    return [alpha % R, beta % R, 1, delta % R, tau % R]


@functools.lru_cache(maxsize=None)
def oracle_exponents(name, alpha=ALPHA, beta=BETA, tau=TAU):
    """(ex1, ex2, io) as integer lists: the oracle's setup exponents for (alpha, beta, 1, 1, tau)"""
    cs, _ = circuit(name)
    e1, e2, eio = O.groth16_setup_exponents(cs.n, cs.m, *csrs(cs), cs.mid, frs(toxic(alpha, beta, tau)))
    return RC.fr_ints(e1), RC.fr_ints(e2), RC.fr_ints(eio)


def srs_of_exponents(t1, at1, bt1, b2, t2):
    """the string as points, every one through the oracle's multiplication of the generator"""
    g1 = lambda ex: np.frombuffer(O.points_of_exponents_g1(frs(ex)), dtype=np.uint8).copy()
    g2 = lambda ex: np.frombuffer(O.points_of_exponents_g2(frs(ex)), dtype=np.uint8).copy()
    return SRS(g1(t1), g1(at1), g1(bt1), bytes(g2([b2])), g2(t2))


@functools.lru_cache(maxsize=None)
def honest_srs(n, alpha=ALPHA, beta=BETA, tau=TAU):
    return srs_of_exponents(*SM.honest_string(n, alpha % R, beta % R, tau % R))
