"""Constraint counts n that are no power of two and no longer fit one LDS tile (n2 = 2^ceil(log2 n) > NTT_T): the sizes with the reason for each, the
Fr stage's plan restated as plain functions of n (csrc/frstage.hip, csrc/ntt.hip -- tests/test_nonpow2_plan.py holds the restatement to the source by
text and every size to its reason), a circuit whose operand values the caller chooses freely, six degenerate witnesses on it, and the evaluation of an
interpolant from its values in Python integers.  Helpers only; tests/test_nonpow2_plan.py (CPU) and tests/test_gpu_nonpow2.py (GPU) use them."""
import numpy as np

from zukelang_amd import r1cs as RC

R = RC.FR_MODULUS

# ---- csrc/ntt_lds.cuh, csrc/frstage.hip, csrc/frstage.cuh
NTT_LOG_T = 10
FCH = 256
LEAD_THREADS = 256
LEAD_BLOCKS = 128

# ---- the sizes: ONE table, a case cannot drift from its reason
SIZES = {
    1025: "odd; the first size with an unfused tree level (11); S = 2^12; a tree nearly half empty (1023 of 2048 leaves are no points)",
    2047: "odd; one short of a full tree",
    3000: "even; the last step of the power-series inverse goes 2048 -> 2999, no doubling; not a multiple of 256",
    8193: "odd; four unfused levels (11 .. 14); the transforms of S = 2^15 put a strided pass of five stages in front of the tile",
    40000: "S = 2^17; crosses LEAD_BLOCKS * 256 = 32768 values: k_lead_partial makes a second, ragged trip of 7232",
}


def ceil_log2(n):
    return (n - 1).bit_length()


def ntt_passes(log_len, log_total):
    """csrc/ntt.hip `plan`: (stages of every strided pass, first to last; stages of the contiguous pass in the tile)"""
    log_T = min(log_total, NTT_LOG_T)
    s_last = min(log_len, log_T)
    rem = log_len - s_last
    strided = []
    if rem:
        smax = log_T - 2
        np_ = (rem + smax - 1) // smax
        for p in range(np_):
            s = (rem + (np_ - p) - 1) // (np_ - p)
            strided.append(s)
            rem -= s
    return strided, s_last


def plan(n):
    """What frstage_init / frstage_eval / frstage_init_lagrange / frstage_leading_coeffs do for n constraints, n > 1."""
    log_n2 = ceil_log2(n)
    n2 = 1 << log_n2
    log_S = log_n2 + 1
    fused = min(log_n2, NTT_LOG_T)                       # levels inside k_tree_levels_fused (tree_convert, batch 1: total = n2)
    need = n - 1                                         # (rev Z)^-1 mod X^(n-1)
    prec, precisions = 1, [1]
    while prec < need:
        prec = prec * 2 if prec * 2 < need else need     # uint64_t p2 = prec * 2 < need ? prec * 2 : need;
        precisions.append(prec)
    cnt = n - 1                                          # k_zt: zt[t] for t < n - 1, 256 per lane
    blocks = min((n + LEAD_THREADS - 1) // LEAD_THREADS, LEAD_BLOCKS)
    stride = blocks * LEAD_THREADS
    return dict(
        n=n, n2=n2, log_n2=log_n2, log_S=log_S, S=1 << log_S,
        z_from_newton=n != n2,                           # the else branch of `if (n == n2)`
        fused_levels=fused, unfused_levels=list(range(fused + 1, log_n2 + 1)), rns_first_level=fused + 1,
        empty_leaves=n2 - n,
        inverse_precisions=precisions,
        last_inverse_step_is_a_doubling=len(precisions) < 2 or precisions[-1] == 2 * precisions[-2],
        zt_chunks=(cnt + FCH - 1) // FCH, zt_last_chunk=cnt % FCH or FCH, zt_ragged=cnt % FCH != 0,
        zt_catch_up_steps=n % FCH + 1,                   # for e = ch * FCH; e <= j0 with j0 = n + 256 c: (j0 mod 256) + 1 steps
        lead_blocks=blocks, lead_full_trips=n // stride, lead_tail=n % stride,
        passes_S=ntt_passes(log_S, log_S + 1),           # the Newton step transforms two vectors of S in one batch
    )


# ---- a circuit with free operand values
def free_circuit(n):
    """Variables ONE, a_0 .. a_{n-1}, b_0 .., c_0 ..; row i: a_i * b_i = c_i.  m = 3 n + 1, public = {ONE, c_{n-1}}; ONE occurs in no row.  The caller
    chooses a_i and b_i at will (witness_of)."""
    L = RC.Matrix.from_rows([{1 + i: 1} for i in range(n)])
    Rm = RC.Matrix.from_rows([{1 + n + i: 1} for i in range(n)])
    O = RC.Matrix.from_rows([{1 + 2 * n + i: 1} for i in range(n)])
    mid = np.ones(3 * n + 1, dtype=np.uint8)
    mid[0] = 0
    mid[3 * n] = 0
    return RC.R1CS(n, 3 * n + 1, L, Rm, O, mid)


def witness_of(a, b, one=1):
    a, b = [x % R for x in a], [x % R for x in b]
    return [one] + a + b + [x * y % R for x, y in zip(a, b)]


# name -> (a, b, ONE) as functions of n, and what h must be: "zero" (no coefficient), "one" (the constant 1), "full" (n - 1 non-zero coefficients)
DEGENERATE = {
    "zero": (lambda n: ([0] * n, [0] * n, 0), "zero"),                                              # v = w = y = h = 0, every MSM scalar is 0
    "v_zero": (lambda n: ([0] * n, [5 + i for i in range(n)], 1), "zero"),
    "v_constant": (lambda n: ([7] * n, [pow(3, i, R) for i in range(n)], 1), "zero"),               # h = 0 while v, w, y are not
    "r_minus_1": (lambda n: ([R - 1] * n, [R - 1] * n, 1), "zero"),
    "h_one": (lambda n: ([pow(i, n - 1, R) for i in range(n)], list(range(n)), 1), "one"),          # v w = X^n, y = X^n - Z
    "full_degree": (lambda n: ([pow(i, n - 1, R) for i in range(n)], [(pow(i, n - 1, R) + 1) % R for i in range(n)], 1), "full"),
}


def degenerate_witness(name, n):
    """(witness, kind of h)"""
    make, kind = DEGENERATE[name]
    a, b, one = make(n)
    return witness_of(a, b, one), kind


# ---- the reference for coefficient vectors beyond the literal oracle's reach
def product_formula(n, first, x, idx):
    """l_i(x) = prod_{j != i} (x - p_j) / (p_i - p_j) over the points p_j = first + j, for the indices `idx`, and Z(x): plain products in Python
    integers, one pass of prefix / suffix products of the numerators and ONE modular inversion (of (n-1)!) for all the denominators."""
    d = [(x - first - j) % R for j in range(n)]
    pre = [1] * (n + 1)
    for j in range(n):
        pre[j + 1] = pre[j] * d[j] % R
    suf = [1] * (n + 1)
    for j in range(n - 1, -1, -1):
        suf[j] = suf[j + 1] * d[j] % R
    fact = [1] * n
    for j in range(1, n):
        fact[j] = fact[j - 1] * j % R
    invfact = [1] * n
    invfact[n - 1] = pow(fact[n - 1], R - 2, R)
    for j in range(n - 1, 0, -1):
        invfact[j - 1] = invfact[j] * j % R
    vals = {}
    for i in idx:
        inv = invfact[i] * invfact[n - 1 - i] % R                 # 1 / (prod_{j<i} (i - j) * |prod_{j>i} (i - j)|)
        if (n - 1 - i) & 1:
            inv = R - inv
        vals[i] = pre[i] * suf[i + 1] % R * inv % R
    return vals, pre[n]


def eval_by_values(values, x):
    """The interpolant of `values` over the points 0 .. n-1, evaluated at x."""
    n = len(values)
    lag, _ = product_formula(n, 0, x, range(n))
    return sum(values[i] * lag[i] for i in range(n)) % R


def vanishing_at(n, x):
    """Z(x) = prod_{i<n} (x - i), the plain product"""
    z = 1
    for i in range(n):
        z = z * (x - i) % R
    return z


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def sparse_products(cs, w):
    """a = L w, b = R w, c = O w in Python integers"""
    out = []
    for M in (cs.L, cs.R, cs.O):
        vals = RC.fr_ints(M.val)
        ptr, col = [int(p) for p in M.ptr], [int(c) for c in M.col]
        out.append([sum(vals[e] * w[col[e]] for e in range(ptr[g], ptr[g + 1])) % R for g in range(cs.n)])
    return out
