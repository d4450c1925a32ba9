"""Trapdoors and blindings that no seeded random draw ever gives: tau (Pinocchio: s) inside the QAP's own points 0 .. n-1, on the shifted points
n .. 2n-2 that carry the Lagrange-form h basis, 1, r - 1, a 4th root of unity; alpha, beta or a Pinocchio scalar zero; blindings that make the
proof elements A and B the identity.  ONE table, the circuits it runs on, an independent Lagrange basis in Python integers (lagrange_ref: the plain
product formula, O(n^2), no shared inversion -- every expectation that needs l_i(tau), lambda_t(tau) or Z(tau) takes it from here, never from
groth16._lagrange_at, zk_fr_lagrange_at or the oracle's own shortcut) and the expectations both test modules share, computed once and never
changed.  Helpers only, no GPU; tests/test_degenerate_trapdoors.py (CPU) and tests/test_gpu_degenerate_trapdoors.py (GPU) use them."""
import functools

import numpy as np

import oracle_lib as O
from nonpow2_cases import sparse_products
from oracle import pyref as P
from zukelang_amd import r1cs as RC

R = RC.FR_MODULUS
I4 = pow(7, (R - 1) // 4, R)                    # 7 generates Fr*: a primitive 4th root of unity (I4^2 = -1)
assert I4 * I4 % R == R - 1
frb = P.fr_to_bytes
frs = lambda xs: b"".join(frb(x % R) for x in xs)
csrs = lambda cs: [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
IDENT1, IDENT2 = b"\x40" + bytes(95), b"\x40" + bytes(191)
IDENT1_WIRE, IDENT2_WIRE = b"\xc0" + bytes(47), b"\xc0" + bytes(95)
G16 = dict(alpha=0, beta=1, gamma=2, delta=3, tau=4)
PIN = dict(rv=0, rw=1, s=2, av=3, aw=4, ay=5, b=6, gm=7)


# ---- circuits: made once, shared, never changed
def _single_gate():
    """n = 1: out = x * x, the circuit of tests/test_gpu_edges.py"""
    Mx = RC.Matrix.from_rows
    cs = RC.R1CS(1, 3, Mx([{2: 1}]), Mx([{2: 1}]), Mx([{1: 1}]), np.array([0, 0, 1], dtype=np.uint8))
    x = 0x1234567
    return cs, [1, x * x % R, x]


_MAKERS = {
    "gate1": _single_gate,
    "readme": lambda: RC.readme_circuit(3),
    "cubic6": lambda: RC.iterated_cubic(6, 9),
    "random24": lambda: RC.random_r1cs(24, 40, 0xDE6E24),
    "cubic64": lambda: RC.iterated_cubic(64, 0xDE6E64),
    "random1025": lambda: RC.random_r1cs(1025, 1300, 0xDE6E1025, nnz=(1, 4)),          # n2 = 2048: the tree and the derivation leave the LDS-fused node sizes
}
CIRCUITS = list(_MAKERS)
LITERAL = [c for c in CIRCUITS if c != "random1025"]          # n <= 64: the literal oracle serves them
SMALL = [c for c in LITERAL if c != "cubic64"]                # n <= 24
PER_VARIABLE = ["gate1", "readme", "cubic6"]                  # n <= 6: groth16_proof folds per variable (1.7 s a proof at n = 24, 5 s at 64)


@functools.lru_cache(maxsize=None)
def circuit(name):
    """(cs, satisfying witness as Python integers)"""
    cs, w = _MAKERS[name]()
    assert cs.n <= 64 and cs.check(w) or name == "random1025"
    return cs, w


def n_of(name):
    return {"gate1": 1, "readme": 3, "cubic6": 6, "random24": 24, "cubic64": 64, "random1025": 1025}[name]


# ---- the table
def tau_values(name):
    """label -> tau, in the issue's order; a later label whose value already stands is dropped (small n)"""
    n = n_of(name)
    if name == "random1025":
        cand = [("0", 0), ("n-1", n - 1), ("2n-2", 2 * n - 2), ("r-1", R - 1)]
    else:
        cand = [("0", 0), ("1", 1), ("2", 2), ("n-1", n - 1), ("n", n), ("2n-2", 2 * n - 2), ("2n-1", 2 * n - 1), ("r-1", R - 1), ("i4", I4)]
    out, seen = [], set()
    for label, v in cand:
        if v % R not in seen:
            seen.add(v % R)
            out.append((label, v % R))
    return out


def _base(name, count):
    st = P.fr_stream(0xDE6E0000 + 64 * n_of(name) + count)
    return [next(st) for _ in range(count)]


def groth16_rows(name):
    """[(row label, (alpha, beta, gamma, delta, tau))]: a seeded random base with the named entries replaced"""
    base = _base(name, 5)
    assert all(x > 2 * n_of(name) and x != R - 1 for x in base)

    def put(**kw):
        t = list(base)
        for k, v in kw.items():
            t[G16[k]] = v
        return tuple(t)
    rows = [("tau=" + label, put(tau=v)) for label, v in tau_values(name)]
    if name != "random1025":
        rows += [("alpha=0", put(alpha=0)), ("beta=0", put(beta=0)), ("alpha=beta=0", put(alpha=0, beta=0)), ("delta=1", put(delta=1)), ("gamma=r-1", put(gamma=R - 1))]
    return rows


def pinocchio_rows(name):
    """[(row label, (rv, rw, s, av, aw, ay, b, gm))].  At n = 1025 only s = 2n-2 and s = r-1: no oracle serves s inside the domain there (the
    trapdoor form has no h(s) at Z(s) = 0 and the literal form ends at n = 64), so those rows do not exist."""
    base = _base(name, 8)
    assert all(x > 2 * n_of(name) and x != R - 1 for x in base)

    def put(k, v):
        t = list(base)
        t[PIN[k]] = v
        return tuple(t)
    if name == "random1025":
        return [("s=" + label, put("s", v)) for label, v in tau_values(name) if label in ("2n-2", "r-1")]
    return [("s=" + label, put("s", v)) for label, v in tau_values(name)] + [(k + "=0", put(k, 0)) for k in PIN if k != "s"]


def base_row(name, count):
    """the seeded random trapdoor the rows start from: the honest key of the blinding cases"""
    return tuple(_base(name, count))


def tau_label(name, value):
    """the label under which a value stands in the circuit's list (n-1 stands as "2" at n = 3)"""
    return next(label for label, v in tau_values(name) if v == value % R)


def cases(names, rows_of):
    return [(name, label) for name in names for label, _ in rows_of(name)]


def row(rows_of, name, label):
    return dict(rows_of(name))[label]


# ---- the independent basis
@functools.lru_cache(maxsize=None)
def lagrange_ref(n, first, x):
    """(l_0(x) .. l_{n-1}(x)), Z(x) over the points first .. first+n-1: l_i(x) = prod_{j != i} (x - p_j) / (p_i - p_j), each numerator, each
    denominator and each inverse on its own.  Nothing is shared between the l_i and nothing divides by x - p_i, so a point of the domain is no
    special case: there every numerator but one holds the factor 0 and the remaining one equals its denominator."""
    pts = [first + j for j in range(n)]
    lag = []
    for i in range(n):
        num = den = 1
        for j in range(n):
            if j != i:
                num = num * (x - pts[j]) % R
                den = den * (pts[i] - pts[j]) % R
        lag.append(num * pow(den, R - 2, R) % R)
    z = 1
    for p in pts:
        z = z * (x - p) % R
    return tuple(lag), z


def in_domain(name, x):
    return x % R < n_of(name)


@functools.lru_cache(maxsize=None)
def _matrices(name):
    """the three matrices as {(row, column): value} in Python integers"""
    cs, _ = circuit(name)
    out = []
    for M in (cs.L, cs.R, cs.O):
        vals = RC.fr_ints(M.val)
        out.append([(g, int(M.col[e]), vals[e]) for g in range(cs.n) for e in range(int(M.ptr[g]), int(M.ptr[g + 1]))])
    return out


def columns_ref(name, x):
    """v_k(x), w_k(x), y_k(x) for every variable k: sum_g M[g][k] l_g(x) with l from lagrange_ref"""
    cs, _ = circuit(name)
    lag, _z = lagrange_ref(cs.n, 0, x)
    out = []
    for M in _matrices(name):
        col = [0] * cs.m
        for g, k, c in M:
            col[k] = (col[k] + c * lag[g]) % R
        out.append(col)
    return out


def vw_at(name, x):
    """v(x), w(x), y(x) of the circuit's witness: the interpolants of L w, R w, O w"""
    cs, w = circuit(name)
    lag, _z = lagrange_ref(cs.n, 0, x)
    return tuple(sum(a * l for a, l in zip(vals, lag)) % R for vals in sparse_products(cs, w))


# ---- expected exponents, from lagrange_ref alone
def groth16_exponents_ref(name, tox):
    """The key's exponents in both forms: (tau-power g1, g2, vkey io, Lagrange-form g1, g2)."""
    cs, _ = circuit(name)
    n, m = cs.n, cs.m
    a, b, gm, d, t = tox
    lag, z = lagrange_ref(n, 0, t)
    lam, _ = lagrange_ref(n - 1, n, t)
    vk, wk, yk = columns_ref(name, t)
    dinv, ginv = pow(d, R - 2, R), pow(gm, R - 2, R)
    Lk = [(b * vk[k] + a * wk[k] + yk[k]) % R for k in range(m)]
    ztd = z * dinv % R
    ltd = [Lk[k] * dinv % R for k in range(m) if cs.mid[k]]
    e1 = [a, d, b] + [pow(t, i, R) for i in range(n + 2)] + [pow(t, i, R) * ztd % R for i in range(n - 1)] + ltd
    e2 = [b, d] + [pow(t, i, R) for i in range(n + 2)]
    eio = [Lk[k] * ginv % R for k in range(m) if not cs.mid[k]]
    l1 = [a, d, b] + list(lag) + [x * ztd % R for x in lam] + ltd
    l2 = [b, d] + list(lag)
    return e1, e2, eio, l1, l2


def pinocchio_h_exponents_ref(name, tox, compact):
    """pool 5 of a derived Pinocchio key: [lambda_t(s)] (n-1) | [Z(s)] | [1] | then [s^(n-1)] (compact) or v_all | w_all"""
    cs, _ = circuit(name)
    n = cs.n
    s = tox[PIN["s"]]
    lam, _ = lagrange_ref(n - 1, n, s)
    _, z = lagrange_ref(n, 0, s)
    if compact:
        return list(lam) + [z, 1, pow(s, n - 1, R)]
    vk, wk, _yk = columns_ref(name, s)
    return list(lam) + [z, 1] + vk + wk


@functools.lru_cache(maxsize=None)
def points1(exps):
    return O.points_of_exponents_g1(frs(exps))


@functools.lru_cache(maxsize=None)
def points2(exps):
    return O.points_of_exponents_g2(frs(exps))


# ---- blindings
def blindings(name, tox):
    """[(label, (r, s))] for a Groth16 key: the pair that makes A = [alpha + v(tau) + r delta]_1 and B = [beta + w(tau) + s delta]_2 the identity,
    (0, 0) and (r-1, r-1).  v(tau), w(tau) from lagrange_ref."""
    a, b, _gm, d, t = tox
    v, w, _y = vw_at(name, t)
    dinv = pow(d, R - 2, R)
    return [("A=B=identity", ((R - (a + v) % R) * dinv % R, (R - (b + w) % R) * dinv % R)), ("zero", (0, 0)), ("minus one", (R - 1, R - 1))]


def public(name):
    """indices of the public variables, in the key's order"""
    cs, _ = circuit(name)
    return [k for k in range(cs.m) if not cs.mid[k]]


def groth16_accepts_changed_input(name, tox, j):
    """Does a good proof still verify when public input j is changed?  The two sides of groth16.ml:163-173 then differ by (the change) * L_k(tau):
    it must be rejected exactly where [L_k(tau) / gamma]_1, the input's ltgm_io point, is not the identity."""
    a, b, _gm, _d, t = tox
    k = public(name)[j]
    vk, wk, yk = columns_ref(name, t)
    return (b * vk[k] + a * wk[k] + yk[k]) % R == 0


def pinocchio_accepts_changed_input(name, tox, d, j):
    """The same for Verify.f with input j raised by 1: the four knowledge-of-coefficient checks never read the inputs; the divisibility check
    e(V, W) = e(Y, 1) e(h, yt) (pinocchio.ml:418-420) is rv rw ((v + v_k)(w + w_k) - (y + y_k) - h t) = 0 in the exponent, v = v(s) + dv t,
    w = w(s) + dw t the proof's totals: it moves by rv rw (v_k w + w_k v + v_k w_k - y_k).  tests/test_degenerate_trapdoors.py holds this rule to
    the big-integer pairing of oracle_lib.pinocchio_verify."""
    rv, rw, s = tox[0], tox[1], tox[2]
    k = public(name)[j]
    vk, wk, yk = columns_ref(name, s)
    v, w, _y = vw_at(name, s)
    _, t = lagrange_ref(n_of(name), 0, s)
    v, w = (v + d[0] * t) % R, (w + d[1] * t) % R
    return rv * rw * (vk[k] * w + wk[k] * v + vk[k] * wk[k] - yk[k]) % R == 0


def draws(name, label, count, width=2):
    st = P.fr_stream(0xD7A30000 + 64 * n_of(name) + sum(label.encode()))
    return [tuple(next(st) for _ in range(width)) for _ in range(count)]


# ---- the oracle's answers, once per row
@functools.lru_cache(maxsize=None)
def qap(name):
    cs, _ = circuit(name)
    assert name in LITERAL
    return O.QAP(cs.n, cs.m, *csrs(cs))


@functools.lru_cache(maxsize=None)
def groth16_key(name, tox):
    """(pk_g1, pk_g2, vk_g1, vk_g2) bytes: the literal setup (Poly.apply on the dense QAP) at n <= 64; at n = 1025 the exponent form, which
    tests/test_degenerate_trapdoors.py holds to the literal one on every row of the smaller circuits"""
    cs, _ = circuit(name)
    if name in LITERAL:
        return qap(name).groth16_setup(frs(tox), cs.mid)
    e1, e2, eio = O.groth16_setup_exponents(cs.n, cs.m, *csrs(cs), cs.mid, frs(tox))
    from zukelang_amd.curve import G1, G2          # fixed-base kernel: n = 1025 is reached by the GPU module only
    return bytes(G1.of_Fr(e1)), bytes(G2.of_Fr(e2)), O.g1_generator() + bytes(G1.of_Fr(eio)), O.g2_generator() + bytes(G2.of_Fr(frs([tox[2], tox[3]])))


@functools.lru_cache(maxsize=None)
def groth16_proof(name, tox, r, s, w=None):
    """(a, b, c) of the satisfying witness (or of `w`, a tuple): orc_groth16_prove on the dense QAP and the literal setup's points -- per variable
    (literal = 1, groth16.ml:116-121) at n <= 6; from n = 24 on the summed coefficient vectors (literal = 0: the same function after one use of
    linearity), which tests/test_degenerate_trapdoors.py holds to the per-variable fold on every row it keeps; the trapdoor form at n = 1025."""
    cs, wit = circuit(name)
    wit = list(w) if w is not None else wit
    if name in LITERAL:
        pk1, pk2, _, _ = groth16_key(name, tox)
        rc, a, b, c = qap(name).groth16_prove(pk1, pk2, cs.mid, frs(wit), frb(r), frb(s), literal=name in PER_VARIABLE)
        assert rc == 0, rc
        return a, b, c
    return O.groth16_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, frs(wit), frs(tox), frb(r), frb(s))


@functools.lru_cache(maxsize=None)
def pinocchio_key(name, tox):
    """(pk_g1, pk_g2, vk_g1, vk_g2) bytes from the literal exponents (n <= 64) or the Lagrange-basis ones (n = 1025)"""
    cs, _ = circuit(name)
    lit = name in LITERAL
    ex = O.pinocchio_keygen_exponents(qap(name) if lit else None, cs.n, cs.m, *csrs(cs), cs.mid, frs(tox), lit)
    if lit:
        return O.points_of_exponents_g1(ex[0]), O.points_of_exponents_g2(ex[1]), O.points_of_exponents_g1(ex[2]), O.points_of_exponents_g2(ex[3])
    from zukelang_amd.curve import G1, G2
    return bytes(G1.of_Fr(ex[0])), bytes(G2.of_Fr(ex[1])), bytes(G1.of_Fr(ex[2])), bytes(G2.of_Fr(ex[3]))


@functools.lru_cache(maxsize=None)
def pinocchio_proof(name, tox, d):
    """960 bytes: the literal ZKCompute.f on the key's points (n <= 64), the trapdoor form at n = 1025 (s outside the domain there)"""
    cs, wit = circuit(name)
    if name in LITERAL:
        pk1, pk2, _, _ = pinocchio_key(name, tox)
        rc, out = O.pinocchio_prove(qap(name), pk1, pk2, cs.mid, frs(wit), *(frb(x) for x in d))
        assert rc == 0, rc
        return out
    return O.pinocchio_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, frs(wit), frs(tox), *(frb(x) for x in d))


def bad_witness(name):
    """the witness with one variable of a row of O changed: some row no longer holds"""
    cs, w = circuit(name)
    val = RC.fr_ints(cs.O.val)
    k = int(cs.O.col[next(e for e in range(len(val)) if val[e])])
    bad = list(w)
    bad[k] = (bad[k] + 1) % R
    assert any(x * y % R != z for x, y, z in zip(*sparse_products(cs, bad)))
    return bad
