"""The specification of zk_groth16_pk_specialize as an integer model on EXPONENTS: the call is a linear map of the string's points, so on a string
[t1[i]] G1, [at1[i]] G1, [bt1[i]] G1, [b2] G2, [t2[i]] G2 -- whatever those exponents are, honest powers or not -- every output point is
[model exponent] G.  No group, no device code, Python integers only.

  a = at1[0]   d1 = 1   b1 = bt1[0]   ti1 = t1[0 .. n+1]   tiztd[i] = sum_j z_j t1[i+j], i < n-1   b2   d2 = 1   ti2 = t2[0 .. n+1]
  L_k = sum_i (L[i,k] <bt1, l_i> + R[i,k] <at1, l_i> + O[i,k] <t1, l_i>),  <e, l_i> = sum_j (l_i)_j e[j]   (beta with L, alpha with R: groth16.ml:59-68)
  ltd_mid = L_k of the mids, ltgm_io = L_k of the others (gamma = delta = 1), one1 = one2 = gm = d = 1

The Lagrange basis is interpolated here, independently of every other basis in the tree (as tests/degenerate_cases.py keeps its own): l_i is the
plain product of its n - 1 linear factors (X - j) / (i - j), coefficient by coefficient, every denominator inverted on its own.  O(n^3): for the
small n of tests/test_specialize_model.py and of the crafted strings of tests/test_gpu_specialize.py."""
import functools

from zukelang_amd.r1cs import FR_MODULUS as P


def srs_sizes(n):
    return max(n + 2, 2 * n - 1), n, n + 2


@functools.lru_cache(maxsize=None)
def lagrange_coeffs(n):
    """l_0 .. l_{n-1} over the points 0 .. n-1, each as n coefficients, lowest first"""
    out = []
    for i in range(n):
        poly = [1]
        for j in range(n):
            if j == i:
                continue
            inv = pow((i - j) % P, P - 2, P)
            nxt = [0] * (len(poly) + 1)
            for d, c in enumerate(poly):          # poly * (X - j) / (i - j)
                nxt[d + 1] = (nxt[d + 1] + c * inv) % P
                nxt[d] = (nxt[d] - c * j % P * inv) % P
            poly = nxt
        out.append(tuple(poly))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def z_coeffs(n):
    """Z = prod_{i<n} (X - i), n + 1 coefficients, lowest first"""
    z = [1]
    for i in range(n):
        z = [((z[d - 1] if d else 0) - i * (z[d] if d < len(z) else 0)) % P for d in range(len(z) + 1)]
    return tuple(z)


def _entries(M):
    vals = bytes(M.val)
    for g in range(len(M.ptr) - 1):
        for t in range(int(M.ptr[g]), int(M.ptr[g + 1])):
            yield g, int(M.col[t]), int.from_bytes(vals[32 * t:32 * t + 32], "little")


def honest_string(n, alpha, beta, tau):
    """(t1, at1, bt1, b2, t2) of a well-formed string, exactly the lengths a circuit of n constraints needs"""
    n1, nab, n2 = srs_sizes(n)
    pw = [pow(tau, i, P) for i in range(max(n1, n2))]
    return pw[:n1], [alpha * x % P for x in pw[:nab]], [beta * x % P for x in pw[:nab]], beta % P, pw[:n2]


def specialize_exponents(circuit, t1, at1, bt1, b2, t2):
    """(ex1, ex2, vk): the exponents of pk_g1, of pk_g2 and of the verification key (the dict tests/key_check_model.py takes)"""
    n, m = circuit.n, circuit.m
    n1, nab, n2 = srs_sizes(n)
    assert (len(t1), len(at1), len(bt1), len(t2)) == (n1, nab, nab, n2)
    basis = lagrange_coeffs(n)
    dot = lambda e, i: sum(c * e[j] for j, c in enumerate(basis[i])) % P
    lists = (bt1, at1, t1)          # L, R, O
    dots = [[dot(e, i) for i in range(n)] for e in lists]
    Lk = [0] * m
    for q, M in enumerate((circuit.L, circuit.R, circuit.O)):
        for g, k, c in _entries(M):
            Lk[k] = (Lk[k] + c * dots[q][g]) % P
    z = z_coeffs(n)
    tiztd = [sum(z[j] * t1[i + j] for j in range(n + 1)) % P for i in range(n - 1)]
    ex1 = [at1[0] % P, 1, bt1[0] % P] + [x % P for x in t1[:n + 2]] + tiztd + [Lk[k] for k in range(m) if circuit.mid[k]]
    ex2 = [b2 % P, 1] + [x % P for x in t2[:n + 2]]
    vk = dict(one1=1, ltgm_io=[Lk[k] for k in range(m) if not circuit.mid[k]], one2=1, gm=1, d=1)
    return ex1, ex2, vk


def crafted_alpha(n, alpha, beta, tau, other=0xBAD0A1FA):
    """the honest string with alpha_tau1[3] replaced: the [alpha l_i] change, a = alpha_tau1[0] does not -- the key check's relation L fails"""
    t1, at1, bt1, b2, t2 = honest_string(n, alpha, beta, tau)
    at1 = list(at1)
    assert at1[3] != other
    at1[3] = other
    return t1, at1, bt1, b2, t2


def crafted_high_power(n, alpha, beta, tau, other=0xBAD7A0):
    """the honest string with tau1[n+3] replaced: beyond ti1 and beyond the n powers the l_i are made of, inside tiztd's reach -- H_BASES alone"""
    t1, at1, bt1, b2, t2 = honest_string(n, alpha, beta, tau)
    t1 = list(t1)
    assert n + 3 < len(t1) and t1[n + 3] != other
    t1[n + 3] = other
    return t1, at1, bt1, b2, t2
