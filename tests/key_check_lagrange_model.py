"""The specification of zk_groth16_key_check_lagrange as an integer model: every relation of include/zkmi355x.h ("a Lagrange-form key as a whole")
evaluated on the EXPONENTS of the key's points, over Python integers -- once index by index (`lagrange_mask`: a bit is set exactly if some index
violates its relation) and once in the COMBINED form the device runs (`combined_mask`: one random linear combination per family, as a function of the
coefficients a seed would expand to).  A pairing equation e(P, Q) = e(R, S) between subgroup points is p q = r s (mod r) between their exponents.

  lx1: exponents of the G1 pool a | d1 | b1 | l1[n] | hl[n-1] | ltd_mid[n_mid]          lx2: of the G2 pool b2 | d2 | l2[n]
  vk:  None, or dict(one1, ltgm_io (list, variable order), one2, gm, d) of exponents
  l_i: the Lagrange basis of the points 0..n-1     lambda_t: of the points n..2n-2     w_i = (-1)^(n-1-i) / (i! (n-1-i)!): the weights of 0..n-1
  g1 := sum l1, g2 := sum l2 (honestly the generators: sum l_i = 1)      T2 := sum i l2[i] (honestly [tau]_2: sum i l_i(X) = X for n >= 2)

Why the relations pin the key down (held to direct interpolation in tests/test_key_check_lagrange_model.py):
  TAU_G1  d_i := l1[i] (i g2 - T2) proportional to w_i.  A linear form in pi vanishes on the whole hyperplane {sum w_i pi_i = 0} exactly when its
          coefficient vector is proportional to w, so the combined form forces (i - tau) x_i = c w_i for ONE c; with sum x_i = 1 that is x_i = l_i(tau),
          also for a tau inside the domain (c = 0, x a unit vector).
  H_BASES w_0 hl[t] d2 = l2[0] sum_i i lambda_t(i) l1[i]: sum_i i lambda_t(i) l_i(tau) = tau lambda_t(tau) (degree n - 1), tau l_0(tau) / w_0 = Z(tau),
          so hl[t] delta = lambda_t(tau) Z(tau).  The hyperplane is the values on 0..n-1 of the polynomials q of degree <= n - 2; q -> (q(n + t))_t is a
          bijection onto Fr^(n-1), so every t has a coefficient of its own.
  L       needs only VALUES: sum_i M[i][k] l1[i] is u_k(tau) through the Lagrange basis (a sparse product)."""
import functools

from key_check_model import BETA, DELTA, GAMMA, GENERATORS, H_BASES, L, NAMES, TAU_G1, TAU_G2, P, _entries, column_dots, honest_exponents, names  # noqa: F401


def inv(x):
    return pow(x % P, P - 2, P)


def factorials(n):
    f = [1] * (n + 1)
    for i in range(1, n + 1):
        f[i] = f[i - 1] * i % P
    return f


def weights(n):
    """w_i = 1 / prod_{j != i} (i - j) = (-1)^(n-1-i) / (i! (n-1-i)!), i < n"""
    f = factorials(n)
    return [(P - 1 if (n - 1 - i) & 1 else 1) * inv(f[i] * f[n - 1 - i]) % P for i in range(n)]


def basis_at(first, count, x):
    """the Lagrange basis of the points first .. first + count - 1 at x (a unit vector when x is one of them)"""
    x %= P
    pts = [(first + j) % P for j in range(count)]
    if x in pts:
        return [1 if p == x else 0 for p in pts]
    z = 1
    for p in pts:
        z = z * (x - p) % P
    w = weights(count)
    return [z * w[j] % P * inv(x - pts[j]) % P for j in range(count)]


def z_at(n, x):
    z = 1
    for i in range(n):
        z = z * (x - i) % P
    return z


@functools.lru_cache(maxsize=8)
def lambda_table(n):
    """lam[t][i] = lambda_t(i) for t < n - 1, i < n: exact, the basis of n..2n-2 at the integer points 0..n-1.
    lambda_t(i) = N(i) / ((i - n - t) D_t), N(i) = prod_u (i - n - u), D_t = prod_{u != t} (t - u) = (-1)^(n-2-t) t! (n-2-t)!"""
    if n < 2:
        return []
    f = factorials(n)
    inv_neg = [0] + [inv(-e) for e in range(1, 2 * n)]                      # 1 / (-e): i - n - t = -e, 1 <= e <= 2n - 2
    N = []
    for i in range(n):
        v = 1
        for u in range(n - 1):
            v = v * (i - n - u) % P
        N.append(v)
    out = []
    for t in range(n - 1):
        dinv = inv(f[t] * f[n - 2 - t])
        if (n - 2 - t) & 1:
            dinv = P - dinv
        out.append([N[i] * inv_neg[n + t - i] % P * dinv % P for i in range(n)])
    return out


@functools.lru_cache(maxsize=8)
def _h_sums(n, l1):
    """sum_i i lambda_t(i) l1[i] for t < n - 1 (l1 a tuple: the crafted keys that leave l1 alone share one evaluation)"""
    lam = lambda_table(n)
    return [sum(i * lam[t][i] * l1[i] for i in range(1, n)) % P for t in range(n - 1)]


def split_pools(n, n_mid, lx1, lx2):
    assert len(lx1) == 3 + n + (n - 1) + n_mid and len(lx2) == 2 + n
    return dict(a=lx1[0], d1=lx1[1], b1=lx1[2], l1=lx1[3:3 + n], hl=lx1[3 + n:2 + 2 * n], ltd=lx1[2 + 2 * n:], b2=lx2[0], d2=lx2[1], l2=lx2[2:])


def _static_bits(K, g1, g2, vk):
    """what is tested on bytes and identities, not by a pairing: the same in both forms"""
    mask = 0
    if g1 != 1 or g2 != 1 or (vk and (vk["one1"] % P != 1 or vk["one2"] % P != 1)):
        mask |= GENERATORS
    if K["d1"] == 0 or K["d2"] == 0 or (vk and vk["d"] % P != K["d2"]):
        mask |= DELTA
    if vk and vk["gm"] % P == 0:
        mask |= GAMMA
    return mask


def lagrange_mask(circuit, lx1, lx2, vk=None):
    n, m = circuit.n, circuit.m
    mids = [k for k in range(m) if circuit.mid[k]]
    ios = [k for k in range(m) if not circuit.mid[k]]
    K = split_pools(n, len(mids), [x % P for x in lx1], [x % P for x in lx2])
    l1, l2 = K["l1"], K["l2"]
    g1, g2, T2 = sum(l1) % P, sum(l2) % P, sum(i * x for i, x in enumerate(l2)) % P
    w = weights(n)
    mask = _static_bits(K, g1, g2, vk)
    if any(l1[i] * g2 % P != g1 * l2[i] % P for i in range(n)):
        mask |= TAU_G2
    if n >= 2:
        d = [l1[i] * (i * g2 - T2) % P for i in range(n)]
        if any(d[i] * w[0] % P != d[0] * w[i] % P for i in range(n)):
            mask |= TAU_G1
        hs = _h_sums(n, tuple(l1))
        if any(w[0] * K["hl"][t] % P * K["d2"] % P != l2[0] * hs[t] % P for t in range(n - 1)):
            mask |= H_BASES
    if K["b1"] * g2 % P != g1 * K["b2"] % P:
        mask |= BETA
    if K["d1"] * g2 % P != g1 * K["d2"] % P:
        mask |= DELTA
    V, W, Y = column_dots(circuit, circuit.L, l1), column_dots(circuit, circuit.R, l2), column_dots(circuit, circuit.O, l1)
    rhs = [(V[k] * K["b2"] + K["a"] * W[k] + Y[k] * g2) % P for k in range(m)]
    bad = any(K["ltd"][j] * K["d2"] % P != rhs[k] for j, k in enumerate(mids))
    if vk:
        assert len(vk["ltgm_io"]) == len(ios)
        bad = bad or any(vk["ltgm_io"][j] * vk["gm"] % P != rhs[k] for j, k in enumerate(ios))
    if bad:
        mask |= L
    return mask


# ---------------------------------------------------------------- the combined form: what the device computes, in integers
def project(n, r):
    """pi from a raw vector r without a division: pi_i = r_i / (n-1)! for i < n - 1, pi_(n-1) = - sum_{i < n-1} w_i r_i; then sum w_i pi_i = 0
    (w_(n-1) = 1 / (n-1)!).  Onto: every pi of the hyperplane comes from r_i = (n-1)! pi_i."""
    w = weights(n)
    invf = w[n - 1]
    return [invf * r[i] % P for i in range(n - 1)] + [(-sum(w[i] * r[i] for i in range(n - 1))) % P]


def extrapolate(n, pi):
    """sigma_t = q(n + t), t < n - 1, for the interpolant q of pi on 0..n-1, by the barycentric sum the device's convolution computes:
    q(j) = Z(j) sum_i pi_i w_i / (j - i)"""
    w = weights(n)
    return [z_at(n, n + t) * sum(pi[i] * w[i] % P * inv(n + t - i) for i in range(n)) % P for t in range(n - 1)]


def matvec(circuit, M, x):
    out = [0] * circuit.n
    for g, k, c in _entries(M):
        out[g] = (out[g] + c * x[k]) % P
    return out


def combined_mask(circuit, lx1, lx2, vk, rho, r, mu):
    """rho, r: n coefficients each; mu: m (those outside mids are not read without a verification key).  The six combined equations."""
    n, m = circuit.n, circuit.m
    mids = [k for k in range(m) if circuit.mid[k]]
    ios = [k for k in range(m) if not circuit.mid[k]]
    K = split_pools(n, len(mids), [x % P for x in lx1], [x % P for x in lx2])
    l1, l2 = K["l1"], K["l2"]
    g1, g2, T2 = sum(l1) % P, sum(l2) % P, sum(i * x for i, x in enumerate(l2)) % P
    mask = _static_bits(K, g1, g2, vk)
    dot = lambda c, x: sum(a * b for a, b in zip(c, x)) % P
    if dot(rho, l1) * g2 % P != g1 * dot(rho, l2) % P:
        mask |= TAU_G2
    if n >= 2:
        pi = project(n, r)
        sigma = extrapolate(n, pi)
        w0 = weights(n)[0]
        S = dot([i * p for i, p in enumerate(pi)], l1)
        if S * g2 % P != dot(pi, l1) * T2 % P:
            mask |= TAU_G1
        if dot([w0 * s for s in sigma], K["hl"]) * K["d2"] % P != S * l2[0] % P:
            mask |= H_BASES
    if K["b1"] * g2 % P != g1 * K["b2"] % P:
        mask |= BETA
    if K["d1"] * g2 % P != g1 * K["d2"] % P:
        mask |= DELTA
    mu = [x % P if (vk or circuit.mid[k]) else 0 for k, x in enumerate(mu)]
    V, W, Y = dot(matvec(circuit, circuit.L, mu), l1), dot(matvec(circuit, circuit.R, mu), l2), dot(matvec(circuit, circuit.O, mu), l1)
    lhs = dot([mu[k] for k in mids], K["ltd"]) * K["d2"]
    if vk:
        lhs += dot([mu[k] for k in ios], vk["ltgm_io"]) * vk["gm"]
    if lhs % P != (V * K["b2"] + K["a"] * W + Y * g2) % P:
        mask |= L
    return mask


def honest_lagrange_exponents(circuit, toxic):
    """(lx1, lx2, vk): the exponent lists Groth16.keygen(lagrange=True) uploads for toxic = (alpha, beta, gamma, delta, tau), also for a tau inside
    either domain (where keygen's one-inversion formula does not apply)"""
    a, b, gm, d, t = (x % P for x in toxic)
    n, m = circuit.n, circuit.m
    lag = basis_at(0, n, t)
    lam = basis_at(n, n - 1, t)
    v_, w_, y_ = (column_dots(circuit, M, lag) for M in (circuit.L, circuit.R, circuit.O))
    Lk = [(b * v_[k] + a * w_[k] + y_[k]) % P for k in range(m)]
    dinv, ginv = inv(d), inv(gm)
    ztd = z_at(n, t) * dinv % P
    lx1 = [a, d, b] + lag + [x * ztd % P for x in lam] + [Lk[k] * dinv % P for k in range(m) if circuit.mid[k]]
    lx2 = [b, d] + lag
    vk = dict(one1=1, ltgm_io=[Lk[k] * ginv % P for k in range(m) if not circuit.mid[k]], one2=1, gm=gm, d=d)
    return lx1, lx2, vk
