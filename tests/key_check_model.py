"""The specification of zk_groth16_key_check as an integer model: every relation of include/zkmi355x.h ("the key as a whole") evaluated index by
index on the EXPONENTS of the key's points, over Python integers.  No random combination, no group, no device code: a bit is set exactly if some
index violates its relation.  A pairing equation e(P, Q) = e(R, S) between subgroup points is the equation p q = r s (mod r) between their exponents.

  ex1: exponents of the G1 pool a | d1 | b1 | ti1[n+2] | tiztd[n-1] | ltd_mid[n_mid]      ex2: of the G2 pool b2 | d2 | ti2[n+2]
  vk:  None, or dict(one1, ltgm_io (list, variable order), one2, gm, d) of exponents
  circuit: an r1cs.R1CS; its per-variable polynomials v_k, w_k, y_k are the interpolants of the columns of L, R, O on the points 0..n-1

What the relation L needs of a polynomial u_k is <e, u_k> = sum_j (u_k)_j e[j] for an exponent list e (ti1 or ti2, whatever they hold).  With the
Lagrange basis l_g of 0..n-1, u_k = sum_g M[g][k] l_g, so <e, u_k> = sum_g M[g][k] <e, l_g>: `basis_dots` interpolates in big integers -- every l_g by
synthetic division of Z, O(n^2) -- and the columns are sparse sums."""
import functools

from zukelang_amd.r1cs import FR_MODULUS as P

GENERATORS, TAU_G1, TAU_G2, BETA, DELTA, H_BASES, L, GAMMA = 1, 2, 4, 8, 16, 32, 64, 128
NAMES = {GENERATORS: "generators", TAU_G1: "tau_g1", TAU_G2: "tau_g2", BETA: "beta", DELTA: "delta", H_BASES: "h_bases", L: "l", GAMMA: "gamma"}


def z_coeffs(n):
    """Z = prod_{i<n} (X - i), n + 1 coefficients, lowest first"""
    return list(_z_coeffs(n))


@functools.lru_cache(maxsize=8)
def _z_coeffs(n):
    z = [1]
    for i in range(n):
        nz = [0] * (len(z) + 1)
        for j, c in enumerate(z):
            nz[j + 1] = (nz[j + 1] + c) % P
            nz[j] = (nz[j] - i * c) % P
        z = nz
    return tuple(z)


def basis_dots(n, e):
    """[<e[0..n), l_g> for g < n]: l_g = c_g Z / (X - g), c_g = 1 / prod_{i != g} (g - i).  Crafted keys that leave a tau basis alone share its pass."""
    return list(_basis_dots(n, tuple(e[:n])))


@functools.lru_cache(maxsize=16)
def _basis_dots(n, e):
    z = _z_coeffs(n)
    fact = [1] * n
    for i in range(1, n):
        fact[i] = fact[i - 1] * i % P
    out = []
    for g in range(n):
        q = 1                       # coefficient n - 1 of Z / (X - g)
        acc = e[n - 1]
        for j in range(n - 1, 0, -1):
            q = (z[j] + g * q) % P  # coefficient j - 1
            acc = (acc + q * e[j - 1]) % P
        den = fact[g] * fact[n - 1 - g] % P
        if (n - 1 - g) & 1:
            den = P - den
        out.append(acc * pow(den, P - 2, P) % P)
    return tuple(out)


def _entries(M):
    """(gate, variable, coefficient) of a CSR matrix"""
    vals = bytes(M.val)
    for g in range(len(M.ptr) - 1):
        for t in range(int(M.ptr[g]), int(M.ptr[g + 1])):
            yield g, int(M.col[t]), int.from_bytes(vals[32 * t:32 * t + 32], "little")


def column_dots(circuit, M, dots):
    out = [0] * circuit.m
    for g, k, c in _entries(M):
        out[k] = (out[k] + c * dots[g]) % P
    return out


def split_pools(n, n_mid, ex1, ex2):
    assert len(ex1) == 3 + (n + 2) + (n - 1) + n_mid and len(ex2) == 2 + (n + 2)
    return dict(a=ex1[0], d1=ex1[1], b1=ex1[2], ti1=ex1[3:5 + n], tiztd=ex1[5 + n:4 + 2 * n], ltd=ex1[4 + 2 * n:], b2=ex2[0], d2=ex2[1], ti2=ex2[2:])


def key_check_mask(circuit, ex1, ex2, vk=None):
    n, m = circuit.n, circuit.m
    mids = [k for k in range(m) if circuit.mid[k]]
    ios = [k for k in range(m) if not circuit.mid[k]]
    K = split_pools(n, len(mids), [x % P for x in ex1], [x % P for x in ex2])
    ti1, ti2, g1, g2 = K["ti1"], K["ti2"], K["ti1"][0], K["ti2"][0]
    mask = 0
    if g1 != 1 or g2 != 1 or (vk and (vk["one1"] % P != 1 or vk["one2"] % P != 1)):
        mask |= GENERATORS
    if any(ti1[i + 1] * g2 % P != ti1[i] * ti2[1] % P for i in range(n + 1)):
        mask |= TAU_G1
    if any(ti1[i] * g2 % P != g1 * ti2[i] % P for i in range(n + 2)):
        mask |= TAU_G2
    if K["b1"] * g2 % P != g1 * K["b2"] % P:
        mask |= BETA
    if K["d1"] * g2 % P != g1 * K["d2"] % P or K["d1"] == 0 or K["d2"] == 0 or (vk and vk["d"] % P != K["d2"]):
        mask |= DELTA
    zz = sum(c * ti2[j] for j, c in enumerate(z_coeffs(n))) % P
    if any(K["tiztd"][i] * K["d2"] % P != ti1[i] * zz % P for i in range(n - 1)):
        mask |= H_BASES
    d1, d2 = basis_dots(n, ti1), basis_dots(n, ti2)
    V, W, Y = column_dots(circuit, circuit.L, d1), column_dots(circuit, circuit.R, d2), column_dots(circuit, circuit.O, d1)
    rhs = [(V[k] * K["b2"] + K["a"] * W[k] + Y[k] * g2) % P for k in range(m)]
    bad = any(K["ltd"][j] * K["d2"] % P != rhs[k] for j, k in enumerate(mids))
    if vk:
        assert len(vk["ltgm_io"]) == len(ios)
        bad = bad or any(vk["ltgm_io"][j] * vk["gm"] % P != rhs[k] for j, k in enumerate(ios))
        if vk["gm"] % P == 0:
            mask |= GAMMA
    if bad:
        mask |= L
    return mask


def honest_exponents(circuit, toxic):
    """groth16.ml:45-108 in exponents: (ex1, ex2, vk) of the key the setup makes from toxic = (alpha, beta, gamma, delta, tau)"""
    a, b, gm, d, t = (x % P for x in toxic)
    n, m = circuit.n, circuit.m
    pw = [pow(t, i, P) for i in range(n + 2)]
    dots = basis_dots(n, pw)                                     # l_g(tau)
    vk_, wk, yk = (column_dots(circuit, M, dots) for M in (circuit.L, circuit.R, circuit.O))
    Lk = [(b * vk_[k] + a * wk[k] + yk[k]) % P for k in range(m)]
    zt = 1
    for i in range(n):
        zt = zt * (t - i) % P
    dinv, ginv = pow(d, P - 2, P), pow(gm, P - 2, P)
    ex1 = [a, d, b] + pw + [pw[i] * zt % P * dinv % P for i in range(n - 1)] + [Lk[k] * dinv % P for k in range(m) if circuit.mid[k]]
    ex2 = [b, d] + pw
    vk = dict(one1=1, ltgm_io=[Lk[k] * ginv % P for k in range(m) if not circuit.mid[k]], one2=1, gm=gm, d=d)
    return ex1, ex2, vk


def names(mask):
    return [NAMES[b] for b in sorted(NAMES) if mask & b]
