"""The specification of zk_groth16_srs_check and zk_groth16_srs_contribute as an integer model on EXPONENTS: a string is [t1[i]] G1, [a1[i]] G1,
[b1[i]] G1, [b2] G2, [t2[i]] G2 -- whatever those exponents are, honest powers or not.  The check's mask is five predicates on them, exactly, with no
randomness; the contribution is a map on them.  No group, no device code, Python integers only."""
from zukelang_amd.r1cs import FR_MODULUS as P

GENERATORS, TAU_G1, TAU_G2, ALPHA, BETA, TRIVIAL = 1, 2, 4, 8, 16, 32
NAMES = {GENERATORS: "generators", TAU_G1: "tau_g1", TAU_G2: "tau_g2", ALPHA: "alpha", BETA: "beta", TRIVIAL: "trivial"}


def lengths_ok(n1, nab, n2):
    return n1 >= 2 and n2 >= 2 and nab >= 1 and nab <= n1 and n2 <= n1 and n1 <= 1 << 25


def mask(t1, a1, b1, b2, t2):
    """include/zkmi355x.h, ZK_SRSCHK_*: the relations that do NOT hold"""
    assert len(a1) == len(b1) and lengths_ok(len(t1), len(a1), len(t2))
    t1, a1, b1, t2 = ([x % P for x in e] for e in (t1, a1, b1, t2))
    b2 %= P
    tau = t2[1]
    f = 0
    if t1[0] != 1 or t2[0] != 1:
        f |= GENERATORS
    if any(t1[i + 1] != tau * t1[i] % P for i in range(len(t1) - 1)):
        f |= TAU_G1
    if any(t2[i] != t1[i] for i in range(len(t2))):
        f |= TAU_G2
    if any(a1[i + 1] != tau * a1[i] % P for i in range(len(a1) - 1)):
        f |= ALPHA
    if any(b1[i] != b2 * t1[i] % P for i in range(len(b1))):
        f |= BETA
    if tau == 0 or a1[0] == 0 or b2 == 0:
        f |= TRIVIAL
    return f


def honest(n1, nab, n2, alpha, beta, tau):
    """(t1, a1, b1, b2, t2) of the well-formed string of (alpha, beta, tau) at free lengths"""
    pw = [pow(tau, i, P) for i in range(max(n1, n2))]
    return pw[:n1], [alpha * x % P for x in pw[:nab]], [beta * x % P for x in pw[:nab]], beta % P, pw[:n2]


def contributed(t1, a1, b1, b2, t2, am, bm, tm):
    """the string times (alpha', beta', tau') = (am, bm, tm): a linear map, whatever the string"""
    pw = [pow(tm, i, P) for i in range(max(len(t1), len(t2)))]
    return ([x * pw[i] % P for i, x in enumerate(t1)], [x * am % P * pw[i] % P for i, x in enumerate(a1)], [x * bm % P * pw[i] % P for i, x in enumerate(b1)],
            b2 * bm % P, [x * pw[i] % P for i, x in enumerate(t2)])


def link(t1, a1, b1, after, am, bm, tm):
    """what a link shows, as exponents: (before, after) of tau1[1], alpha_tau1[0], beta_tau1[0] and the G2 factors tau', alpha', beta'"""
    return [t1[1] % P, after[0][1], a1[0] % P, after[1][0], b1[0] % P, after[2][0]], [tm % P, am % P, bm % P]
