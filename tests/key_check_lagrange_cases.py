"""Crafted Lagrange-form Groth16 keys for zk_groth16_key_check_lagrange, as edited exponent lists: one edit each of the honest key of `toxic`
(key_check_lagrange_model.honest_lagrange_exponents).  Shared by tests/test_key_check_lagrange_model.py (model against hand-derived bits, no GPU) and
tests/test_gpu_key_check_lagrange.py (device against model).  Every case is (name, lx1, lx2, vk); BITS holds the hand-derived masks, without and
with a verification key, for circuits in which the moved points carry a coefficient of some mid variable (the README circuit, the random families)
and a tau outside both domains."""
from key_check_lagrange_model import BETA, DELTA, GAMMA, GENERATORS, H_BASES, L, TAU_G1, TAU_G2, P, basis_at, honest_lagrange_exponents, inv

OTHER = 0x1234567      # what "another" tau / delta differs by; the D of the +D / -D pairs


def crafted(circuit, toxic, other_circuit=None):
    a, b, gm, d, t = (x % P for x in toxic)
    n, n_mid = circuit.n, sum(1 for x in circuit.mid if x)
    lx1, lx2, vk = honest_lagrange_exponents(circuit, toxic)
    L1, HL, LT, L2 = 3, 3 + n, 2 + 2 * n, 2

    def edit(**kw):
        e1, e2, v = list(lx1), list(lx2), dict(vk, ltgm_io=list(vk["ltgm_io"]))
        for pos, val in kw.get("g1", {}).items():
            e1[pos] = val % P
        for pos, val in kw.get("g2", {}).items():
            e2[pos] = val % P
        for key, val in kw.get("vk", {}).items():
            v[key] = val
        return e1, e2, v

    def both(basis):
        return edit(g1={L1 + i: x for i, x in enumerate(basis)}, g2={L2 + i: x for i, x in enumerate(basis)})

    out = [("honest", *edit())]
    if n >= 2:
        out.append(("l1_opposite", *edit(g1={L1: lx1[L1] + OTHER, L1 + 1: lx1[L1 + 1] - OTHER})))
        out.append(("l2_one", *edit(g2={L2 + 1: lx2[L2 + 1] + OTHER})))
        out.append(("l_other_tau", *both(basis_at(0, n, t + OTHER))))
        out.append(("l_domain_from_one", *both(basis_at(1, n, t))))
    if n >= 3:
        # the basis of 0 .. n-2, n at tau: l'_i = l_i (tau - n) / (i - n) * (i - (n-1)) / (tau - (n-1)) for i < n - 1; the last one makes the sum 1
        den = inv(t - (n - 1))
        gap = [lx1[L1 + i] * (t - n) % P * inv(i - n) % P * (i - (n - 1)) % P * den % P for i in range(n - 1)]
        gap.append((1 - sum(gap)) % P)
        out.append(("l_gapped_domain", *both(gap)))
    out.append(("l1_doubled", *edit(g1={L1 + i: 2 * lx1[L1 + i] for i in range(n)})))
    if n >= 2:
        out.append(("hl_one", *edit(g1={HL + n - 2: lx1[HL + n - 2] + 1})))
        scale = d * inv(d + OTHER) % P
        out.append(("hl_other_delta", *edit(g1={HL + i: lx1[HL + i] * scale for i in range(n - 1)})))
    if n >= 3:
        out.append(("hl_opposite", *edit(g1={HL: lx1[HL] + OTHER, HL + 1: lx1[HL + 1] - OTHER})))
    if n_mid >= 1:
        out.append(("ltd_mid_one", *edit(g1={LT + n_mid - 1: lx1[LT + n_mid - 1] + 1})))
    if n_mid >= 2:
        out.append(("ltd_mid_opposite", *edit(g1={LT: lx1[LT] + OTHER, LT + 1: lx1[LT + 1] - OTHER})))
    if other_circuit is not None:
        o1, _, _ = honest_lagrange_exponents(other_circuit, toxic)
        out.append(("ltd_mid_other_circuit", *edit(g1={LT + j: o1[LT + j] for j in range(n_mid)})))
    out.append(("b1_other", *edit(g1={2: b + OTHER})))
    out.append(("d1_other", *edit(g1={1: d + OTHER})))
    out.append(("vk_d_other", *edit(vk={"d": (d + OTHER) % P})))
    out.append(("vk_gm_zero", *edit(vk={"gm": 0})))
    out.append(("vk_one2_two", *edit(vk={"one2": 2})))
    return out


# name -> (mask without a verification key, mask with it), derived by hand from the relations of include/zkmi355x.h:
BITS = {
    "honest": (0, 0),
    # the sum is kept, so GENERATORS holds; l1[0], l1[1] no longer match l2; d_0 and d_1 move, d_(n-1) does not (n >= 3), or move by (-D tau, -D (1 - tau))
    # against w = (-1, 1) (n = 2): not proportional; sum i lambda_t(i) l1[i] moves by -D lambda_t(1) != 0; V and Y read l1[0], l1[1]
    "l1_opposite": (TAU_G1 | TAU_G2 | H_BASES | L,) * 2,
    # g2 = 1 + D: every relation that pairs with g2 (TAU_G2, BETA, DELTA, Y in L) sees it; T2 = tau + D; the h bases are paired with d2 and l2[0] only
    "l2_one": (GENERATORS | TAU_G1 | TAU_G2 | BETA | DELTA | L,) * 2,
    # a well-formed basis, of another point: only what was made at tau disagrees
    "l_other_tau": (H_BASES | L,) * 2,
    # the basis of 1..n at tau IS the basis of 0..n-1 at tau - 1 (l_i(X - 1)): every arithmetic progression is a well-formed basis at ONE point, so
    # TAU_G1 holds -- as it must: the relation says "the Lagrange basis at one point", not "at the tau of hl" -- and H_BASES and L catch it
    "l_domain_from_one": (H_BASES | L,) * 2,
    # a domain that is no arithmetic progression (0..n-2, n): sums to 1, l1 = l2, and no basis of 0..n-1 at any point
    "l_gapped_domain": (TAU_G1 | H_BASES | L,) * 2,
    # g1 = 2: l1[i] g2 = g1 l2[i] still holds, d stays proportional to w; b1 g2 != g1 b2, d1 g2 != g1 d2; S, V and Y double
    "l1_doubled": (GENERATORS | BETA | DELTA | H_BASES | L,) * 2,
    "hl_one": (H_BASES,) * 2,
    "hl_other_delta": (H_BASES,) * 2,
    "hl_opposite": (H_BASES,) * 2,                            # cancels in a plain sum, not under the bijection pi -> sigma
    "ltd_mid_one": (L,) * 2,
    "ltd_mid_opposite": (L,) * 2,                             # cancels in a plain sum, not under independent mu_k
    "ltd_mid_other_circuit": (L,) * 2,                        # the changed coefficient belongs to a mid variable
    "b1_other": (BETA,) * 2,                                  # b1 is in no other relation: L pairs with b2
    "d1_other": (DELTA,) * 2,                                 # hl and ltd_mid are paired with d2
    "vk_d_other": (0, DELTA),
    "vk_gm_zero": (0, GAMMA | L),                             # ltgm_io gm = 0 is no L_k
    "vk_one2_two": (0, GENERATORS),
}


def honest_inside_domain(circuit, toxic, tau=2):
    """an honest key whose tau is a point of the domain 0..n-1: l1 and l2 are unit vectors, Z(tau) = 0 and every hl is the identity"""
    return honest_lagrange_exponents(circuit, list(toxic[:4]) + [tau])
