"""Crafted Groth16 keys for the key check, as edited exponent lists: one edit each of the honest key of `toxic` (key_check_model.honest_exponents).
Shared by tests/test_key_check_model.py (model against hand-derived bits, no GPU) and tests/test_gpu_key_check.py (device against model).
Every case is (name, ex1, ex2, vk); BITS holds the hand-derived masks, with and without a verification key, for circuits in which every tau power
below n carries a coefficient of some v_k or y_k (the README circuit, the random families)."""
from key_check_model import BETA, DELTA, H_BASES, L, TAU_G1, TAU_G2, P, honest_exponents

OTHER = 0x1234567      # what "another" tau / beta / gamma / delta differs by


def crafted(circuit, toxic, other_circuit=None):
    a, b, gm, d, t = (x % P for x in toxic)
    n, n_mid = circuit.n, sum(1 for x in circuit.mid if x)
    ex1, ex2, vk = honest_exponents(circuit, toxic)
    TI1, TZ, LT, TI2 = 3, 5 + n, 4 + 2 * n, 2

    def edit(**kw):
        e1, e2, v = list(ex1), list(ex2), dict(vk, ltgm_io=list(vk["ltgm_io"]))
        for pos, val in kw.get("g1", {}).items():
            e1[pos] = val % P
        for pos, val in kw.get("g2", {}).items():
            e2[pos] = val % P
        for key, val in kw.get("vk", {}).items():
            v[key] = val
        return e1, e2, v

    out = [("honest", *edit())]
    out.append(("ti1_last", *edit(g1={TI1 + n + 1: ex1[TI1 + n + 1] + 1})))
    if n >= 3:
        out.append(("ti1_middle", *edit(g1={TI1 + 1: ex1[TI1 + 1] + 1})))
    t2 = (t + OTHER) % P
    out.append(("ti2_other_tau", *edit(g2={TI2 + i: pow(t2, i, P) for i in range(n + 2)})))
    out.append(("b2_other_beta", *edit(g2={0: b + OTHER})))
    out.append(("d2_other_delta", *edit(g2={1: d + OTHER})))
    if n >= 2:
        scale = d * pow((d + OTHER) % P, P - 2, P) % P
        out.append(("tiztd_other_delta", *edit(g1={TZ + i: ex1[TZ + i] * scale for i in range(n - 1)})))
        out.append(("tiztd_one", *edit(g1={TZ + n - 2: ex1[TZ + n - 2] + 1})))
    if n_mid >= 1:
        out.append(("ltd_mid_one", *edit(g1={LT + n_mid - 1: ex1[LT + n_mid - 1] + 1})))
    if n_mid >= 2:
        out.append(("ltd_mid_opposite", *edit(g1={LT: ex1[LT] + OTHER, LT + 1: ex1[LT + 1] - OTHER})))
    if other_circuit is not None:
        o1, o2, ov = honest_exponents(other_circuit, toxic)
        out.append(("other_circuit", o1, o2, ov))
    out.append(("vk_gm_other_gamma", *edit(vk={"gm": (gm + OTHER) % P})))
    out.append(("vk_d_other", *edit(vk={"d": (d + OTHER) % P})))
    lt = list(vk["ltgm_io"])
    lt[-1] = (lt[-1] + 1) % P
    out.append(("vk_ltgm_io_one", *edit(vk={"ltgm_io": lt})))
    out.append(("delta_zero", *edit(g1={1: 0}, g2={1: 0})))
    return out


# name -> (mask without a verification key, mask with it), derived by hand from the relations of include/zkmi355x.h:
BITS = {
    "honest": (0, 0),
    "ti1_last": (TAU_G1 | TAU_G2,) * 2,                       # ti1[n+1] is in no other relation: h bases read i < n-1, V and Y read i < n
    "ti1_middle": (TAU_G1 | TAU_G2 | H_BASES | L,) * 2,       # tiztd[1] no longer matches ti1[1]; V and Y read ti1[1]
    "ti2_other_tau": (TAU_G1 | TAU_G2 | H_BASES | L,) * 2,    # ti2[1] is the tau of TAU_G1; <ti2, Z> = Z(tau'); W reads ti2
    "b2_other_beta": (BETA | L,) * 2,                         # e(V, b2)
    "d2_other_delta": (DELTA | H_BASES | L,) * 2,             # tiztd and ltd_mid are paired with d2; vk.d != d2 is DELTA again
    "tiztd_other_delta": (H_BASES,) * 2,
    "tiztd_one": (H_BASES,) * 2,
    "ltd_mid_one": (L,) * 2,
    "ltd_mid_opposite": (L,) * 2,                             # cancels in a plain sum, not under independent mu_k
    "other_circuit": (L,) * 2,                                # when the changed coefficient belongs to a mid variable; else (0, L)
    "vk_gm_other_gamma": (0, L),                              # ltgm_io still holds L_k / gamma
    "vk_d_other": (0, DELTA),
    "vk_ltgm_io_one": (0, L),
    "delta_zero": (DELTA | H_BASES | L,) * 2,
}
