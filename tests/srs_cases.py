"""Strings the string-check tests share (tests/test_srs_model.py on the CPU, tests/test_gpu_srs_*.py on the GPU) -- helpers and ONE table.  Every crafted
string stands here as exponents with the mask it must get WRITTEN OUT beside it: tests/test_srs_model.py holds tests/srs_model.py to the table, the
GPU tests hold the device to both.  Points are [exponent] G through the oracle (specialize_cases.srs_of_exponents), never the library under test."""
import functools

import specialize_cases as SC
import srs_model as M

R = SC.R
ALPHA, BETA, TAU = SC.ALPHA % R, SC.BETA % R, SC.TAU % R
OTHER = 0x0DDBA11 + (1 << 190)          # another tau / beta / scale
N1, NAB, N2 = 12, 6, 8                   # the crafted strings: every list end differs, tau1 runs past both others
D = 0xD1FF


def base():
    return [list(x) if isinstance(x, list) else x for x in M.honest(N1, NAB, N2, ALPHA, BETA, TAU)]


def _bump(which, index, d=1):
    def make():
        s = base()
        s[which][index] = (s[which][index] + d) % R
        return s
    return make


def _first_pair_alpha():
    t1, a1, b1, b2, t2 = base()          # alpha_tau1[i] scaled from index 1 on: only the pair (0, 1) disagrees
    return t1, [a1[0]] + [x * OTHER % R for x in a1[1:]], b1, b2, t2


def _first_pair_tau1():
    t1, a1, b1, b2, t2 = base()          # the same in tau1: pair (0, 1) alone in TAU_G1; tau2 and beta_tau1 then disagree with tau1 from index 1 on
    return [t1[0]] + [x * OTHER % R for x in t1[1:]], a1, b1, b2, t2


def _other_tau_g2():
    t1, a1, b1, b2, t2 = base()          # tau2 holds the powers of another tau: tau1 and alpha_tau1 no longer step by "the exponent of tau2[1]"
    return t1, a1, b1, b2, [pow(OTHER, i, R) for i in range(N2)]


def _other_tau_alpha():
    t1, a1, b1, b2, t2 = base()
    return t1, [ALPHA * pow(OTHER, i, R) % R for i in range(NAB)], b1, b2, t2


def _other_beta():
    t1, a1, b1, b2, t2 = base()
    return t1, a1, [OTHER * x % R for x in t1[:NAB]], b2, t2


def _generator_g1():
    t1, a1, b1, b2, t2 = base()          # every G1 list over [OTHER] G1: steps and beta hold, tau2 no longer matches tau1
    return [OTHER * x % R for x in t1], [OTHER * x % R for x in a1], [OTHER * x % R for x in b1], b2, t2


def _generator_g2():
    t1, a1, b1, b2, t2 = base()          # tau2 over [OTHER] G2: the exponent of tau2[1] is OTHER tau, so the steps of tau1 and alpha_tau1 fail with it
    return t1, a1, b1, b2, [OTHER * x % R for x in t2]


def _cancelling():
    """errors +D at pair 8 and -D at pair 10 of TAU_G1 (pair i: tau1[i+1] - tau tau1[i]), pair 9 kept whole by the matching multiple of tau: they
    cancel under equal coefficients, not under random ones.  All three indices lie past NAB and N2."""
    t1, a1, b1, b2, t2 = base()
    t1[9] = (t1[9] + D) % R
    t1[10] = (t1[10] + D * TAU) % R
    t1[11] = (t1[11] + D * TAU * TAU - D) % R
    pairs = [(t1[i + 1] - TAU * t1[i]) % R for i in range(N1 - 1)]
    assert pairs[8] == D and pairs[9] == 0 and pairs[10] == R - D and sum(pairs) % R == 0
    return t1, a1, b1, b2, t2


# name -> (maker of the exponent lists, the mask the check must give)
CRAFTED = {
    "last_tau1": (_bump(0, N1 - 1), M.TAU_G1),
    "last_alpha": (_bump(1, NAB - 1), M.ALPHA),
    "last_beta": (_bump(2, NAB - 1), M.BETA),
    "last_tau2": (_bump(4, N2 - 1), M.TAU_G2),
    "first_pair_alpha": (_first_pair_alpha, M.ALPHA),
    "first_pair_tau1": (_first_pair_tau1, M.TAU_G1 | M.TAU_G2 | M.BETA),
    "index1_beta": (_bump(2, 1), M.BETA),
    "index1_tau2": (_bump(4, 1), M.TAU_G1 | M.TAU_G2 | M.ALPHA),          # tau2[1] DEFINES tau
    "other_tau_g2": (_other_tau_g2, M.TAU_G1 | M.TAU_G2 | M.ALPHA),
    "other_tau_alpha": (_other_tau_alpha, M.ALPHA),
    "other_beta": (_other_beta, M.BETA),
    "generator_g1": (_generator_g1, M.GENERATORS | M.TAU_G2),
    "generator_g2": (_generator_g2, M.GENERATORS | M.TAU_G1 | M.TAU_G2 | M.ALPHA),
    "cancelling": (_cancelling, M.TAU_G1),
}
# degenerate trapdoors, honest strings of them: name -> ((alpha, beta, tau), mask)
DEGENERATE = {
    "tau_0": ((ALPHA, BETA, 0), M.TRIVIAL),
    "alpha_0": ((0, BETA, TAU), M.TRIVIAL),
    "beta_0": ((ALPHA, 0, TAU), M.TRIVIAL),
    "tau_1": ((ALPHA, BETA, 1), 0),
    "tau_minus_1": ((ALPHA, BETA, R - 1), 0),
}
# honest strings: free lengths (N1, NAB, N2), beside the exact sizes of n = 1, 2, 5, 64, 129; 257 and 65 points of tau1 cross a workgroup and a wave of the
# coefficient kernel with a ragged end
HONEST_N = (1, 2, 5, 64, 129)
HONEST_FREE = ((300, 7, 9), (2, 1, 2), (257, 3, 5), (65, 65, 65))
MUL = (0xA1FA0001 + (1 << 200), 0xBE7A0002 + (1 << 210), 0x7A0003 + (1 << 220))          # alpha', beta', tau' of the contribution tests


def crafted(name):
    return tuple(CRAFTED[name][0]())


@functools.lru_cache(maxsize=None)
def crafted_srs(name):
    return SC.srs_of_exponents(*crafted(name))


@functools.lru_cache(maxsize=None)
def honest_srs(n1, nab, n2, alpha=ALPHA, beta=BETA, tau=TAU):
    return SC.srs_of_exponents(*M.honest(n1, nab, n2, alpha, beta, tau))
