"""A Pinocchio verification key and proofs built from chosen exponents, for any number of public inputs (no circuit is involved: every key and proof
point is a chosen multiple of a generator, and the proof's remaining scalars are solved from the five equations of Verify.f, pinocchio.ml:254-420, in
Python integers).  tests/test_pairing_host.py holds the construction to zk_pinocchio_verify; tests/test_gpu_verify_many.py gives it to the batched
verifier with more public inputs than one narrow table of the short products holds.

  vk_g1 = one | aw | bgm | vv_io[n_io] | yy_io[n_io]      vk_g2 = one2 | av | ay | gm2 | bgm2 | yt | ww_io[n_io]      one = G1, one2 = gm2 = yt = G2
  proof = vv | ww (G2) | yy | h | vavv | waww (G2) | yayy | bvwy
  vavv = av vv    waww = aw ww    yayy = ay yy    bvwy = bgm2 (vv + yy) + bgm ww    h = (vio + vv)(wio + ww) - (yio + yy)
with vio = sum_k w_k vv_io_k and so on.  The IO lists hold TWO distinct points each -- the first below index `split`, the second from there on -- and
the public inputs are w_k = k + 1: a sum that reads a wrong point or a wrong scalar is another sum."""
from oracle import pyref as P

R = P.R
SPLIT = 8192          # the points of an IO list change here (the length of one narrow table); a shorter list changes at its last point
AV, AW, AY, BGM, BGM2 = 3, 5, 7, 11, 13
VV_IO, YY_IO, WW_IO = (17, 19), (23, 29), (31, 37)
VV, WW, YY = 41, 43, 47

g1 = lambda k: P.g1_to_bytes(P.pt_mul(P.G1, k % R))
g2 = lambda k: P.g2_to_bytes(P.pt_mul(P.G2, k % R))


def public_inputs(n_io):
    return [k + 1 for k in range(n_io)]


def key(n_io):
    """(vk_g1, vk_g2) for n_io public inputs"""
    split = min(SPLIT, n_io - 1)
    blocks = lambda enc, pair: enc(pair[0]) * split + enc(pair[1]) * (n_io - split)
    vk1 = g1(1) + g1(AW) + g1(BGM) + blocks(g1, VV_IO) + blocks(g1, YY_IO)
    vk2 = g2(1) + g2(AV) + g2(AY) + g2(1) + g2(BGM2) + g2(1) + blocks(g2, WW_IO)
    return vk1, vk2


def proof(n_io, io=None):
    """The 960 bytes of the proof that verifies under key(n_io) with the public inputs `io` (public_inputs(n_io) when None)"""
    io = public_inputs(n_io) if io is None else io
    split = min(SPLIT, n_io - 1)
    dot = lambda pair: sum(w * (pair[0] if k < split else pair[1]) for k, w in enumerate(io)) % R
    vio, yio, wio = dot(VV_IO), dot(YY_IO), dot(WW_IO)
    h = ((vio + VV) * (wio + WW) - (yio + YY)) % R
    bvwy = (BGM2 * (VV + YY) + BGM * WW) % R
    return g1(VV) + g2(WW) + g1(YY) + g1(h) + g1(AV * VV) + g2(AW * WW) + g1(AY * YY) + g1(bvwy)


def ww_off_the_curve(pr):
    """`pr` with the last byte of ww's y changed: the same x with another y that is not its negative is no point of the twist"""
    bad = bytearray(pr)
    bad[287] ^= 1
    return bytes(bad)
