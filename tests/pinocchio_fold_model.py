"""The folded Pinocchio equation of zk_pinocchio_verify_folded (include/zkmi355x.h) built from pyref's big-integer points: a helper, no tests in it.
tests/test_pinocchio_fold_model.py decides the equation with pyref's pairing (no device); tests/test_gpu_pinocchio_verify_folded.py holds the device's
ten sums and its GT value to what this builds.  Every proof given is taken as live.

  vk_g1 = one | aw | bgm | vv_io[n_io] | yy_io[n_io]      vk_g2 = one2 | av | ay | gm2 | bgm2 | yt | ww_io[n_io]
  proof = vv | ww (G2) | yy | h | vavv | waww (G2) | yayy | bvwy            rho: one row rho_0 .. rho_4 per proof"""
from oracle import pyref as P

R = P.R
G1_FIELDS = {"vv": 0, "yy": 288, "h": 384, "vavv": 480, "yayy": 768, "bvwy": 864}
G2_FIELDS = {"ww": 96, "waww": 576}
SUMS_G1 = ("S_av", "S_one2", "S_ay", "S_gm2", "S_bgm2", "S_yt", "S_yio")
SUMS_G2 = ("T_aw", "T_one", "T_bgm")


def proof_points(proof):
    """the eight points of a proof's 960 bytes by name"""
    pts = {f: P.g1_from_bytes(proof[o:o + 96]) for f, o in G1_FIELDS.items()}
    pts.update({f: P.g2_from_bytes(proof[o:o + 192]) for f, o in G2_FIELDS.items()})
    return pts


def proof_bytes(pts):
    return (P.g1_to_bytes(pts["vv"]) + P.g2_to_bytes(pts["ww"]) + P.g1_to_bytes(pts["yy"]) + P.g1_to_bytes(pts["h"]) + P.g1_to_bytes(pts["vavv"])
            + P.g2_to_bytes(pts["waww"]) + P.g1_to_bytes(pts["yayy"]) + P.g1_to_bytes(pts["bvwy"]))


def moved(proof, **by):
    """the proof with the named G1 points moved: moved(p, vavv=D, yayy=-D)"""
    pts = proof_points(proof)
    for f, d in by.items():
        pts[f] = P.pt_add(pts[f], d)
    return proof_bytes(pts)


def key_points(vk1, vk2):
    n_io = len(vk2) // 192 - 6
    g1 = [P.g1_from_bytes(vk1[96 * k:96 * k + 96]) for k in range(3 + 2 * n_io)]
    g2 = [P.g2_from_bytes(vk2[192 * k:192 * k + 192]) for k in range(6 + n_io)]
    key = dict(zip(("one", "aw", "bgm"), g1[:3]))
    key.update(zip(("one2", "av", "ay", "gm2", "bgm2", "yt"), g2[:6]))
    key.update(vv_io=g1[3:3 + n_io], yy_io=g1[3 + n_io:], ww_io=g2[6:])
    return key


def fold(vk1, vk2, ios, proofs, rho, mul=P.pt_mul_jac):
    """(sums_g1, sums_g2, pairs): the seven G1 sums and the three G2 sums by name (S_one2 the proofs' part alone), and the count + 9 pairs whose product
    of pairings is 1 exactly when the folded equation holds.  ios: one list of integers per proof.  mul(point, k), 0 <= k < r: every multiple is taken
    through it, the products over the public inputs too, so the caller may memoise it."""
    key = key_points(vk1, vk2)
    n_io = len(key["vv_io"])
    s = dict.fromkeys(SUMS_G1 + SUMS_G2)
    add = lambda name, pt: s.__setitem__(name, P.pt_add(s[name], pt))
    pairs = []

    def msm(points, scalars):
        acc = None
        for pt, k in zip(points, scalars):
            acc = P.pt_add(acc, mul(pt, k % R))
        return acc

    for io, proof, r in zip(ios, proofs, rho):
        assert len(io) == n_io and len(r) == 5
        p = proof_points(proof)
        vio, wio = msm(key["vv_io"], io), msm(key["ww_io"], io)
        pairs.append((mul(P.pt_add(vio, p["vv"]), r[4]), P.pt_add(wio, p["ww"])))
        add("S_av", mul(p["vv"], r[0]))
        for f, e in (("vavv", 0), ("yayy", 2), ("yy", 4)):
            add("S_one2", mul(p[f], r[e]))
        add("S_ay", mul(p["yy"], r[2]))
        add("S_gm2", mul(p["bvwy"], r[3]))
        add("S_bgm2", P.pt_add(mul(p["vv"], r[3]), mul(p["yy"], r[3])))
        add("S_yt", mul(p["h"], r[4]))
        add("T_aw", mul(p["ww"], r[1]))
        add("T_one", mul(p["waww"], r[1]))
        add("T_bgm", mul(p["ww"], r[3]))
    t = [sum(r[4] * io[k] for io, r in zip(ios, rho)) % R for k in range(n_io)]
    s["S_yio"] = msm(key["yy_io"], t)
    neg = P.pt_neg
    pairs += [(s["S_av"], key["av"]), (neg(P.pt_add(s["S_one2"], s["S_yio"])), key["one2"]), (s["S_ay"], key["ay"]), (s["S_gm2"], key["gm2"]),
              (neg(s["S_bgm2"]), key["bgm2"]), (neg(s["S_yt"]), key["yt"]),
              (key["aw"], s["T_aw"]), (neg(key["one"]), s["T_one"]), (neg(key["bgm"]), s["T_bgm"])]
    return {k: s[k] for k in SUMS_G1}, {k: s[k] for k in SUMS_G2}, pairs


def sums_bytes(sums_g1, sums_g2):
    """the hook's two outputs: 7 x 96 B and 3 x 192 B"""
    return b"".join(P.g1_to_bytes(sums_g1[k]) for k in SUMS_G1), b"".join(P.g2_to_bytes(sums_g2[k]) for k in SUMS_G2)


def pairs_bytes(pairs):
    return b"".join(P.g1_to_bytes(a) for a, _ in pairs), b"".join(P.g2_to_bytes(b) for _, b in pairs)
