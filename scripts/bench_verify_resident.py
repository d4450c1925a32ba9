#!/usr/bin/env python3
"""Resident verification keys against the batched verifiers on one MI355X, in ONE process: host wall time of a whole call, both PCIe copies included.

  zk_groth16_verify_many   | zk_groth16_verify_resident      counts 1, 16, 256, 4096   README circuit's key (2 public values), a key with 64 public values
  zk_pinocchio_verify_many | zk_pinocchio_verify_resident    counts 1, 16, 256, 1024   iterated_cubic(6, x) (2 public values)

For every count the two calls ALTERNATE (many, resident, many, resident, ...) after one warm-up call of each shape; a figure is the best of three, the
spread of a figure is the largest minus the smallest of those three timings of the same call.  Every verdict is checked to be true, and equal between
the two paths, outside the timed region; a batch with one broken proof must say so on both.  The record also holds the one-time cost of the upload,
the kernel families' device times of both paths from passes of their own at count 256 (the subgroup checks: pairing_point_checks of the _many call,
verify_point_checks of the resident one), and the smallest count of a doubling sweep at which the resident call beats that many single-proof host calls.
Two conditions are recorded under "holds" and decide the exit status: the resident call is faster than the _many call at every count by more than the
larger of the two spreads, and its verify_point_checks at 256 is below the _many call's pairing_point_checks.
Usage: python scripts/bench_verify_resident.py [--out profiles/verify_resident.json] [--quick]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from zukelang_amd import _lib, r1cs as RC, pinocchio as PIN  # noqa: E402
from zukelang_amd.groth16 import Groth16  # noqa: E402

FAMILIES = ["pairing_point_checks", "verify_point_checks", "pairing_miller", "pairing_final_exp", "msm_short"]
HOST_CALLS = 32
u8 = lambda b: C.cast(C.c_char_p(bytes(b)), _lib._P8) if len(b) else None


def alternate(call_a, call_b, reps=3):
    """(best, all timings) of each of two calls run in turn, after one warm-up of each"""
    call_a()
    call_b()
    ta, tb = [], []
    for _ in range(reps):
        for call, ts in ((call_a, ta), (call_b, tb)):
            t = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t)
    return ta, tb


def profile_pass(run):
    L = _lib.lib()
    _lib.check(L.zk_profile_enable(2))
    _lib.check(L.zk_profile_reset())
    run()
    out = {}
    for fam in FAMILIES:
        ms, cnt = C.c_double(), C.c_uint64()
        _lib.check(L.zk_profile_get(fam.encode(), C.byref(ms), C.byref(cnt)))
        if cnt.value:
            out[fam] = {"ms": round(ms.value, 3), "launches": cnt.value}
    _lib.check(L.zk_profile_enable(0))
    _lib.check(L.zk_profile_reset())
    return out


def timed_upload(upload):
    """seconds of the first upload of a key in this process and the best of three more; leaves the last handle"""
    ts, h = [], None
    for _ in range(4):
        if h is not None:
            _lib.check(_lib.lib().zk_vk_free(C.c_uint64(h)))
        t = time.perf_counter()
        h = upload()
        ts.append(time.perf_counter() - t)
    return h, {"first_ms": round(ts[0] * 1e3, 3), "best_of_3_ms": round(min(ts[1:]) * 1e3, 3)}


def case(name, n_io, proof_len, io, pr, many_args, many_fn, res_fn, upload, host_one, break_proof, counts, sweep_limit):
    lib = _lib.lib()
    h, up = timed_upload(upload)

    def calls(count, broken=None):
        ios = b"".join(io[i % len(pr)] for i in range(count))
        prs = [pr[i % len(pr)] for i in range(count)]
        if broken is not None:
            prs[broken] = break_proof(prs[broken])
        pall = b"".join(prs)
        ok_m, ok_r = (C.c_uint8 * count)(), (C.c_uint8 * count)()
        st_m, st_r = (C.c_int32 * count)(), (C.c_int32 * count)()
        am = many_args + (u8(ios), u8(pall), count, C.cast(ok_m, _lib._P8), st_m)
        ar = (C.c_uint64(h), u8(ios), u8(pall), count, C.cast(ok_r, _lib._P8), st_r)
        return (lambda: _lib.check(getattr(lib, many_fn)(*am))), (lambda: _lib.check(getattr(lib, res_fn)(*ar))), (ok_m, st_m), (ok_r, st_r)

    rows = []
    for count in counts:
        cm, cr, om, orr = calls(count)
        tm, tr = alternate(cm, cr)
        assert list(om[0]) == [1] * count == list(orr[0]) and list(om[1]) == [0] * count == list(orr[1])
        if count > 1:
            bm, br, obm, obr = calls(count, broken=count // 2)
            bm(); br()
            assert list(obm[0]) == [1] * (count // 2) + [0] + [1] * (count - count // 2 - 1) == list(obr[0])
        spread = max(max(tm) - min(tm), max(tr) - min(tr))
        rows.append({"count": count, "many_ms": round(min(tm) * 1e3, 3), "resident_ms": round(min(tr) * 1e3, 3),
                     "many_ms_all": [round(x * 1e3, 3) for x in tm], "resident_ms_all": [round(x * 1e3, 3) for x in tr], "spread_ms": round(spread * 1e3, 3),
                     "many_over_resident": round(min(tm) / min(tr), 2), "resident_wins_by_more_than_spread": min(tm) - min(tr) > spread})
        print(name, rows[-1], flush=True)
    # against the single-proof host calls
    t = time.perf_counter()
    for i in range(HOST_CALLS):
        host_one(i)
    host_per = (time.perf_counter() - t) / HOST_CALLS
    first, sw, c = None, [], 1
    while c <= sweep_limit:
        _, cr, _, _ = calls(c)
        cr()
        ts = []
        for _ in range(2):
            t = time.perf_counter()
            cr()
            ts.append(time.perf_counter() - t)
        sw.append({"count": c, "resident_ms": round(min(ts) * 1e3, 3), "host_ms": round(host_per * c * 1e3, 3)})
        if first is None and min(ts) < host_per * c:
            first = c
        c *= 2
    cm, cr, _, _ = calls(256)
    prof = {"many": profile_pass(cm), "resident": profile_pass(cr)}
    _lib.check(lib.zk_vk_free(C.c_uint64(h)))
    pc, vc = prof["many"]["pairing_point_checks"]["ms"], prof["resident"]["verify_point_checks"]["ms"]
    return {"key": name, "n_io": n_io, "upload": up, "rows": rows, "host_ms_per_call": round(host_per * 1e3, 3), "smallest_count_device_wins": first, "sweep": sw,
            "kernel_families_at_256": prof, "point_checks_at_256": {"many_pairing_point_checks_ms": pc, "resident_verify_point_checks_ms": vc,
                                                                   "ratio": round(pc / vc, 2) if vc else None, "resident_is_below": vc < pc}}


def groth16_case(name, cs, wits, rng, st, counts):
    lib = _lib.lib()
    prover, _, vk = Groth16.generate(rng, cs)
    proofs = [prover.prove_rs(w, next(st), next(st)) for w in wits]
    prover.close()
    lt = bytes(np.ascontiguousarray(vk.ltgm_io, dtype=np.uint8))
    n_io = len(lt) // 96
    pr = [bytes(p.a) + bytes(p.b) + bytes(p.c) for p in proofs]
    io = [bytes(RC.fr_bytes([w[k] for k in range(cs.m) if not cs.mid[k]])) for w in wits]

    def upload():
        h = C.c_uint64(0)
        _lib.check(lib.zk_groth16_vk_upload(u8(vk.ab), u8(lt), n_io, u8(vk.gm), u8(vk.d), C.byref(h)))
        return h.value

    def host_one(i):
        ok = C.c_int(0)
        _lib.check(lib.zk_groth16_verify(vk.ab, u8(lt), u8(io[i % len(pr)]), C.c_size_t(n_io), vk.gm, vk.d, pr[i % len(pr)], C.byref(ok)))
        assert ok.value == 1

    return case(name, n_io, 384, io, pr, (u8(vk.ab), u8(lt), n_io, u8(vk.gm), u8(vk.d)), "zk_groth16_verify_many", "zk_groth16_verify_resident", upload, host_one,
                lambda p: p[:288] + p[:96], counts, 256)          # A in the place of C: a valid point, a wrong proof


def pinocchio_case(cs, wits, rng, counts):
    lib = _lib.lib()
    prover, _, vk = PIN.ZK.generate(rng, cs)
    pr = [prover.prove(rng, w).to_bytes() for w in wits]
    prover.close()
    g1, g2 = bytes(np.ascontiguousarray(vk.g1, dtype=np.uint8)), bytes(np.ascontiguousarray(vk.g2, dtype=np.uint8))
    io = [bytes(RC.fr_bytes([w[k] for k in range(cs.m) if not cs.mid[k]])) for w in wits]
    n_io = len(io[0]) // 32

    def upload():
        h = C.c_uint64(0)
        _lib.check(lib.zk_pinocchio_vk_upload(u8(g1), u8(g2), n_io, C.byref(h)))
        return h.value

    def host_one(i):
        ok = C.c_int(0)
        _lib.check(lib.zk_pinocchio_verify(g1, g2, u8(io[i % len(io)]), C.c_size_t(n_io), pr[i % len(io)], C.byref(ok)))
        assert ok.value == 1

    return case("iterated_cubic(6)", n_io, 960, io, pr, (u8(g1), u8(g2), n_io), "zk_pinocchio_verify_many", "zk_pinocchio_verify_resident", upload, host_one,
                lambda p: p[:384] + p[:96] + p[480:], counts, 64)          # vv in the place of h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small counts only (a rehearsal)")
    a = ap.parse_args()
    _lib.check(_lib.lib().zk_init(0))
    st = RC.fr_stream(0x5EED0B17)
    rng = lambda: next(st)
    g_counts, p_counts = ([1, 16, 256], [1, 16, 256]) if a.quick else ([1, 16, 256, 4096], [1, 16, 256, 1024])
    rec = {"what": "host wall ms of one zk_*_verify_many call next to one zk_*_verify_resident call on the same key and proofs (both PCIe copies), "
                   "alternating in one process; best of three each, spread = max - min of the three timings of one call",
           "device": "MI355X", "groth16": []}
    readme = [RC.readme_circuit(x) for x in range(3, 19)]
    rec["groth16"].append(groth16_case("README circuit", readme[0][0], [w for _, w in readme], rng, st, g_counts))
    cs64, w64 = RC.random_r1cs(256, 512, 12)
    assert int((cs64.mid == 0).sum()) == 64
    rec["groth16"].append(groth16_case("random R1CS, 64 public values", cs64, [w64], rng, st, g_counts))
    cub = [RC.iterated_cubic(6, x) for x in range(9, 25)]
    rec["pinocchio"] = pinocchio_case(cub[0][0], [w for _, w in cub], rng, p_counts)
    cases = rec["groth16"] + [rec["pinocchio"]]
    rec["holds"] = {"resident_faster_at_every_count_by_more_than_the_spread": all(r["resident_wins_by_more_than_spread"] for c in cases for r in c["rows"]),
                    "verify_point_checks_below_pairing_point_checks_at_256": all(c["point_checks_at_256"]["resident_is_below"] for c in cases)}
    if a.out:
        open(a.out, "w").write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({"holds": rec["holds"], "point_checks_at_256": {c["key"]: c["point_checks_at_256"] for c in cases},
                      "smallest_count_device_wins": {c["key"]: c["smallest_count_device_wins"] for c in cases}}))
    if not all(rec["holds"].values()):
        sys.exit("a condition is missed: see \"holds\" and the rows")


if __name__ == "__main__":
    main()
