#!/usr/bin/env python3
"""The folded verifier against the per-proof verifier on one MI355X, in ONE process, on the same handle and the same proofs: host wall time of a whole
call, both PCIe copies and the call's own synchronisation included.

  zk_groth16_verify_resident | zk_groth16_verify_folded      counts 1, 16, 256, 4096, 16384
  keys: the README circuit's (2 public values), a random R1CS with 64 public values
  --protocol pinocchio: zk_pinocchio_verify_resident | zk_pinocchio_verify_folded on the same circuits' Pinocchio keys, five coefficients per proof

For every count the two calls ALTERNATE (resident, folded, resident, folded, ...) after one warm-up call of each shape; a figure is the best of three,
the spread of a row is the larger of (max - min) of the three timings of either call.  The baseline is the resident call of THIS run.  Outside the
timed region every answer is checked: all proofs good -> every ok and all_ok = 1; one proof replaced by a valid-looking wrong one -> all_ok = 0.
The kernel families' device times of both calls come from passes of their own at 256 and 4096 (profiling brackets every family with events and is
off while the wall times are taken).  rho is drawn from `secrets` once per shape, outside the timed region: drawing it is the caller's business.
"holds" records whether the folded call is faster than the resident call by more than the spread at 4096 and 16384 for both keys; it decides nothing
else -- the exit status is 0 either way, the record says which it was.
Usage: python scripts/bench_verify_fold.py [--protocol groth16|pinocchio] [--out profiles/verify_fold.json] [--quick]"""
import argparse
import ctypes as C
import json
import os
import secrets
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from zukelang_amd import _lib, r1cs as RC  # noqa: E402
from zukelang_amd import pinocchio as PIN  # noqa: E402
from zukelang_amd.groth16 import Groth16  # noqa: E402

FAMILIES = ["verify_point_checks", "msm_short", "pairing_miller", "pairing_final_exp", "verify_fold_scale", "verify_fold_scale_g2", "verify_fold_tree", "verify_fold_pow"]
MUST_WIN = (4096, 16384)
u8 = lambda b: C.cast(C.c_char_p(bytes(b)), _lib._P8) if len(b) else None


def alternate(call_a, call_b, reps=3):
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


def groth16_case(name, cs, wits, rng, st, counts, profile_counts):
    lib = _lib.lib()
    prover, _, vk = Groth16.generate(rng, cs)
    proofs = [prover.prove_rs(w, next(st), next(st)) for w in wits]
    prover.close()
    lt = bytes(np.ascontiguousarray(vk.ltgm_io, dtype=np.uint8))
    n_io = len(lt) // 96
    pr = [bytes(p.a) + bytes(p.b) + bytes(p.c) for p in proofs]
    io = [bytes(RC.fr_bytes([w[k] for k in range(cs.m) if not cs.mid[k]])) for w in wits]
    h = C.c_uint64(0)
    _lib.check(lib.zk_groth16_vk_upload(u8(vk.ab), u8(lt), n_io, u8(vk.gm), u8(vk.d), C.byref(h)))
    wrong = lambda p: p[:288] + p[:96]                                  # A in the place of C: a valid point, a wrong proof
    return measure(name, n_io, h, io, pr, wrong, 1, lib.zk_groth16_verify_resident, lib.zk_groth16_verify_folded, counts, profile_counts)


def pinocchio_case(name, cs, wits, rng, st, counts, profile_counts):
    lib = _lib.lib()
    prover, _, vk = PIN.ZK.generate(rng, cs)
    pr = [bytes(prover.prove(rng, w).to_bytes()) for w in wits]
    prover.close()
    g1, g2 = bytes(np.ascontiguousarray(vk.g1, dtype=np.uint8)), bytes(np.ascontiguousarray(vk.g2, dtype=np.uint8))
    n_io = len(g2) // 192 - 6
    io = [bytes(RC.fr_bytes([w[k] for k in range(cs.m) if not cs.mid[k]])) for w in wits]
    h = C.c_uint64(0)
    _lib.check(lib.zk_pinocchio_vk_upload(u8(g1), u8(g2), n_io, C.byref(h)))
    wrong = lambda p: p[:384] + p[:96] + p[480:]                        # vv in the place of h: a valid point, a wrong proof
    return measure(name, n_io, h, io, pr, wrong, 5, lib.zk_pinocchio_verify_resident, lib.zk_pinocchio_verify_folded, counts, profile_counts)


def measure(name, n_io, h, io, pr, wrong, coefficients, resident, folded, counts, profile_counts):
    """The rows and the kernel families of one key: `resident` and `folded` on handle h, `coefficients` of 16 bytes per proof"""
    lib = _lib.lib()

    def calls(count, broken=None):
        ios = b"".join(io[i % len(pr)] for i in range(count))
        prs = [pr[i % len(pr)] for i in range(count)]
        if broken is not None:
            prs[broken] = wrong(prs[broken])
        pall = b"".join(prs)
        rho = b"".join((secrets.token_bytes(15) + bytes([1 + secrets.randbelow(255)])) for _ in range(coefficients * count))
        ok_r, st_r, st_f, all_ok = (C.c_uint8 * count)(), (C.c_int32 * count)(), (C.c_int32 * count)(), C.c_int(-1)
        ar = (h, u8(ios), u8(pall), count, C.cast(ok_r, _lib._P8), st_r)
        af = (h, u8(ios), u8(pall), u8(rho), count, C.byref(all_ok), st_f)
        return (lambda: _lib.check(resident(*ar))), (lambda: _lib.check(folded(*af))), (ok_r, st_r), (all_ok, st_f)

    rows = []
    for count in counts:
        cr, cf, o_r, o_f = calls(count)
        tr, tf = alternate(cr, cf)
        assert list(o_r[0]) == [1] * count and list(o_r[1]) == [0] * count and o_f[0].value == 1 and list(o_f[1]) == [0] * count
        br, bf, ob_r, ob_f = calls(count, broken=count // 2)
        br(); bf()
        assert list(ob_r[0]) == [1] * (count // 2) + [0] + [1] * (count - count // 2 - 1) and ob_f[0].value == 0 and list(ob_f[1]) == [0] * count
        spread = max(max(tr) - min(tr), max(tf) - min(tf))
        rows.append({"count": count, "resident_ms": round(min(tr) * 1e3, 3), "folded_ms": round(min(tf) * 1e3, 3),
                     "resident_ms_all": [round(x * 1e3, 3) for x in tr], "folded_ms_all": [round(x * 1e3, 3) for x in tf], "spread_ms": round(spread * 1e3, 3),
                     "resident_over_folded": round(min(tr) / min(tf), 2), "folded_wins_by_more_than_spread": min(tr) - min(tf) > spread})
        print(name, rows[-1], flush=True)
    prof = {}
    for count in profile_counts:
        cr, cf, _, _ = calls(count)
        cr(); cf()
        prof[str(count)] = {"resident": profile_pass(cr), "folded": profile_pass(cf)}
    _lib.check(lib.zk_vk_free(h))
    return {"key": name, "n_io": n_io, "rows": rows, "kernel_families": prof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--protocol", choices=("groth16", "pinocchio"), default="groth16")
    ap.add_argument("--quick", action="store_true", help="small counts only (a rehearsal)")
    a = ap.parse_args()
    _lib.check(_lib.lib().zk_init(0))
    st = RC.fr_stream(0x5EED0F01)
    rng = lambda: next(st)
    counts, pcounts = ([1, 16, 256], [256]) if a.quick else ([1, 16, 256, 4096, 16384], [256, 4096])
    proto, case = a.protocol, groth16_case if a.protocol == "groth16" else pinocchio_case
    rec = {"what": "host wall ms of one zk_%s_verify_resident call next to one zk_%s_verify_folded call on the same handle and proofs (both PCIe " % (proto, proto) +
                   "copies), alternating in one process; best of three each, spread = the larger (max - min) of the three timings of either call; kernel "
                   "families: device ms from passes of their own",
           "device": "MI355X", proto: []}
    readme = [RC.readme_circuit(x) for x in range(3, 19)]
    rec[proto].append(case("README circuit", readme[0][0], [w for _, w in readme], rng, st, counts, pcounts))
    cs64, w64 = RC.random_r1cs(256, 512, 12)
    assert int((cs64.mid == 0).sum()) == 64
    rec[proto].append(case("random R1CS, 64 public values", cs64, [w64], rng, st, counts, pcounts))
    must = [r for c in rec[proto] for r in c["rows"] if r["count"] in MUST_WIN]
    rec["holds"] = {"folded_faster_than_resident_by_more_than_the_spread_at_4096_and_16384": bool(must) and all(r["folded_wins_by_more_than_spread"] for r in must)}
    if a.out:
        open(a.out, "w").write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({"holds": rec["holds"], "rows": {c["key"]: [(r["count"], r["resident_ms"], r["folded_ms"], r["spread_ms"]) for r in c["rows"]] for c in rec[proto]}}))


if __name__ == "__main__":
    main()
