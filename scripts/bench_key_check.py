#!/usr/bin/env python3
"""What zk_groth16_key_check costs: host wall time of Groth16.check_key with a verification key on a tau-power handle, on one MI355X, best of
--repeats, at Groth16 2^16 and 2^20 constraints (iterated cubic).  In the same run, as context: one blocking zk_groth16_prove on the same handle
(best of the same number) and the handle's upload from compressed wire bytes (Groth16.from_compressed, to a handle).  Then, in a run of its own
under zk_profile_enable(2), the device time of ONE check by timer family (zk_profile_get; the check's own launches are the family key_check).

The claim under test is "a check costs a small multiple of one proof": the JSON holds both figures and their ratio, whatever it is.
(zk_groth16_key_check_lagrange has a script of its own, scripts/bench_key_check_lagrange.py, which times both calls side by side.)

    python scripts/bench_key_check.py --out profiles/key_check.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zukelang_amd import _lib, r1cs as RC               # noqa: E402
from zukelang_amd.curve import G1, G2                   # noqa: E402
from zukelang_amd.groth16 import Groth16                # noqa: E402


def families():
    L = _lib.lib()
    buf = C.create_string_buffer(1 << 14)
    _lib.check(L.zk_profile_names(buf, C.c_size_t(len(buf))))
    out = {}
    for f in filter(None, buf.value.decode().split(",")):
        ms, cnt = C.c_double(), C.c_uint64()
        _lib.check(L.zk_profile_get(f.encode(), C.byref(ms), C.byref(cnt)))
        if cnt.value:
            out[f] = {"ms": round(ms.value, 3), "launches": cnt.value}
    return out


def best(fn, repeats):
    L = _lib.lib()
    ts = []
    for _ in range(repeats):
        _lib.check(L.zk_sync())
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"best_ms": round(1e3 * min(ts), 3), "all_ms": [round(1e3 * t, 3) for t in ts]}


def measure(log_n, repeats):
    L = _lib.lib()
    n = 1 << log_n
    cs, w = RC.iterated_cubic(n, 0xC0FFEE)
    st = RC.fr_stream(0x5EED0000 + log_n)
    prover, pk, vk = Groth16.generate(lambda: next(st), cs, form="tau_powers")
    r, s = next(st), next(st)
    wb = prover._sol_bytes(w)
    res = prover.check_key(vk)          # warm-up: workspaces, module load -- and the verdict
    if not res.ok:
        raise SystemExit("2^%d: the generated key fails its own check: %s" % (log_n, res.names))
    prover.prove_rs(wb, r, s)
    out = {"constraints": n, "variables": cs.m, "g1_points": len(pk.g1) // 96, "g2_points": len(pk.g2) // 192}
    out["check_key_with_vkey"] = best(lambda: prover.check_key(vk), repeats)
    out["check_key_without_vkey"] = best(lambda: prover.check_key(), repeats)
    out["prove_blocking"] = best(lambda: prover.prove_rs(wb, r, s), repeats)
    out["check_over_prove"] = round(out["check_key_with_vkey"]["best_ms"] / out["prove_blocking"]["best_ms"], 2)
    # one check alone under the per-family timers (they serialise the launches: not the wall time above)
    _lib.check(L.zk_profile_enable(2))
    _lib.check(L.zk_profile_reset())
    prover.check_key(vk)
    _lib.check(L.zk_sync())
    out["device_ms_by_family_one_check"] = families()
    _lib.check(L.zk_profile_reset())
    prover.prove_rs(wb, r, s)
    _lib.check(L.zk_sync())
    out["device_ms_by_family_one_proof"] = families()
    _lib.check(L.zk_profile_enable(0))
    prover.close()
    g1w, g2w = G1.to_compressed_bytes_many(bytes(pk.g1)), G2.to_compressed_bytes_many(bytes(pk.g2))
    ts = []
    for i in range(repeats + 1):          # the first is a warm-up
        _lib.check(L.zk_sync())
        t0 = time.perf_counter()
        p = Groth16.from_compressed(cs, g1w, g2w)
        if i:
            ts.append(time.perf_counter() - t0)
        p.close()
    out["upload_compressed"] = {"best_ms": round(1e3 * min(ts), 3), "all_ms": [round(1e3 * t, 3) for t in ts]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_check.json"))
    ap.add_argument("--log-n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    _lib.check(_lib.lib().zk_init(0))
    doc = {"how": "python scripts/bench_key_check.py (host wall time, best of %d; one MI355X)" % a.repeats,
           "see_also": "zk_groth16_key_check_lagrange: scripts/bench_key_check_lagrange.py -> profiles/key_check_lagrange.json", "sizes": {}}
    for log_n in a.log_n:
        doc["sizes"]["2^%d" % log_n] = measure(log_n, a.repeats)
        print("2^%d:" % log_n, json.dumps({k: (v["best_ms"] if isinstance(v, dict) and "best_ms" in v else v) for k, v in doc["sizes"]["2^%d" % log_n].items()
                                            if not k.startswith("device_")}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
