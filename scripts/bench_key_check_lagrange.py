#!/usr/bin/env python3
"""What zk_groth16_key_check_lagrange costs: host wall time of Groth16.check_lagrange_key on a Lagrange-form handle, with and without a verification
key, on one MI355X, at Groth16 2^16 and 2^20 constraints (iterated cubic).  In the same process and on the same key, ALTERNATING round by round so
that drift hits every figure alike, best of --repeats:
  - zk_groth16_key_check on the tau-power form of that key (the reference point: the same shape of products and pairings, plus a basis conversion);
  - one blocking zk_groth16_prove on the Lagrange-form handle;
then the load the check follows in a key cache: Groth16.from_compressed(lagrange=True) of the handle's own pools in wire form.  Last, in a run of its
own under zk_profile_enable(2), the device time of ONE check by timer family.

    python scripts/bench_key_check_lagrange.py --out profiles/key_check_lagrange.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_key_check import families                    # noqa: E402
from zukelang_amd import _lib, r1cs as RC               # noqa: E402
from zukelang_amd.groth16 import Groth16                # noqa: E402


def timed(fn):
    _lib.check(_lib.lib().zk_sync())
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def summary(ts):
    return {"best_ms": round(1e3 * min(ts), 3), "all_ms": [round(1e3 * t, 3) for t in ts]}


def measure(log_n, repeats):
    L = _lib.lib()
    n = 1 << log_n
    cs, w = RC.iterated_cubic(n, 0xC0FFEE)
    st = RC.fr_stream(0x5EED0000 + log_n)
    toxic = [next(st) for _ in range(5)]
    r, s = next(st), next(st)
    it = iter(toxic)
    powers, pk, vk = Groth16.generate(lambda: next(it), cs, form="tau_powers")
    it = iter(toxic)
    lag, _, _ = Groth16.generate(lambda: next(it), cs, form="lagrange")
    wb = lag._sol_bytes(w)
    for res, what in ((lag.check_lagrange_key(vk), "Lagrange-form"), (powers.check_key(vk), "tau-power")):          # warm-up -- and the verdicts
        if not res.ok:
            raise SystemExit("2^%d: the generated %s key fails its own check: %s" % (log_n, what, res.names))
    lag.check_lagrange_key()
    lag.prove_rs(wb, r, s)
    runs = {
        "check_lagrange_with_vkey": lambda: lag.check_lagrange_key(vk),
        "check_lagrange_without_vkey": lambda: lag.check_lagrange_key(),
        "check_tau_powers_with_vkey": lambda: powers.check_key(vk),
        "prove_blocking_lagrange": lambda: lag.prove_rs(wb, r, s),
    }
    ts = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            ts[k].append(timed(fn))
    out = {"constraints": n, "variables": cs.m, "g1_points": len(pk.g1) // 96, "g2_points": len(pk.g2) // 192}
    out.update({k: summary(v) for k, v in ts.items()})
    tau = ts["check_tau_powers_with_vkey"]
    out["tau_powers_spread_ms"] = round(1e3 * (max(tau) - min(tau)), 3)
    out["lagrange_minus_tau_powers_ms"] = round(out["check_lagrange_with_vkey"]["best_ms"] - out["check_tau_powers_with_vkey"]["best_ms"], 3)
    out["check_over_prove"] = round(out["check_lagrange_with_vkey"]["best_ms"] / out["prove_blocking_lagrange"]["best_ms"], 2)
    powers.close()
    g1w, g2w = lag.pool_points(1, compressed=True), lag.pool_points(2, compressed=True)
    loads = []
    for i in range(repeats + 1):          # the first is a warm-up
        holder = []
        t = timed(lambda: holder.append(Groth16.from_compressed(cs, g1w, g2w, lagrange=True)))
        if i:
            loads.append(t)
        holder[0].close()
    out["upload_compressed_lagrange"] = summary(loads)
    # one check alone under the per-family timers (they serialise the launches: not the wall time above)
    _lib.check(L.zk_profile_enable(2))
    _lib.check(L.zk_profile_reset())
    lag.check_lagrange_key(vk)
    _lib.check(L.zk_sync())
    out["device_ms_by_family_one_check"] = families()
    _lib.check(L.zk_profile_enable(0))
    lag.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_check_lagrange.json"))
    ap.add_argument("--log-n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    _lib.check(_lib.lib().zk_init(0))
    doc = {"how": "python scripts/bench_key_check_lagrange.py (host wall time, best of %d, the four calls alternating; one MI355X)" % a.repeats, "sizes": {}}
    for log_n in a.log_n:
        doc["sizes"]["2^%d" % log_n] = measure(log_n, a.repeats)
        print("2^%d:" % log_n, json.dumps({k: (v["best_ms"] if isinstance(v, dict) and "best_ms" in v else v) for k, v in doc["sizes"]["2^%d" % log_n].items()
                                            if not k.startswith("device_")}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
