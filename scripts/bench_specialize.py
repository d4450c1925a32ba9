#!/usr/bin/env python3
"""What zk_groth16_pk_specialize costs.  One MI355X (the script needs one: without a GPU every call below fails with ZK_ERR_HIP).

  sizes   iterated cubic at 2^16 and 2^18 constraints, both handle forms: host wall time of Groth16.specialize (string already in host memory), best
          of --repeats with every run recorded, and ONE call under zk_profile_enable(2) for the device time by stage -- specialize_derive (the three
          derivations, side by side), specialize_correlate (tiztd), specialize_mul (the general entries), specialize_sum (the summing launches),
          lagrange_derive (the [l_i]_2 and h bases of a Lagrange-form handle) and the table builds.  Beside them, for scale and not as gates, on the
          same circuit: Groth16.generate (zk_groth16_keygen, which needs the trapdoor) and derive_lagrange of an uploaded key.
  --single-log-n 20   one single run of the tau-power form at that size (its own process and time limit are the caller's business)
  --split   the column sums alone, device time of specialize_mul + specialize_sum of a whole call, on the random R1CS at 2^16 (8 entries per row,
            coefficients small, negative and full-width) and on iterated cubic at 2^16: this library against the variant that multiplies every entry
            (make -C zukelang_amd/csrc specialize-nosplit; each candidate in a process of its own, --split-child).  The split stays only if it wins by
            more than the spread of the other's runs.
Every timed result is compared with the pools of a zk_groth16_keygen handle of the same trapdoor and form before it counts.

    python scripts/bench_specialize.py --out profiles/specialize.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                          # noqa: E402

from zukelang_amd import _lib, r1cs as RC                   # noqa: E402
from zukelang_amd.groth16 import SRS, Groth16               # noqa: E402
from zukelang_amd.r1cs import FR_MODULUS                    # noqa: E402

TRAPDOOR = (0xA11FA + (3 << 190), 0xBE7A + (5 << 200), 0x7A0 + (7 << 210))          # alpha, beta, tau
STAGES = ("specialize_derive", "specialize_correlate", "specialize_mul", "specialize_sum", "lagrange_derive")


def timed(fn):
    _lib.check(_lib.lib().zk_sync())
    t0 = time.perf_counter()
    out = fn()
    _lib.check(_lib.lib().zk_sync())
    return 1e3 * (time.perf_counter() - t0), out


def stats(ts):
    return {"best_ms": round(min(ts), 3), "spread_ms": round(max(ts) - min(ts), 3), "all_ms": [round(t, 3) for t in ts]}


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


def circuit(kind, log_n):
    n = 1 << log_n
    if kind == "cubic":
        return RC.iterated_cubic(n, 0xC0FFEE)[0]
    return RC.random_r1cs(n, n, 0x5EC0000 + log_n, nnz=(8, 8))[0]


def string_and_pools(cs, form):
    """the honest string of TRAPDOOR for this circuit, and the pools of the keygen handle of (alpha, beta, 1, 1, tau) in `form`"""
    it = iter(TRAPDOOR)
    srs = SRS.generate(lambda: next(it), cs.n)
    a, b, t = TRAPDOOR
    it = iter([a, b, 1, 1, t])
    ms, (gen, _, _) = timed(lambda: Groth16.generate(lambda: next(it), cs, form=form))
    pools = (gen.pool_points(1).copy(), gen.pool_points(2).copy())
    gen.close()
    return srs, pools, ms


def checked(pr, pools, what):
    if not (np.array_equal(pr.pool_points(1), pools[0]) and np.array_equal(pr.pool_points(2), pools[1])):
        raise SystemExit("%s: the pools differ from the keygen handle's" % what)


def entry_classes(cs):
    unit = general = zero = 0
    for M in (cs.L, cs.R, cs.O):
        v = M.val.reshape(-1, 32)
        one = np.zeros(32, dtype=np.uint8); one[0] = 1
        neg = np.frombuffer(int(FR_MODULUS - 1).to_bytes(32, "little"), dtype=np.uint8)
        u = int(np.count_nonzero((v == one).all(axis=1) | (v == neg).all(axis=1)))
        z = int(np.count_nonzero((v == 0).all(axis=1)))
        unit, zero, general = unit + u, zero + z, general + len(v) - u - z
    return {"unit": unit, "general": general, "zero": zero}


def measure(log_n, form, repeats):
    cs = circuit("cubic", log_n)
    srs, pools, keygen_ms = string_and_pools(cs, form)
    what = "2^%d %s" % (log_n, form)
    pr = Groth16.specialize(cs, srs, form=form)[0]          # warm-up: module load, first allocations
    checked(pr, pools, what)
    pr.close()
    whole = []
    for _ in range(repeats):
        ms, (pr, _, _) = timed(lambda: Groth16.specialize(cs, srs, form=form))
        checked(pr, pools, what)
        pr.close()
        whole.append(ms)
    out = {"constraints": cs.n, "variables": cs.m, "form": form, "entries": entry_classes(cs), "specialize_whole_call": stats(whole)}
    L = _lib.lib()
    _lib.check(L.zk_profile_enable(2))
    _lib.check(L.zk_profile_reset())
    pr = Groth16.specialize(cs, srs, form=form)[0]
    _lib.check(L.zk_sync())
    out["device_ms_by_family_one_call"] = families()
    _lib.check(L.zk_profile_enable(0))
    checked(pr, pools, what)
    pr.close()
    out["for_scale_keygen_same_form_ms"] = round(keygen_ms, 3)
    if form == "tau_powers":          # the derivation of an uploaded key, once: what a host pays today to get from tau powers to the Lagrange form
        a, b, t = TRAPDOOR
        it = iter([a, b, 1, 1, t])
        gen = Groth16.generate(lambda: next(it), cs, form="tau_powers")[0]
        out["for_scale_derive_lagrange_ms"] = round(timed(gen.derive_lagrange)[0], 3)
        gen.close()
    return out


def single(log_n):
    cs = circuit("cubic", log_n)
    srs, pools, keygen_ms = string_and_pools(cs, "tau_powers")
    L = _lib.lib()
    _lib.check(L.zk_profile_enable(2))
    _lib.check(L.zk_profile_reset())
    ms, (pr, _, _) = timed(lambda: Groth16.specialize(cs, srs, form="tau_powers"))
    fam = families()
    _lib.check(L.zk_profile_enable(0))
    checked(pr, pools, "2^%d single run" % log_n)
    pr.close()
    return {"constraints": cs.n, "form": "tau_powers", "specialize_single_run_ms": round(ms, 3), "first_call_of_its_process": True,
            "device_ms_by_family": fam, "for_scale_keygen_same_form_ms": round(keygen_ms, 3)}


def split_child(kind, log_n, repeats):
    """prints one JSON line: device ms of specialize_mul + specialize_sum per run, for the library this process loaded"""
    _lib.check(_lib.lib().zk_init(0))
    cs = circuit(kind, log_n)
    srs, pools, _ = string_and_pools(cs, "tau_powers")
    L = _lib.lib()
    runs = []
    for i in range(repeats + 1):
        _lib.check(L.zk_profile_enable(2))
        _lib.check(L.zk_profile_reset())
        pr = Groth16.specialize(cs, srs, form="tau_powers")[0]
        _lib.check(L.zk_sync())
        fam = families()
        _lib.check(L.zk_profile_enable(0))
        checked(pr, pools, "split %s" % kind)
        pr.close()
        if i:          # the first run warms up
            runs.append({k: fam.get(k, {"ms": 0.0})["ms"] for k in ("specialize_mul", "specialize_sum")})
    print("SPLIT-RESULT " + json.dumps({"entries": entry_classes(cs), "runs": runs}), flush=True)


def split(repeats):
    out = {}
    variant = os.path.join(ROOT, "zukelang_amd", "libzkmi355x_nosplit.so")
    if not os.path.exists(variant):
        raise SystemExit("build the variant first: make -C zukelang_amd/csrc specialize-nosplit")
    for kind in ("random", "cubic"):
        row = {}
        for name, lib in (("split", None), ("multiply_every_entry", variant)):
            env = dict(os.environ)
            if lib:
                env["ZK_LIBZKMI355X_PATH"] = lib
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--split-child", kind, "--repeats", str(repeats)], capture_output=True, text=True, env=env,
                                 timeout=900)
            line = [x for x in res.stdout.splitlines() if x.startswith("SPLIT-RESULT ")]
            if res.returncode or not line:
                raise SystemExit("split child %s / %s failed: %s" % (kind, name, res.stdout[-1000:] + res.stderr[-3000:]))
            got = json.loads(line[0][len("SPLIT-RESULT "):])
            total = [r["specialize_mul"] + r["specialize_sum"] for r in got["runs"]]
            row["entries"] = got["entries"]
            row[name] = dict(stats(total), mul_ms=[r["specialize_mul"] for r in got["runs"]], sum_ms=[r["specialize_sum"] for r in got["runs"]])
        win = row["multiply_every_entry"]["best_ms"] - row["split"]["best_ms"]
        row["split_wins_by_ms"] = round(win, 3)
        row["split_stays"] = bool(win > row["multiply_every_entry"]["spread_ms"])
        out["%s 2^16" % kind] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specialize.json"))
    ap.add_argument("--log-n", type=int, nargs="*", default=[16, 18])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--single-log-n", type=int, default=0)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--split-child", default="")
    a = ap.parse_args()
    if a.split_child:
        return split_child(a.split_child, 16, a.repeats)
    _lib.check(_lib.lib().zk_init(0))          # ZK_ERR_HIP without a GPU: this script measures a device
    doc = {"how": "python scripts/bench_specialize.py (host wall time, best of %d; one MI355X)" % a.repeats, "sizes": {}}
    if os.path.exists(a.out):
        doc = json.load(open(a.out))          # the parts are measured in calls of their own and kept side by side

    def save():
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if a.single_log_n:
        doc["single_run 2^%d" % a.single_log_n] = single(a.single_log_n)
        print(json.dumps(doc["single_run 2^%d" % a.single_log_n]), flush=True)
        return save()
    if a.split:
        doc["unit_general_split"] = split(a.repeats)
        print(json.dumps(doc["unit_general_split"]), flush=True)
        return save()
    for log_n in a.log_n:
        for form in ("tau_powers", "lagrange"):
            key = "2^%d %s" % (log_n, form)
            doc["sizes"][key] = measure(log_n, form, a.repeats)
            print(key, json.dumps({k: (v["best_ms"] if isinstance(v, dict) and "best_ms" in v else v) for k, v in doc["sizes"][key].items()}), flush=True)
            save()          # after every size: a run cut short keeps what it has measured


if __name__ == "__main__":
    main()
