#!/usr/bin/env python3
"""What zk_groth16_srs_check and zk_groth16_srs_contribute cost.  One MI355X (the script needs one: without a GPU every call below fails with ZK_ERR_HIP).

  sizes   the honest string of a circuit of 2^16 and 2^18 constraints (SRS.sizes: 2n-1 / n / n+2 points), already in host memory as the C calls take
          it: host wall time of each call, best of --repeats with every run recorded, and ONE call each under zk_profile_enable(2) for the device
          time by stage -- srs_check:decode, :subgroup, :sums, :pairings; srs_contribute:decode, :subgroup, :scalars, :multiply.  Beside them, for
          scale and not as gates, on the same string: Groth16.specialize (tau powers) of iterated cubic and check_key of the result -- what a host
          paid before to learn anything about a string.
  --single-log-n 20   one single run of both calls at that size
  --ab    the check's sums over window tables built for the call (make -C zukelang_amd/csrc srs-tabled) against the shipped form without tables, whole
          call at 2^18, each candidate in a process of its own (--ab-child).  The tabled form would ship only if it won by more than the spread of the
          un-tabled form's runs.  Written to --ab-out.
Every timed check must return mask 0; every timed contribution is compared with SRS.generate of the product trapdoor before it counts.

    python scripts/bench_srs.py --out profiles/srs.json
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
from zukelang_amd.groth16 import SRS, Groth16, _p           # noqa: E402
from zukelang_amd.r1cs import FR_MODULUS as R               # noqa: E402

TRAPDOOR = (0xA11FA + (3 << 190), 0xBE7A + (5 << 200), 0x7A0 + (7 << 210))          # alpha, beta, tau
MUL = (0xA1FA0001 + (1 << 200), 0xBE7A0002 + (1 << 210), 0x7A0003 + (1 << 220))      # alpha', beta', tau'
SEED = np.frombuffer(bytes(range(32)), dtype=np.uint8)
KEEP = ("srs_check", "srs_contribute", "subgroup_check", "msm_precompute", "msm_sort", "msm_accumulate_g1", "msm_accumulate_g2", "msm_reduce_g1", "msm_reduce_g2",
        "pairing_miller", "pairing_final_exp")


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
        if cnt.value and f.split(":")[0] in KEEP:
            out[f] = {"ms": round(ms.value, 3), "launches": cnt.value}
    return out


def profiled(fn):
    L = _lib.lib()
    _lib.check(L.zk_profile_enable(2))
    _lib.check(L.zk_profile_reset())
    out = fn()
    _lib.check(L.zk_sync())
    fam = families()
    _lib.check(L.zk_profile_enable(0))
    return fam, out


def string(n, trapdoor=TRAPDOOR):
    it = iter(trapdoor)
    return SRS.generate(lambda: next(it), n)


class Flat:
    """a string as the C calls take it"""

    def __init__(self, srs):
        self.s1, self.n1, self.nab, self.s2, self.n2 = srs._lists("bench")

    def check(self):
        failed = C.c_uint32(0xFFFFFFFF)
        _lib.check(_lib.lib().zk_groth16_srs_check(_p(self.s1), self.n1, self.nab, _p(self.s2), self.n2, _p(SEED), C.byref(failed)))
        if failed.value:
            raise SystemExit("the honest string fails the check: mask %d" % failed.value)

    def contribute(self):
        k = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in MUL), dtype=np.uint8)
        o1, o2 = np.empty_like(self.s1), np.empty_like(self.s2)
        _lib.check(_lib.lib().zk_groth16_srs_contribute(_p(self.s1), self.n1, self.nab, _p(self.s2), self.n2, _p(k), _p(o1), _p(o2), None, None))
        return o1, o2


def measure(log_n, repeats, scale=True):
    n = 1 << log_n
    srs = string(n)
    f = Flat(srs)
    want = Flat(string(n, tuple(x * y % R for x, y in zip(TRAPDOOR, MUL))))
    out = {"constraints_the_string_serves": n, "points": {"tau1": f.n1, "alpha_tau1": f.nab, "beta_tau1": f.nab, "tau2": f.n2}}

    def contributed():
        o1, o2 = f.contribute()
        if not (np.array_equal(o1, want.s1) and np.array_equal(o2, want.s2)):
            raise SystemExit("2^%d: the contributed string is not the string of the product trapdoor" % log_n)
    f.check()          # warm-up: module load, first allocations
    contributed()
    chk, con = [], []
    for _ in range(repeats):
        chk.append(timed(f.check)[0])
    for _ in range(repeats):
        ms, (o1, o2) = timed(f.contribute)
        con.append(ms)
    out["srs_check_whole_call"] = stats(chk)
    out["srs_contribute_whole_call"] = stats(con)
    out["srs_check_device_ms_by_family_one_call"] = profiled(f.check)[0]
    out["srs_contribute_device_ms_by_family_one_call"] = profiled(f.contribute)[0]
    if scale:
        cs = RC.iterated_cubic(n, 0xC0FFEE)[0]
        ms, (pr, _, vk) = timed(lambda: Groth16.specialize(cs, srs, form="tau_powers"))
        out["for_scale_specialize_tau_powers_ms"] = round(ms, 3)
        ms, verdict = timed(lambda: pr.check_key(vk, seed=bytes(SEED)))
        out["for_scale_check_key_ms"] = round(ms, 3)
        if not verdict.ok:
            raise SystemExit("the specialised key fails check_key")
        pr.close()
    return out


def ab_child(log_n, repeats):
    """prints one JSON line: whole-call ms of the check per run, for the library this process loaded"""
    _lib.check(_lib.lib().zk_init(0))
    f = Flat(string(1 << log_n))
    f.check()
    runs = [timed(f.check)[0] for _ in range(repeats)]
    fam = profiled(f.check)[0]
    print("AB-RESULT " + json.dumps({"runs": runs, "device_ms_by_family_one_call": fam}), flush=True)


def ab(log_n, repeats):
    variant = os.path.join(ROOT, "zukelang_amd", "libzkmi355x_srstabled.so")
    if not os.path.exists(variant):
        raise SystemExit("build the variant first: make -C zukelang_amd/csrc srs-tabled")
    row = {"size": "the string of 2^%d constraints, whole zk_groth16_srs_check call, host wall time" % log_n}
    for name, lib in (("untabled", None), ("tabled", variant)):
        env = dict(os.environ)
        if lib:
            env["ZK_LIBZKMI355X_PATH"] = lib
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--ab-log-n", str(log_n), "--repeats", str(repeats)], capture_output=True, text=True,
                             env=env, timeout=900)
        line = [x for x in res.stdout.splitlines() if x.startswith("AB-RESULT ")]
        if res.returncode or not line:
            raise SystemExit("A/B child %s failed: %s" % (name, res.stdout[-1000:] + res.stderr[-3000:]))
        got = json.loads(line[0][len("AB-RESULT "):])
        row[name] = dict(stats(got["runs"]), device_ms_by_family_one_call=got["device_ms_by_family_one_call"])
    win = row["untabled"]["best_ms"] - row["tabled"]["best_ms"]
    row["tabled_wins_by_ms"] = round(win, 3)
    row["rule"] = "the tabled form ships only if it wins the whole call by more than the spread of the un-tabled form's runs"
    row["tabled_ships"] = bool(win > row["untabled"]["spread_ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srs.json"))
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "srs_ab.json"))
    ap.add_argument("--log-n", type=int, nargs="*", default=[16, 18])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--single-log-n", type=int, default=0)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--ab-child", action="store_true")
    ap.add_argument("--ab-log-n", type=int, default=18)
    a = ap.parse_args()
    if a.ab_child:
        return ab_child(a.ab_log_n, a.repeats)
    if a.ab:
        doc = {"how": "python scripts/bench_srs.py --ab (best of %d, each candidate in a process of its own; one MI355X)" % a.repeats, "2^%d" % a.ab_log_n: ab(a.ab_log_n, a.repeats)}
        print(json.dumps(doc), flush=True)
        with open(a.ab_out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    _lib.check(_lib.lib().zk_init(0))          # ZK_ERR_HIP without a GPU: this script measures a device
    doc = {"how": "python scripts/bench_srs.py (host wall time, best of %d; one MI355X)" % a.repeats, "sizes": {}}
    if os.path.exists(a.out):
        doc = json.load(open(a.out))          # the parts are measured in calls of their own and kept side by side

    def save():
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if a.single_log_n:
        doc["single_run 2^%d" % a.single_log_n] = measure(a.single_log_n, 1)
        print(json.dumps(doc["single_run 2^%d" % a.single_log_n]), flush=True)
        return save()
    for log_n in a.log_n:
        doc["sizes"]["2^%d" % log_n] = measure(log_n, a.repeats)
        print("2^%d" % log_n, json.dumps(doc["sizes"]["2^%d" % log_n]), flush=True)
        save()          # after every size: a run cut short keeps what it has measured


if __name__ == "__main__":
    main()
