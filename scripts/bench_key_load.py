#!/usr/bin/env python3
"""Loading a proving key from its compressed wire bytes: host wall time from the bytes in host memory to a handle that has produced one proof equal
to the trapdoor oracle's, on one MI355X.

  route A   zk_g1/g2_decompress_batch on both lists, then zk_*_pk_upload        (what wire.*_pkey_of_json -> Groth16(...) / pinocchio.ZK(...) does)
  route B   zk_*_pk_upload_compressed                                           (Groth16.from_compressed / pinocchio.ZK.from_compressed)
  route B0  route B under ZK_KEY_SUBGROUP_CHECK=0

Best of --repeats with the routes alternating in one process; every timing of every route is kept (the spread of A decides what "faster" means).
Also: the per-family device times of route B (zk_profile_get: key_decompress, subgroup_check, msm_precompute) in a run of their own, and
pool_points(compressed=True) against pool_points() + host compression.

    python scripts/bench_key_load.py --out profiles/key_load_compressed.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O                                  # noqa: E402
from zukelang_amd import _lib, r1cs as RC               # noqa: E402
from zukelang_amd import pinocchio as PIN               # noqa: E402
from zukelang_amd.curve import G1, G2                   # noqa: E402
from zukelang_amd.groth16 import Groth16, PKey          # noqa: E402

FAMILIES = ("key_decompress", "subgroup_check", "msm_precompute")


def frs(xs):
    return bytes(RC.fr_bytes(xs))


def set_option(name, value):
    _lib.check(_lib.lib().zk_set_option(name.encode(), None if value is None else str(value).encode()))


def families():
    out = {}
    for f in FAMILIES:
        ms, cnt = C.c_double(), C.c_uint64()
        _lib.check(_lib.lib().zk_profile_get(f.encode(), C.byref(ms), C.byref(cnt)))
        out[f] = {"ms": round(ms.value, 3), "launches": cnt.value}
    return out


def measure(label, log_n, make_a, make_b, prove, expected, pools, repeats):
    """make_a / make_b: () -> prover; prove: prover -> proof bytes"""
    L = _lib.lib()
    times = {"A": [], "B": [], "B_no_subgroup_check": []}

    def one(route, make):
        _lib.check(L.zk_sync())
        t0 = time.perf_counter()
        p = make()
        t1 = time.perf_counter()
        got = prove(p)
        t2 = time.perf_counter()
        if got != expected:
            raise SystemExit("%s: route %s proved other bytes than the oracle" % (label, route))
        p.close()
        times[route].append({"to_handle_s": round(t1 - t0, 4), "to_first_proof_s": round(t2 - t0, 4)})

    one("A", make_a); one("B", make_b)          # warm-up: module load, first allocations
    for r in times.values():
        r.clear()
    for _ in range(repeats):
        one("A", make_a)
        one("B", make_b)
        set_option("ZK_KEY_SUBGROUP_CHECK", 0)
        try:
            one("B_no_subgroup_check", make_b)
        finally:
            set_option("ZK_KEY_SUBGROUP_CHECK", None)
    # device time per kernel family of route B, in a run of its own (event timers on)
    _lib.check(L.zk_profile_reset())
    _lib.check(L.zk_profile_enable(2))
    p = make_b()
    fam = families()
    _lib.check(L.zk_profile_enable(0))
    _lib.check(L.zk_profile_reset())
    # the way out: the pools in wire form from the device against uncompressed read-back + host compression
    back = {"device_compressed_s": [], "uncompressed_plus_host_compression_s": []}
    for _ in range(repeats):
        t0 = time.perf_counter()
        dev = [bytes(p.pool_points(i, compressed=True)) for i in pools]
        t1 = time.perf_counter()
        host = [(G1 if g == 1 else G2).to_compressed_bytes_many(bytes(p.pool_points(i))) for i, g in pools.items()]
        t2 = time.perf_counter()
        if dev != host:
            raise SystemExit("%s: pool_points(compressed=True) differs from the host compression" % label)
        back["device_compressed_s"].append(round(t1 - t0, 4))
        back["uncompressed_plus_host_compression_s"].append(round(t2 - t1, 4))
    p.close()
    best = {k: min(x["to_first_proof_s"] for x in v) for k, v in times.items()}
    a = [x["to_first_proof_s"] for x in times["A"]]
    return {"protocol": label, "log_n": log_n, "timings": times, "best_to_first_proof_s": best, "route_A_spread_s": round(max(a) - min(a), 4),
            "B_beats_A_by_s": round(best["A"] - best["B"], 4), "B_faster_beyond_A_spread": best["A"] - best["B"] > max(a) - min(a),
            "route_B_device_ms_by_family": fam, "pool_read_back": back}


def groth16(log_n, repeats):
    n = 1 << log_n
    cs, w = RC.iterated_cubic(n, next(RC.fr_stream(0x5EED0001)))
    st = RC.fr_stream(0x5EED0B16 + log_n)
    tox = [next(st) for _ in range(5)]
    it = iter(tox)
    prover, pk, _ = Groth16.generate(lambda: next(it), cs, form="tau_powers")
    prover.close()
    r, s = next(st), next(st)
    csr = [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
    exp = O.groth16_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), frs(tox), frs([r]), frs([s]))
    g1w, g2w = G1.to_compressed_bytes_many(pk.g1), G2.to_compressed_bytes_many(pk.g2)
    points = {"g1": len(g1w) // 48, "g2": len(g2w) // 96}
    del pk
    wb = RC.fr_bytes(w)

    def make_a():
        g1 = np.frombuffer(G1.of_compressed_bytes_many(g1w), dtype=np.uint8)
        g2 = np.frombuffer(G2.of_compressed_bytes_many(g2w), dtype=np.uint8)
        return Groth16(cs, PKey(g1, g2))

    def prove(p):
        pr = p.prove_rs(wb, r, s)
        return (pr.a, pr.b, pr.c)

    out = measure("groth16", log_n, make_a, lambda: Groth16.from_compressed(cs, g1w, g2w), prove, exp, {1: 1, 2: 2}, repeats)
    out["points"] = points
    return out


def pinocchio(log_n, repeats):
    n = 1 << log_n
    cs, w = RC.iterated_cubic(n, next(RC.fr_stream(0x5EED0001)))
    st = RC.fr_stream(0x5EED0B17 + log_n)
    tox = [next(st) for _ in range(8)]
    it = iter(tox)
    prover, pk, _ = PIN.ZK.generate(lambda: next(it), cs, form="tau_powers")
    prover.close()
    d = [next(st) for _ in range(3)]
    csr = [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
    exp = O.pinocchio_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), frs(tox), *(frs([x]) for x in d))
    g1w, g2w = G1.to_compressed_bytes_many(pk.g1), G2.to_compressed_bytes_many(pk.g2)
    points = {"g1": len(g1w) // 48, "g2": len(g2w) // 96}
    del pk
    wb = RC.fr_bytes(w)

    def make_a():
        g1 = np.frombuffer(G1.of_compressed_bytes_many(g1w), dtype=np.uint8)
        g2 = np.frombuffer(G2.of_compressed_bytes_many(g2w), dtype=np.uint8)
        return PIN.ZK(cs, PIN.PKey(g1, g2))

    out = measure("pinocchio", log_n, make_a, lambda: PIN.ZK.from_compressed(cs, g1w, g2w), lambda p: p.prove_with(wb, *d).to_bytes(), exp,
                  {i: (1 if i < 6 else 2) for i in range(8)}, repeats)
    out["points"] = points
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groth16", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--pinocchio", type=int, nargs="*", default=[18])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.check(_lib.lib().zk_init(0))
    res = {"what": "host wall time from a key's compressed wire bytes in host memory to a handle that has produced one proof equal to the trapdoor oracle's",
           "routes": {"A": "zk_g1/g2_decompress_batch x2, then zk_*_pk_upload", "B": "zk_*_pk_upload_compressed",
                      "B_no_subgroup_check": "route B under ZK_KEY_SUBGROUP_CHECK=0"},
           "repeats": args.repeats, "device": "1 x MI355X", "runs": []}
    for ln in args.groth16:
        res["runs"].append(groth16(ln, args.repeats))
        print(json.dumps(res["runs"][-1]), flush=True)
    for ln in args.pinocchio:
        res["runs"].append(pinocchio(ln, args.repeats))
        print(json.dumps(res["runs"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
