#!/usr/bin/env python3
"""A batch of proofs from witnesses to wire bytes: host wall time for --proofs proofs on one key, on one MI355X.

  route A   prove_async / prove_wait over `in_flight` slots by hand, then Proof.to_compressed() per proof   (what a host had before)
  route B   zk_*_prove_many_compressed at the same in_flight                                                 (Groth16.prove_many / pinocchio.ZK.prove_many)

Every proof of one run has the same witness (handed over as a host buffer per proof on both routes) and its own randomness.  Best of --repeats with
the routes alternating in one process; every timing is kept (the spread of A decides what "faster" means).  Every proof of both routes is compared with
the trapdoor oracle's proof through the host compressor.  Also: the device time of the prove_to_wire family (zk_profile_get) in a run of its own.

    python scripts/bench_prove_many.py --out profiles/prove_many.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O                                  # noqa: E402
from zukelang_amd import _lib, r1cs as RC               # noqa: E402
from zukelang_amd import pinocchio as PIN               # noqa: E402
from zukelang_amd.curve import G1, G2                   # noqa: E402
from zukelang_amd.groth16 import Groth16                # noqa: E402


def frs(xs):
    return bytes(RC.fr_bytes(xs))


def family(name):
    ms, cnt = C.c_double(), C.c_uint64()
    _lib.check(_lib.lib().zk_profile_get(name.encode(), C.byref(ms), C.byref(cnt)))
    return {"ms": round(ms.value, 4), "launches": cnt.value}


def measure(label, log_n, prover, route_a, route_b, expected, proofs, in_flight, repeats):
    L = _lib.lib()
    times = {"A": [], "B": []}

    def one(route, fn):
        _lib.check(L.zk_sync())
        t0 = time.perf_counter()
        got = fn()
        t1 = time.perf_counter()
        if got != expected:
            raise SystemExit("%s 2^%d: route %s gave other bytes than the oracle" % (label, log_n, route))
        times[route].append(round(t1 - t0, 5))

    prover.reserve_slots(in_flight)
    one("A", route_a); one("B", route_b)          # warm-up
    for r in times.values():
        r.clear()
    for _ in range(repeats):
        one("A", route_a)
        one("B", route_b)
    _lib.check(L.zk_profile_reset())
    _lib.check(L.zk_profile_enable(2))
    route_b()
    fam = family("prove_to_wire")
    _lib.check(L.zk_profile_enable(0))
    _lib.check(L.zk_profile_reset())
    best = {k: min(v) for k, v in times.items()}
    spread = round(max(times["A"]) - min(times["A"]), 5)
    return {"protocol": label, "log_n": log_n, "proofs": proofs, "in_flight": in_flight, "timings_s": times, "best_s": best,
            "best_ms_per_proof": {k: round(1e3 * v / proofs, 4) for k, v in best.items()}, "route_A_spread_s": spread,
            "B_beats_A_by_s": round(best["A"] - best["B"], 5), "B_faster_beyond_A_spread": best["A"] - best["B"] > spread,
            "every_proof_equals_the_oracle": True, "prove_to_wire_device": fam}


def oracle_all(fn, jobs):
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:          # the oracle is C behind ctypes: the calls run side by side
        return list(ex.map(fn, jobs))


def groth16(log_n, proofs, in_flight, repeats):
    cs, w = RC.iterated_cubic(1 << log_n, next(RC.fr_stream(0x5EED0001)))
    st = RC.fr_stream(0x5EED0C16 + log_n)
    tox = [next(st) for _ in range(5)]
    it = iter(tox)
    prover, pk, _ = Groth16.generate(lambda: next(it), cs, form="lagrange")          # the handle of upload + derive_lagrange
    del pk
    rs = [(next(st), next(st)) for _ in range(proofs)]
    csr = [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
    wb = RC.fr_bytes(w)
    wbytes, toxb = bytes(wb), frs(tox)

    def oracle(job):
        a, b, c = O.groth16_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, wbytes, toxb, frs([job[0]]), frs([job[1]]))
        return G1.to_compressed_bytes(a) + G2.to_compressed_bytes(b) + G1.to_compressed_bytes(c)

    expected = oracle_all(oracle, rs)
    sols = np.tile(np.ascontiguousarray(wb, dtype=np.uint8).reshape(1, -1), (proofs, 1))          # the witnesses back to back, as the call takes them

    def route_a():
        out = [None] * proofs
        for i, (r, s) in enumerate(rs):
            if i >= in_flight:
                out[i - in_flight] = prover.prove_wait(i % in_flight).to_compressed()
            prover.prove_async(wb, r, s, i % in_flight)
        for i in range(max(0, proofs - in_flight), proofs):
            out[i] = prover.prove_wait(i % in_flight).to_compressed()
        return out

    res = measure("groth16", log_n, prover, route_a, lambda: prover.prove_many(rs, sols, in_flight=in_flight), expected, proofs, in_flight, repeats)
    prover.close()
    return res


def pinocchio(log_n, proofs, in_flight, repeats):
    cs, w = RC.iterated_cubic(1 << log_n, next(RC.fr_stream(0x5EED0001)))
    st = RC.fr_stream(0x5EED0C17 + log_n)
    tox = [next(st) for _ in range(8)]
    it = iter(tox)
    prover, pk, _ = PIN.ZK.generate(lambda: next(it), cs, form="lagrange")
    del pk
    ds = [(next(st), next(st), next(st)) for _ in range(proofs)]
    csr = [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
    wb = RC.fr_bytes(w)
    wbytes, toxb = bytes(wb), frs(tox)

    def oracle(d):
        p = O.pinocchio_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, wbytes, toxb, *(frs([x]) for x in d))
        return PIN.Proof(p[:96], p[96:288], p[288:384], p[384:480], p[480:576], p[576:768], p[768:864], p[864:960]).to_compressed()

    expected = oracle_all(oracle, ds)
    prover.set_witness(wb)          # the Python prove_async of this protocol takes the resident witness

    def route_a():
        out = [None] * proofs
        for i, d in enumerate(ds):
            if i >= in_flight:
                out[i - in_flight] = prover.prove_wait(i % in_flight).to_compressed()
            prover.prove_async(*d, i % in_flight)
        for i in range(max(0, proofs - in_flight), proofs):
            out[i] = prover.prove_wait(i % in_flight).to_compressed()
        return out

    res = measure("pinocchio", log_n, prover, route_a, lambda: prover.prove_many(ds, proofs, in_flight=in_flight), expected, proofs, in_flight, repeats)
    res["witness"] = "resident on the device on both routes"
    prover.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groth16", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--pinocchio", type=int, nargs="*", default=[18])
    ap.add_argument("--proofs", type=int, default=64)
    ap.add_argument("--in-flight", type=int, default=14)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.check(_lib.lib().zk_init(0))
    res = {"what": "host wall time from witnesses in host memory to the proofs' wire bytes, all proofs of a run on one key",
           "routes": {"A": "prove_async / prove_wait over in_flight slots, then Proof.to_compressed() per proof", "B": "zk_*_prove_many_compressed at the same in_flight"},
           "repeats": args.repeats, "device": "1 x MI355X", "runs": []}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    for ln in args.groth16:
        res["runs"].append(groth16(ln, args.proofs, args.in_flight, args.repeats))
        print(json.dumps(res["runs"][-1]), flush=True)
        save()
    for ln in args.pinocchio:
        res["runs"].append(pinocchio(ln, args.proofs, args.in_flight, args.repeats))
        print(json.dumps(res["runs"][-1]), flush=True)
        save()


if __name__ == "__main__":
    main()
