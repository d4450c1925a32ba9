#!/usr/bin/env python3
"""Verification in batches on one MI355X against the single-proof host verifiers, in ONE process: host wall time of a whole call, both PCIe
copies included.

  zk_groth16_verify_many      counts 1, 16, 256, 4096   on the README circuit's key (2 public values) and on a key with 64 public values
  zk_pinocchio_verify_many    counts 16, 256, 1024      on iterated_cubic(6, x) (2 public values)
  zk_pairing_product_many     4096 single pairs

next to the same number of zk_groth16_verify / zk_pinocchio_verify / zk_pairing_product calls -- where that would take minutes, 256 host calls are
timed and the time per call is scaled.  Each device figure is the best of three calls after one warm-up call (the first call of a process also
loads the kernels); every verdict is checked to be true outside the timed region, and a batch with one broken proof must say so.  The record also
holds the smallest count of a doubling sweep at which the device call wins, and the kernel families' times from a pass of its own at count 256.
Keys and proofs come from the GPU prover; a batch repeats 16 distinct proofs (what a verification costs does not depend on the proof).
Usage: python scripts/bench_verify_many.py [--out profiles/verify_many.json] [--quick]"""
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
from zukelang_amd.curve import G1, G2  # noqa: E402
from zukelang_amd.groth16 import Groth16  # noqa: E402

FAMILIES = ["pairing_point_checks", "pairing_miller", "pairing_final_exp", "msm_short"]
HOST_CALLS_MAX = 256
u8 = lambda b: C.cast(C.c_char_p(bytes(b)), _lib._P8) if len(b) else None


def best_of(fn, reps=3):
    fn()                                    # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return min(ts), ts


def host_time(one_call, count):
    """seconds for `count` host calls: all of them up to HOST_CALLS_MAX, else HOST_CALLS_MAX timed and scaled"""
    n = min(count, HOST_CALLS_MAX)
    t = time.perf_counter()
    for i in range(n):
        one_call(i)
    dt = time.perf_counter() - t
    return dt * count / n, dt / n, n


def profile_pass(run):
    L = _lib.lib()
    _lib.check(L.zk_profile_enable(2))
    _lib.check(L.zk_profile_reset())
    run()
    out = {}
    for fam in FAMILIES:
        ms, cnt = C.c_double(), C.c_uint64()
        _lib.check(L.zk_profile_get(fam.encode(), C.byref(ms), C.byref(cnt)))
        out[fam] = {"ms": round(ms.value, 3), "launches": cnt.value}
    _lib.check(L.zk_profile_enable(0))
    return out


def sweep(device_call, host_per_call, limit=1024):
    """the smallest count of 1, 2, 4, ... at which one device call is quicker than that many host calls; the whole sweep is recorded"""
    rows, first = [], None
    c = 1
    while c <= limit:
        dt, _ = best_of(lambda: device_call(c), 2)
        rows.append({"count": c, "device_ms": round(dt * 1e3, 3), "host_ms": round(host_per_call * c * 1e3, 3)})
        if first is None and dt < host_per_call * c:
            first = c
        c *= 2
    return first, rows


def groth16_case(name, cs, wits, rng, st, counts):
    lib = _lib.lib()
    prover, _, vk = Groth16.generate(rng, cs)
    proofs = [prover.prove_rs(w, next(st), next(st)) for w in wits]
    prover.close()
    lt = bytes(np.ascontiguousarray(vk.ltgm_io, dtype=np.uint8))
    n_io = len(lt) // 96
    pr = [bytes(p.a) + bytes(p.b) + bytes(p.c) for p in proofs]
    io = [bytes(RC.fr_bytes([w[k] for k in range(cs.m) if not cs.mid[k]])) for w in wits]

    def host_one(i):
        ok = C.c_int(0)
        _lib.check(lib.zk_groth16_verify(vk.ab, u8(lt), u8(io[i % len(pr)]), C.c_size_t(n_io), vk.gm, vk.d, pr[i % len(pr)], C.byref(ok)))
        assert ok.value == 1

    def device(count, broken=None):
        ios = b"".join(io[i % len(pr)] for i in range(count))
        prs = [pr[i % len(pr)] for i in range(count)]
        if broken is not None:
            prs[broken] = prs[broken][:288] + prs[broken][:96]          # A in the place of C: a valid point, a wrong proof
        ok = (C.c_uint8 * count)()
        st_ = (C.c_int32 * count)()
        pall = b"".join(prs)
        args = (u8(vk.ab), u8(lt), n_io, u8(vk.gm), u8(vk.d), u8(ios), u8(pall), count, C.cast(ok, _lib._P8), st_)
        return (lambda: _lib.check(lib.zk_groth16_verify_many(*args))), ok, st_

    rows = []
    for count in counts:
        call, ok, st_ = device(count)
        dt, all_ts = best_of(call)
        assert list(ok) == [1] * count and list(st_) == [0] * count
        if count > 1:
            callb, okb, _ = device(count, broken=count // 2)
            callb()
            assert list(okb) == [1] * (count // 2) + [0] + [1] * (count - count // 2 - 1)
        ht, hper, hn = host_time(host_one, count)
        rows.append({"count": count, "device_ms": round(dt * 1e3, 3), "device_ms_all": [round(x * 1e3, 3) for x in all_ts], "host_ms": round(ht * 1e3, 1),
                     "host_ms_per_call": round(hper * 1e3, 3), "host_calls_timed": hn, "host_over_device": round(ht / dt, 1)})
        print(name, rows[-1], flush=True)
    hper = rows[-1]["host_ms_per_call"] / 1e3
    first, sw = sweep(lambda c: device(c)[0](), hper)
    prof = profile_pass(device(256)[0])
    return {"key": name, "n_io": n_io, "rows": rows, "smallest_count_device_wins": first, "sweep": sw, "kernel_families_at_256": prof}


def pinocchio_case(cs, wits, rng, counts):
    lib = _lib.lib()
    prover, _, vk = PIN.ZK.generate(rng, cs)
    proofs = [prover.prove(rng, w).to_bytes() for w in wits]
    prover.close()
    g1, g2 = bytes(np.ascontiguousarray(vk.g1, dtype=np.uint8)), bytes(np.ascontiguousarray(vk.g2, dtype=np.uint8))
    io = [bytes(RC.fr_bytes([w[k] for k in range(cs.m) if not cs.mid[k]])) for w in wits]
    n_io = len(io[0]) // 32

    def host_one(i):
        ok = C.c_int(0)
        _lib.check(lib.zk_pinocchio_verify(g1, g2, u8(io[i % len(io)]), C.c_size_t(n_io), proofs[i % len(io)], C.byref(ok)))
        assert ok.value == 1

    def device(count):
        ios = b"".join(io[i % len(io)] for i in range(count))
        pall = b"".join(proofs[i % len(io)] for i in range(count))
        ok = (C.c_uint8 * count)()
        args = (u8(g1), u8(g2), n_io, u8(ios), u8(pall), count, C.cast(ok, _lib._P8), None)
        return (lambda: _lib.check(lib.zk_pinocchio_verify_many(*args))), ok

    rows = []
    for count in counts:
        call, ok = device(count)
        dt, all_ts = best_of(call)
        assert list(ok) == [1] * count
        ht, hper, hn = host_time(host_one, count)
        rows.append({"count": count, "device_ms": round(dt * 1e3, 3), "device_ms_all": [round(x * 1e3, 3) for x in all_ts], "host_ms": round(ht * 1e3, 1),
                     "host_ms_per_call": round(hper * 1e3, 3), "host_calls_timed": hn, "host_over_device": round(ht / dt, 1)})
        print("pinocchio", rows[-1], flush=True)
    first, sw = sweep(lambda c: device(c)[0](), rows[-1]["host_ms_per_call"] / 1e3, 256)
    prof = profile_pass(device(256)[0])
    return {"key": "iterated_cubic(6)", "n_io": n_io, "rows": rows, "smallest_count_device_wins": first, "sweep": sw, "kernel_families_at_256": prof}


def pairing_case(count, st):
    lib = _lib.lib()
    frs = lambda xs: bytes(RC.fr_bytes(xs))
    base = 64
    p1 = bytes(G1.of_Fr(frs([next(st) for _ in range(base)])))
    p2 = bytes(G2.of_Fr(frs([next(st) for _ in range(base)])))
    g1 = b"".join(p1[96 * (i % base):96 * (i % base + 1)] for i in range(count))
    g2 = b"".join(p2[192 * (i % base):192 * (i % base + 1)] for i in range(count))
    lens = (C.c_uint64 * count)(*([1] * count))
    out = np.zeros(576 * count, dtype=np.uint8)
    call = lambda: _lib.check(lib.zk_pairing_product_many(u8(g1), u8(g2), lens, count, out.ctypes.data_as(_lib._P8)))
    dt, all_ts = best_of(call)
    ref = C.create_string_buffer(576)

    def host_one(i):
        _lib.check(lib.zk_pairing_product(g1[96 * i:96 * i + 96], g2[192 * i:192 * i + 192], C.c_size_t(1), ref))
        assert ref.raw == out[576 * i:576 * (i + 1)].tobytes()

    ht, hper, hn = host_time(host_one, count)
    row = {"single_pairs": count, "device_ms": round(dt * 1e3, 3), "device_ms_all": [round(x * 1e3, 3) for x in all_ts], "host_ms": round(ht * 1e3, 1),
           "host_ms_per_call": round(hper * 1e3, 3), "host_calls_timed": hn, "host_over_device": round(ht / dt, 1)}
    print("pairing", row, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small counts only (a rehearsal)")
    a = ap.parse_args()
    _lib.check(_lib.lib().zk_init(0))
    st = RC.fr_stream(0x5EED0B16)
    rng = lambda: next(st)
    g_counts, p_counts, pair_count = ([1, 16], [16], 64) if a.quick else ([1, 16, 256, 4096], [16, 256, 1024], 4096)
    rec = {"what": "host wall ms of one batched device call (both PCIe copies) next to the same number of single-proof host calls, one process",
           "device": "MI355X", "groth16": [], "floor": {}}
    readme = [RC.readme_circuit(x) for x in range(3, 19)]
    rec["groth16"].append(groth16_case("README circuit", readme[0][0], [w for _, w in readme], rng, st, g_counts))
    cs64, w64 = RC.random_r1cs(256, 512, 12)
    assert int((cs64.mid == 0).sum()) == 64
    rec["groth16"].append(groth16_case("random R1CS, 64 public values", cs64, [w64], rng, st, g_counts))
    cub = [RC.iterated_cubic(6, x) for x in range(9, 25)]
    rec["pinocchio"] = pinocchio_case(cub[0][0], [w for _, w in cub], rng, p_counts)
    rec["pairing_product_many"] = pairing_case(pair_count, st)
    if not a.quick:          # the floor: at count = 256 the device call takes at most a tenth of 256 host calls, for both protocols
        for name, rows in (("groth16", rec["groth16"][0]["rows"]), ("groth16_64_public", rec["groth16"][1]["rows"]), ("pinocchio", rec["pinocchio"]["rows"])):
            r = next(x for x in rows if x["count"] == 256)
            rec["floor"][name] = {"host_over_device_at_256": r["host_over_device"], "holds": r["host_over_device"] >= 10.0}
    line = json.dumps(rec, indent=1)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(json.dumps({"floor": rec["floor"], "smallest_count_device_wins": {"groth16": rec["groth16"][0]["smallest_count_device_wins"],
                                                                            "pinocchio": rec["pinocchio"]["smallest_count_device_wins"]}}))
    if not all(f["holds"] for f in rec["floor"].values()):
        sys.exit("the floor is missed: a device call at count = 256 takes more than a tenth of 256 host calls")


if __name__ == "__main__":
    main()
