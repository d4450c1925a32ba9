#!/usr/bin/env python3
"""What zk_groth16_pk_contribute costs.  One MI355X (the script needs one: without a GPU every call below fails with ZK_ERR_HIP), Groth16 at 2^16 and
2^20 constraints (iterated cubic), both key forms; host wall time, best of --repeats, every run recorded so that the spread can be read.

  contribute_whole_call   Groth16.contribute on a resident handle: pools back to dense points, d1, d2, [delta']_2, the tail, new window tables
  device_ms_by_family     one call alone under zk_profile_enable(2): where its device time goes (the call's own launches are the family contribute)
For context, not as gates, on the same handle: pool_points(compressed=True) of both pools plus Groth16.from_compressed of the result -- what a host
route (read back, multiply on the host, upload again) cannot avoid, the host's multiplications not counted -- and one check_key / check_lagrange_key.
Every timed handle ends with a proof compared to the trapdoor oracle under the trapdoor it should hold by then.

The comparison that decided the tail's kernels -- a kernel of the call's own against k_aff_to_raw, k_g_tabmul, k_raw_to_aff -- was run by an earlier
form of this script on a build that held both (a measurement-only entry timed either route on a copy of the handle's tail, alternating); its
record is profiles/contribute_kernel_ab.json, and the kernel it ruled out is not in the tree.

    python scripts/bench_contribute.py --out profiles/contribute.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O                                  # noqa: E402
from zukelang_amd import _lib, r1cs as RC               # noqa: E402
from zukelang_amd.groth16 import Groth16                # noqa: E402
from zukelang_amd.r1cs import FR_MODULUS, fr_bytes      # noqa: E402


def frs(xs):
    return bytes(fr_bytes(list(xs)))


def timed(fn):
    _lib.check(_lib.lib().zk_sync())
    t0 = time.perf_counter()
    out = fn()
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


def measure(log_n, form, repeats):
    n = 1 << log_n
    cs, w = RC.iterated_cubic(n, 0xC0FFEE)
    st = RC.fr_stream(0x5EED0C00 + log_n)
    toxic = [next(st) % FR_MODULUS for _ in range(5)]
    it = iter(toxic)
    prover, pk, vk = Groth16.generate(lambda: next(it), cs, form=form)
    r, s = next(st), next(st)
    wb = prover._sol_bytes(w)
    csr = [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]
    check = prover.check_lagrange_key if form == "lagrange" else prover.check_key

    def oracle_equal(tox, what):
        got = prover.prove_rs(wb, r, s)
        want = O.groth16_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), frs(tox), frs([r]), frs([s]))
        if (got.a, got.b, got.c) != want:
            raise SystemExit("2^%d %s: the proof %s differs from the oracle's" % (log_n, form, what))

    oracle_equal(toxic, "of the generated key")
    ds = [next(st) % FR_MODULUS or 1 for _ in range(repeats + 2)]
    prover.contribute(ds[0])          # warm-up: module load, first allocations
    toxic[3] = toxic[3] * ds[0] % FR_MODULUS
    whole = []
    for d in ds[1:repeats + 1]:
        ms, _ = timed(lambda: prover.contribute(d))
        whole.append(ms)
        toxic[3] = toxic[3] * d % FR_MODULUS
    oracle_equal(toxic, "after %d contributions" % (repeats + 1))
    out = {"constraints": n, "form": form, "g1_points": prover.pool_points(1).size // 96, "tail_points": n - 1 + int(cs.mid.sum()),
           "contribute_whole_call": stats(whole)}
    L = _lib.lib()
    _lib.check(L.zk_profile_enable(2))
    _lib.check(L.zk_profile_reset())
    prover.contribute(ds[repeats + 1])
    toxic[3] = toxic[3] * ds[repeats + 1] % FR_MODULUS
    _lib.check(L.zk_sync())
    out["device_ms_by_family_one_call"] = families()
    _lib.check(L.zk_profile_enable(0))
    # context: what a host route cannot avoid, and one key check
    new_vk = vk.with_delta(bytes(prover.pool_points(2)[192:384]))
    res = check(new_vk)
    if not res.ok:
        raise SystemExit("2^%d %s: the contributed key fails its check: %s" % (log_n, form, res.names))
    out["key_check_with_vkey"] = stats([timed(lambda: check(new_vk))[0] for _ in range(repeats)])
    back, up = [], []
    for _ in range(repeats):
        ms, wires = timed(lambda: (bytes(prover.pool_points(1, compressed=True)), bytes(prover.pool_points(2, compressed=True))))
        back.append(ms)
        ms, p2 = timed(lambda: Groth16.from_compressed(cs, wires[0], wires[1], lagrange=form == "lagrange"))
        up.append(ms)
        p2.close()
    out["pool_points_compressed_both_pools"] = stats(back)
    out["upload_compressed_of_the_result"] = stats(up)
    oracle_equal(toxic, "at the end")
    prover.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contribute.json"))
    ap.add_argument("--log-n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    _lib.check(_lib.lib().zk_init(0))          # ZK_ERR_HIP without a GPU: this script measures a device
    doc = {"how": "python scripts/bench_contribute.py (host wall time, best of %d, candidates alternating; one MI355X)" % a.repeats,
           "see_also": "profiles/contribute_kernel_ab.json: the call's own kernel against the derivation's three, the run that ruled it out", "sizes": {}}
    for log_n in a.log_n:
        for form in ("tau_powers", "lagrange"):
            key = "2^%d %s" % (log_n, form)
            doc["sizes"][key] = measure(log_n, form, a.repeats)
            print(key, json.dumps({k: (v["best_ms"] if isinstance(v, dict) and "best_ms" in v else v) for k, v in doc["sizes"][key].items()
                                   if not k.startswith("device_")}), flush=True)
            with open(a.out, "w") as f:          # after every size: a run cut short keeps what it has measured
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
