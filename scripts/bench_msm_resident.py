#!/usr/bin/env python3
"""Per-call time of a multi-scalar product over a resident point list (zk_msm_resident) against the per-call path (zk_msm_g1/g2, which
uploads, checks and sets up the list on every call), and of zk_msm_resident_many with K = n products of length n (the shape of
sum_apply_powers, groth16.ml:116-121).  Every figure is host wall time per call and INCLUDES the PCIe copies (scalars in, the encoded point
out; zk_msm_g1/g2 also copies the whole list in).  Prints one JSON line.

    python scripts/bench_msm_resident.py                       # the built library: each length takes the path its short_max picks
    python scripts/bench_msm_resident.py --sweep                # both paths at every length: the variant libraries of `make -C
                                                                # zukelang_amd/csrc resident-sweep` (short_max 0: always the chain;
                                                                # 8192: the short path up to 2^13), one child process each
short_max of msm_resident.hip (per group) is the crossover of the --sweep figures for K = n products (profiles/msm_resident.json).
Per length the rows also carry:
  resident_ms     one zk_msm_resident call of n scalars (a lone product: the chain, unless the short path's lone rule picks it)
  short_pair_ms   (n <= short_max) one _many call of that product plus a one-scalar product: both on the short path, i.e. what a lone
                  product costs there -- with resident_ms of the variant 0 library the evidence behind LONE_RATIO_G1 / _G2
  prefix16_*      (n >= 2^16) a 16-scalar prefix of the list: zk_msm_g1/g2 over 16 points, zk_msm_resident (the lone rule picks the path),
                  and, on the variant 0 library, the chain over all n points"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [16, 64, 256, 1024, 2048, 4096, 8192, 1 << 16, 1 << 20]


def _time(fn, reps):
    fn()                                                     # warm-up: first-call set-up stays out of the figure
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    ts.sort()
    return 1e3 * ts[len(ts) // 2]


def run(sizes, many_max, groups):
    import numpy as np
    from zukelang_amd import _lib
    from zukelang_amd import r1cs as RC
    from zukelang_amd.curve import G1, G2
    _lib.check(_lib.lib().zk_init(0))
    rows, many = [], []
    for gname in groups:
        G = G1 if gname == "G1" else G2
        for n in sizes:
            bases = np.array(G.of_Fr(RC.random_fr_bytes(n, 11 + n)), dtype=np.uint8)
            sc = np.array(RC.random_fr_bytes(n, 23 + n), dtype=np.uint8)
            t = time.perf_counter()
            rb = G.resident(bases)
            up = 1e3 * (time.perf_counter() - t)
            reps = 30 if n <= 8192 else (10 if n <= 1 << 16 else 4)
            assert bytes(rb.apply_powers(sc)) == bytes(G.apply_powers(sc, bases))
            row = {"group": gname, "n": n, "upload_ms": round(up, 3),
                   "zk_msm_ms": round(_time(lambda: G.apply_powers(sc, bases), reps), 4),
                   "resident_ms": round(_time(lambda: rb.apply_powers(sc), reps), 4)}
            if n <= rb.short_max:
                pair = [sc, sc[:32]]
                assert [bytes(p) for p in rb.apply_powers_many(pair)] == [bytes(rb.apply_powers(c)) for c in pair]
                row["short_pair_ms"] = round(_time(lambda: rb.apply_powers_many(pair), reps), 4)
            if n >= 1 << 16:
                p16, b16 = sc[:16 * 32], bases[:16 * G.POINT_BYTES]
                assert bytes(rb.apply_powers(p16)) == bytes(G.apply_powers(p16, b16))
                row["prefix16_zk_msm_ms"] = round(_time(lambda: G.apply_powers(p16, b16), reps), 4)
                row["prefix16_resident_ms"] = round(_time(lambda: rb.apply_powers(p16), reps), 4)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            if n <= many_max:
                cs = [sc] * n
                ms = _time(lambda: rb.apply_powers_many(cs), 3)
                m = {"group": gname, "n": n, "K": n, "path": "short" if n <= rb.short_max else "long", "many_ms": round(ms, 3), "many_per_product_ms": round(ms / n, 5),
                     "zk_msm_K_calls_ms": round(row["zk_msm_ms"] * n, 3)}
                many.append(m)
                print(json.dumps(m), file=sys.stderr, flush=True)
            rb.close()
    return {"short_max": _short_max(), "rows": rows, "many": many}


def _short_max():
    from zukelang_amd.curve import G1
    from zukelang_amd.curve import G2
    out = {}
    for name, G in (("G1", G1), ("G2", G2)):
        with G.resident(G.of_Fr(bytes([1]) + bytes(31))) as rb:
            out[name] = rb.short_max
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--many-max", type=int, default=1024)
    ap.add_argument("--groups", default="G1,G2")
    ap.add_argument("--sweep", action="store_true", help="both paths at every length (variant libraries, one child process each)")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    groups = a.groups.split(",")
    if not a.sweep:
        res = run(sizes, a.many_max, groups)
        res.update({"what": "ms per call, host wall time incl. PCIe copies (median)", "library": os.environ.get("ZK_LIBZKMI355X_PATH", "built")})
        print(json.dumps(res), flush=True)
        return
    out = {"what": "ms per call, host wall time incl. PCIe copies (median); per variant library: short_max 0 = every product on the Pippenger chain, "
                   "8192 = the two-launch short path for products of up to 2^13 scalars (two or more per call, or a lone one on a long list)", "variants": {}}
    for v, vs in (("0", sizes), ("8192", [s for s in sizes if s <= 8192])):
        lib = os.path.join(ROOT, "zukelang_amd", "libzkmi355x_short%s.so" % v)
        env = dict(os.environ, ZK_LIBZKMI355X_PATH=lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--sizes", ",".join(str(s) for s in vs), "--many-max", str(a.many_max),
                            "--groups", a.groups], env=env, stdout=subprocess.PIPE, timeout=900)
        if p.returncode != 0:
            raise SystemExit("variant %s: exit %d" % (v, p.returncode))
        out["variants"][v] = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
