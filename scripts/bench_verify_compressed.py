#!/usr/bin/env python3
"""Proofs off the wire under a resident key on one MI355X, in ONE process: host wall time from compressed proof bytes to verdicts, every PCIe copy included.

For Groth16 and Pinocchio under the README circuit's key, at 256, 4096 and 16384 proofs, three routes from the same 192 / 480 wire bytes per proof:
  (a) zk_g1_decompress / zk_g2_decompress per point on the host, then zk_*_verify_resident          (256 proofs only: it is linear in the count)
  (b) zk_g1_decompress_batch + zk_g2_decompress_batch over the batch's points, the proofs put together again on the host, then zk_*_verify_resident
  (c) zk_*_verify_resident_compressed
and, as the floor, zk_*_verify_resident on proofs that were decompressed beforehand.  After one warm-up of each, (b), (c) and the floor ALTERNATE five
times; a figure is the best of five, its spread the largest minus the smallest of the five.  Every route's verdicts are checked outside the timed
region, (b)'s reassembled proofs against the floor's bytes.  The record also holds the device time of (c)'s verify_point_decompress and
verify_point_checks families at each count (a pass of its own with the timers on), and "holds": whether (c) beats (b) at 4096 proofs by more than
(b)'s spread.
--g2-root LIB [LIB ...]: before anything else, one child process per library (ZK_LIBZKMI355X_PATH) times zk_g2_decompress_batch on 4096 points -- the
G2 decompression with the square root of that build -- so that the build before the two-power root and this one stand side by side in the record.
Usage: python scripts/bench_verify_compressed.py [--out profiles/verify_compressed.json] [--quick] [--g2-root name=path ...]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

FAMILIES = ["verify_point_decompress", "verify_point_checks", "msm_short", "pairing_miller", "pairing_final_exp"]
REPS = 5
G16_FIELDS = (1, 2, 1)                          # A B C: the group of each point of the wire form, in order
PIN_FIELDS = (1, 2, 1, 1, 1, 2, 1, 1)           # vv ww yy h vavv waww yayy bvwy


def ms(ts):
    return {"best_ms": round(min(ts) * 1e3, 3), "all_ms": [round(t * 1e3, 3) for t in ts], "spread_ms": round((max(ts) - min(ts)) * 1e3, 3)}


def g2_root_child():
    """zk_g2_decompress_batch on 4096 points of the library this process loaded: best of five after a warm-up, as JSON on stdout"""
    from zukelang_amd import _lib, r1cs as RC
    from zukelang_amd.curve import G2
    _lib.check(_lib.lib().zk_init(0))
    st = RC.fr_stream(0x5EED0C02)
    pts = G2.of_Fr(RC.fr_bytes([next(st) for _ in range(4096)]))
    comp = np.frombuffer(b"".join(G2.to_compressed_bytes(pts[192 * i:192 * (i + 1)]) for i in range(4096)), dtype=np.uint8)
    out = np.zeros(192 * 4096, dtype=np.uint8)
    run = lambda: _lib.check(_lib.lib().zk_g2_decompress_batch(comp.ctypes.data_as(C.c_void_p), C.c_size_t(4096), out.ctypes.data_as(C.c_void_p)))
    run()
    assert bytes(out) == bytes(pts)
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t)
    print(json.dumps(ms(ts)))


def g2_root(libs):
    out = {"what": "host wall ms of zk_g2_decompress_batch on 4096 compressed G2 points (copies, square roots, [r]P = O, encoding), one process per build"}
    for spec in libs:
        name, path = spec.split("=", 1)
        env = dict(os.environ, ZK_LIBZKMI355X_PATH=os.path.abspath(path))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--g2-root-child"], env=env, capture_output=True, text=True, timeout=300)
        if res.returncode:
            sys.exit("the child for %s failed:\n%s" % (name, res.stderr[-2000:]))
        out[name] = json.loads(res.stdout.strip().splitlines()[-1])
        print("g2 decompression,", name, out[name], flush=True)
    return out


def protocol_case(name, fields, wire, plain, ios, n_io, handle, counts, quick):
    """wire / plain: the proofs as wire bytes and as uncompressed bytes (lists); ios: their public inputs"""
    from zukelang_amd import _lib
    lib = _lib.lib()
    res = getattr(lib, "zk_%s_verify_resident" % name)
    res_c = getattr(lib, "zk_%s_verify_resident_compressed" % name)
    stride_c, stride_u = 48 * sum(fields), 96 * sum(fields)
    offs_c = np.cumsum([0] + [48 * g for g in fields])
    offs_u = np.cumsum([0] + [96 * g for g in fields])
    g1_at = [q for q, g in enumerate(fields) if g == 1]
    g2_at = [q for q, g in enumerate(fields) if g == 2]
    p8 = lambda a: a.ctypes.data_as(_lib._P8)
    rows = []
    for count in counts:
        w_all = np.frombuffer(b"".join(wire[i % len(wire)] for i in range(count)), dtype=np.uint8).reshape(count, stride_c)
        u_all = np.frombuffer(b"".join(plain[i % len(plain)] for i in range(count)), dtype=np.uint8).reshape(count, stride_u)
        io_all = np.frombuffer(b"".join(ios[i % len(ios)] for i in range(count)), dtype=np.uint8)
        ok, st = np.zeros(count, dtype=np.uint8), np.zeros(count, dtype=np.int32)
        pst = st.ctypes.data_as(_lib._PI32)
        h = C.c_uint64(handle)
        built = {}

        def verify(fn, proofs):
            ok[:] = 0
            st[:] = 9
            _lib.check(fn(h, p8(io_all), p8(proofs), count, p8(ok), pst))

        def reassemble(d1, d2):
            out = np.empty((count, stride_u), dtype=np.uint8)
            d1, d2 = d1.reshape(count, len(g1_at), 96), d2.reshape(count, len(g2_at), 192)
            for j, q in enumerate(g1_at):
                out[:, offs_u[q]:offs_u[q] + 96] = d1[:, j]
            for j, q in enumerate(g2_at):
                out[:, offs_u[q]:offs_u[q] + 192] = d2[:, j]
            return out

        def gather():
            c1 = np.ascontiguousarray(np.stack([w_all[:, offs_c[q]:offs_c[q] + 48] for q in g1_at], axis=1))
            c2 = np.ascontiguousarray(np.stack([w_all[:, offs_c[q]:offs_c[q] + 96] for q in g2_at], axis=1))
            return c1, c2

        def route_a():
            c1, c2 = gather()
            d1, d2 = np.empty((count * len(g1_at), 96), dtype=np.uint8), np.empty((count * len(g2_at), 192), dtype=np.uint8)
            c1, c2 = c1.reshape(-1, 48), c2.reshape(-1, 96)
            for i in range(len(c1)):
                _lib.check(lib.zk_g1_decompress(p8(c1[i]), p8(d1[i])))
            for i in range(len(c2)):
                _lib.check(lib.zk_g2_decompress(p8(c2[i]), p8(d2[i])))
            built["a"] = reassemble(d1, d2)
            verify(res, built["a"])

        def route_b():
            c1, c2 = gather()
            d1, d2 = np.empty(count * len(g1_at) * 96, dtype=np.uint8), np.empty(count * len(g2_at) * 192, dtype=np.uint8)
            _lib.check(lib.zk_g1_decompress_batch(c1.ctypes.data_as(C.c_void_p), C.c_size_t(count * len(g1_at)), d1.ctypes.data_as(C.c_void_p)))
            _lib.check(lib.zk_g2_decompress_batch(c2.ctypes.data_as(C.c_void_p), C.c_size_t(count * len(g2_at)), d2.ctypes.data_as(C.c_void_p)))
            built["b"] = reassemble(d1, d2)
            verify(res, built["b"])

        route_c = lambda: verify(res_c, w_all)
        floor = lambda: verify(res, u_all)
        routes = (("b", route_b), ("c", route_c), ("floor", floor))
        times = {k: [] for k, _ in routes}
        for k, run in routes:                                   # warm-up, and the verdicts of every route
            run()
            assert ok.all() and not st.any(), (name, count, k)
        assert (built["b"] == u_all).all()
        for _ in range(REPS):
            for k, run in routes:
                t = time.perf_counter()
                run()
                times[k].append(time.perf_counter() - t)
        row = {"count": count, "b_batch_decompress_then_resident": ms(times["b"]), "c_resident_compressed": ms(times["c"]),
               "floor_resident_on_decompressed_proofs": ms(times["floor"])}
        b, c = row["b_batch_decompress_then_resident"], row["c_resident_compressed"]
        row["b_over_c"] = round(b["best_ms"] / c["best_ms"], 2)
        row["c_beats_b_by_more_than_the_spread_of_b"] = b["best_ms"] - c["best_ms"] > b["spread_ms"]
        if count == counts[0]:
            route_a()
            assert ok.all() and not st.any() and (built["a"] == u_all).all()
            ta = []
            for _ in range(1 if quick else 3):
                t = time.perf_counter()
                route_a()
                ta.append(time.perf_counter() - t)
            row["a_host_decompress_per_point_then_resident"] = ms(ta)
        # (c)'s kernel families, timers on: a pass of its own
        _lib.check(lib.zk_profile_enable(2))
        _lib.check(lib.zk_profile_reset())
        route_c()
        fam = {}
        for f in FAMILIES:
            t_ms, cnt = C.c_double(), C.c_uint64()
            _lib.check(lib.zk_profile_get(f.encode(), C.byref(t_ms), C.byref(cnt)))
            if cnt.value:
                fam[f] = {"ms": round(t_ms.value, 3), "launches": cnt.value}
        _lib.check(lib.zk_profile_enable(0))
        _lib.check(lib.zk_profile_reset())
        row["c_kernel_families"] = fam
        rows.append(row)
        print(name, json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small counts only (a rehearsal)")
    ap.add_argument("--g2-root", nargs="*", default=[], metavar="NAME=LIB", help="builds of the library whose G2 decompression is timed first, one child process each")
    ap.add_argument("--g2-root-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.g2_root_child:
        return g2_root_child()
    rec = {"what": "host wall ms from compressed proof bytes to verdicts under a resident key, README circuit, one process; (b), (c) and the floor alternate, "
                   "best of %d each, spread = max - min of the %d timings of one route" % (REPS, REPS), "device": "MI355X"}
    if a.g2_root:
        rec["g2_decompress_batch_4096"] = g2_root(a.g2_root)          # before this process opens the device
    from zukelang_amd import _lib, r1cs as RC, pinocchio as PIN
    from zukelang_amd.groth16 import Groth16
    lib = _lib.lib()
    _lib.check(lib.zk_init(0))
    st = RC.fr_stream(0x5EED0C17)
    rng = lambda: next(st)
    counts = [32, 256] if a.quick else [256, 4096, 16384]
    readme = [RC.readme_circuit(x) for x in range(3, 19)]
    cs, wits = readme[0][0], [w for _, w in readme]
    ios = [bytes(RC.fr_bytes([w[k] for k in range(cs.m) if not cs.mid[k]])) for w in wits]
    n_io = len(ios[0]) // 32
    u8 = lambda b: C.cast(C.c_char_p(bytes(b)), _lib._P8) if len(b) else None
    # Groth16
    prover, _, vk = Groth16.generate(rng, cs)
    proofs = [prover.prove_rs(w, next(st), next(st)) for w in wits]
    prover.close()
    lt = bytes(np.ascontiguousarray(vk.ltgm_io, dtype=np.uint8))
    h = C.c_uint64(0)
    _lib.check(lib.zk_groth16_vk_upload(u8(vk.ab), u8(lt), n_io, u8(vk.gm), u8(vk.d), C.byref(h)))
    rec["groth16"] = protocol_case("groth16", G16_FIELDS, [p.to_compressed() for p in proofs], [bytes(p.a) + bytes(p.b) + bytes(p.c) for p in proofs], ios, n_io,
                                   h.value, counts, a.quick)
    _lib.check(lib.zk_vk_free(h))
    # Pinocchio
    pprover, _, pvk = PIN.ZK.generate(rng, cs)
    pp = [pprover.prove(rng, w) for w in wits]
    pprover.close()
    g1, g2 = bytes(np.ascontiguousarray(pvk.g1, dtype=np.uint8)), bytes(np.ascontiguousarray(pvk.g2, dtype=np.uint8))
    h = C.c_uint64(0)
    _lib.check(lib.zk_pinocchio_vk_upload(u8(g1), u8(g2), n_io, C.byref(h)))
    rec["pinocchio"] = protocol_case("pinocchio", PIN_FIELDS, [p.to_compressed() for p in pp], [p.to_bytes() for p in pp], ios, n_io, h.value, counts, a.quick)
    _lib.check(lib.zk_vk_free(h))
    at = counts[1]
    rec["holds"] = {"c_beats_b_at_%d_by_more_than_the_spread_of_b" % at: {k: next(r for r in rec[k] if r["count"] == at)["c_beats_b_by_more_than_the_spread_of_b"]
                                                                        for k in ("groth16", "pinocchio")}}
    if a.out:
        open(a.out, "w").write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec["holds"]))


if __name__ == "__main__":
    main()
