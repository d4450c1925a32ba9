#!/usr/bin/env python3
"""Key generation on one MI355X: host wall time from the trapdoor to a key handle that has produced one proof, three ways, in ONE process.

  (i)   the host-side path: Groth16.keygen(lagrange=True) + upload of the Lagrange-form pools (exponents in Python integers, points through
        zk_g1/g2_of_fr, then zk_groth16_pk_upload_lagrange).  Pinocchio has no Lagrange-form keygen on the host, so there it is keygen + upload +
        derive_lagrange.
  (ii)  zk_*_keygen with the key bytes requested (Groth16.generate / pinocchio.generate: what a host that also stores the key calls)
  (iii) zk_*_keygen with the handle only

Every timed region ends after one blocking proof; the proofs are compared with the trapdoor oracle OUTSIDE the timed regions (a run whose proof is
wrong writes no result).  (ii) and (iii) run twice after a warm-up at a small size; both times are recorded, the first is quoted.  Per-kernel times come
from zk_profile_get in a pass of its own (event timers serialise the launches).  Sizes: Groth16 2^16 and 2^20, Pinocchio 2^18 (the sizes bench.py and
scripts/bench_pinocchio.py measure).  Usage: python scripts/bench_keygen.py [--out profiles/keygen_device.json] [--sizes 16,20] [--pin-size 18] [--skip-host]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import oracle_lib as O  # noqa: E402
from zukelang_amd import _lib, r1cs as RC, pinocchio as PIN  # noqa: E402
from zukelang_amd.groth16 import Groth16, _csr, _p  # noqa: E402

FAMILIES = ["keygen_lagrange", "keygen_powers", "keygen_columns", "keygen_assemble", "fixed_base_mul", "msm_precompute"]
frs = lambda xs: bytes(RC.fr_bytes(xs))
csrs = lambda cs: [O.CSR(M.ptr, M.col, M.val) for M in (cs.L, cs.R, cs.O)]


def handle_only(proto, cs, toxic):
    """(iii): no output buffer at all"""
    fn = _lib.lib().zk_groth16_keygen if proto == "groth16" else _lib.lib().zk_pinocchio_keygen
    mid = np.ascontiguousarray(cs.mid, dtype=np.uint8)
    L, R, Oo = _csr(cs.L), _csr(cs.R), _csr(cs.O)
    h = C.c_uint64()
    _lib.check(fn(cs.n, cs.m, C.byref(L), C.byref(R), C.byref(Oo), _p(mid), _p(np.frombuffer(toxic, dtype=np.uint8).copy()), 1, None, 0, None, 0, None, None, C.byref(h)))
    cls = Groth16 if proto == "groth16" else PIN.ZK
    pr = cls.__new__(cls)
    pr.circuit, pr._keep, pr.handle = cs, (cs,), h
    if proto == "groth16":
        pr.rank, pr.world = 0, 1
    return pr


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
    _lib.check(L.zk_profile_reset())
    return out


def bench_groth16(log_n, skip_host):
    n = 1 << log_n
    cs, w = RC.iterated_cubic(n, next(RC.fr_stream(0x5EED0001)))
    st = RC.fr_stream(0x5EED0002)
    tox = [next(st) for _ in range(5)]
    r, s = next(st), next(st)
    wb = RC.fr_bytes(w)
    want = O.groth16_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, frs(w), frs(tox), frs([r]), frs([s]))
    res = {"protocol": "groth16", "constraints": n}
    proofs = []

    def timed(tag, make):
        _lib.check(_lib.lib().zk_sync())
        t0 = time.perf_counter()
        pr = make()
        p = pr.prove_rs(wb, r, s)
        dt = time.perf_counter() - t0
        proofs.append((tag, (p.a, p.b, p.c)))
        pr.close()
        return round(dt, 4)

    def host_path():
        it = iter(tox)
        pk, _vk = Groth16.keygen(lambda: next(it), cs, lagrange=True)
        return Groth16(cs, pk, lagrange=True)

    def with_bytes():
        it = iter(tox)
        return Groth16.generate(lambda: next(it), cs, form="lagrange")[0]

    if not skip_host:
        res["host_keygen_lagrange_upload_s"] = timed("host", host_path)
    res["device_keygen_with_bytes_s"] = [timed("bytes", with_bytes) for _ in range(2)]
    res["device_keygen_handle_only_s"] = [timed("handle", lambda: handle_only("groth16", cs, frs(tox))) for _ in range(2)]
    for tag, got in proofs:
        assert got == want, "groth16 2^%d: the proof of path %s differs from the trapdoor oracle" % (log_n, tag)
    res["kernels_with_bytes"] = profile_pass(lambda: with_bytes().close())
    res["proofs_equal_the_trapdoor_oracle"] = len(proofs)
    return res


def bench_pinocchio(log_n, skip_host):
    n = 1 << log_n
    cs, w = RC.iterated_cubic(n, next(RC.fr_stream(0x5EED0001)))
    st = RC.fr_stream(0x5EED0003)
    tox = [next(st) for _ in range(8)]
    d = [next(st) for _ in range(3)]
    wb = RC.fr_bytes(w)
    want = O.pinocchio_prove_trapdoor(cs.n, cs.m, *csrs(cs), cs.mid, frs(w), frs(tox), *(frs([x]) for x in d))
    res = {"protocol": "pinocchio", "constraints": n}
    proofs = []

    def timed(tag, make):
        _lib.check(_lib.lib().zk_sync())
        t0 = time.perf_counter()
        pr = make()
        p = pr.prove_with(wb, *d)
        dt = time.perf_counter() - t0
        proofs.append((tag, p.to_bytes()))
        pr.close()
        return round(dt, 4)

    def host_path():
        it = iter(tox)
        pk, _vk = PIN.ZK.keygen(lambda: next(it), cs)
        pr = PIN.ZK(cs, pk)
        pr.derive_lagrange()
        return pr

    def with_bytes():
        it = iter(tox)
        return PIN.ZK.generate(lambda: next(it), cs, form="lagrange")[0]

    if not skip_host:
        res["host_keygen_upload_derive_s"] = timed("host", host_path)
    res["device_keygen_with_bytes_s"] = [timed("bytes", with_bytes) for _ in range(2)]
    res["device_keygen_handle_only_s"] = [timed("handle", lambda: handle_only("pinocchio", cs, frs(tox))) for _ in range(2)]
    for tag, got in proofs:
        assert got == want, "pinocchio 2^%d: the proof of path %s differs from the trapdoor oracle" % (log_n, tag)
    res["kernels_with_bytes"] = profile_pass(lambda: with_bytes().close())
    res["proofs_equal_the_trapdoor_oracle"] = len(proofs)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keygen_device.json"))
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--pin-size", type=int, default=18)
    ap.add_argument("--skip-host", action="store_true", help="leave out path (i), the slow host-side keygen")
    a = ap.parse_args()
    _lib.check(_lib.lib().zk_init(0))
    # warm-up: code objects, generator tables, the Python paths -- at a small size, both protocols
    cs, _w = RC.iterated_cubic(1 << 10, 5)
    st = RC.fr_stream(1)
    Groth16.generate(lambda: next(st), cs)[0].close()
    PIN.ZK.generate(lambda: next(st), cs)[0].close()
    runs = [bench_groth16(int(x), a.skip_host) for x in a.sizes.split(",") if x]
    if a.pin_size:
        runs.append(bench_pinocchio(a.pin_size, a.skip_host))
    out = {"what": "host wall time in seconds from the trapdoor to a Lagrange-form key handle that has produced one proof (scripts/bench_keygen.py); "
                   "device paths: two runs each, in order; kernels_with_bytes: per-family device time of one zk_*_keygen call with key bytes",
           "circuit": "iterated cubic (the benchmark family)", "devices": 1, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
