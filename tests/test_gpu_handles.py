"""Every kind of handle answers a handle of every OTHER kind with ZK_ERR_HANDLE (csrc/handle_table.h: one table type, one 2^32 range per kind).

Four kinds are alive at once -- a Groth16 key, a Pinocchio key, resident MSM bases, a resident verification key -- first on the one-entry device
list (single-device keys), then, after everything is freed, on a two-entry list (multi-device keys: the other two key tables).  The free, info and
reserve entry points are called with the live handle of every other kind; nothing may be touched: every handle then gives the bytes it gave before,
frees exactly once, and the live count is back at 0 (the device list can change).  The README circuit, 4 G1 points, fixed r, s and deltas."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyref as P
from zukelang_amd import _lib, r1cs as RC
from zukelang_amd import pinocchio as PIN
from zukelang_amd.curve import G1
from zukelang_amd.groth16 import Groth16
from test_gpu_multidevice import physical, seeded_rng

pytestmark = pytest.mark.gpu

ZK_ERR_HANDLE = -7
H = lambda h: C.c_uint64(h)
# (name, call on a raw handle number, the kinds whose handles it serves)
FOREIGN_CALLS = [
    ("zk_bases_info", lambda L, h: L.zk_bases_info(H(h), None, None, None), {"bases"}),
    ("zk_vk_info", lambda L, h: L.zk_vk_info(H(h), None, None), {"vk"}),
    ("zk_pinocchio_reserve_slots", lambda L, h: L.zk_pinocchio_reserve_slots(H(h), C.c_uint32(1)), {"pinocchio"}),
    ("zk_groth16_pk_free", lambda L, h: L.zk_groth16_pk_free(H(h)), {"groth16"}),
    ("zk_pinocchio_pk_free", lambda L, h: L.zk_pinocchio_pk_free(H(h)), {"pinocchio"}),
    ("zk_bases_free", lambda L, h: L.zk_bases_free(H(h)), {"bases"}),
    ("zk_vk_free", lambda L, h: L.zk_vk_free(H(h)), {"vk"}),
]
FREE = {"groth16": "zk_groth16_pk_free", "pinocchio": "zk_pinocchio_pk_free", "bases": "zk_bases_free", "vk": "zk_vk_free"}


@pytest.fixture(scope="module")
def material():
    """keys, points and blinding values, made once: both phases use the same, so both must give the same bytes"""
    _lib.check(_lib.lib().zk_init(0))
    cs, w = RC.readme_circuit(3)
    rng = seeded_rng(0x5EED0A11)
    gpk, gvk = Groth16.keygen(rng, cs)
    ppk, _ = PIN.ZK.keygen(rng, cs)
    points = np.array(G1.of_Fr(RC.random_fr_bytes(4, 0xBA5E5)), dtype=np.uint8).reshape(-1)
    scalars = b"".join(P.fr_to_bytes(rng()) for _ in range(4))
    return dict(cs=cs, w=w, gpk=gpk, gvk=gvk, ppk=ppk, points=points, scalars=scalars, rs=(rng(), rng()), deltas=(rng(), rng(), rng()),
                io=[w[k] for k in range(cs.m) if not cs.mid[k]])


def _phase(m, devs):
    L = _lib.lib()
    _lib.set_device_list(devs)
    assert _lib.device_list() == devs
    g16, pin = Groth16(m["cs"], m["gpk"]), PIN.ZK(m["cs"], m["ppk"])
    bases, vk = G1.resident(m["points"]), m["gvk"].resident()
    objs = {"groth16": g16, "pinocchio": pin, "bases": bases, "vk": vk}
    num = {"groth16": g16.handle.value, "pinocchio": pin.handle.value, "bases": bases.handle, "vk": vk.handle}

    try:
        def outputs():
            proof = g16.prove_rs(m["w"], *m["rs"])
            return dict(groth16=bytes(proof.a) + bytes(proof.b) + bytes(proof.c), pinocchio=pin.prove_with(m["w"], *m["deltas"]).to_bytes(),
                        bases=bytes(bases.apply_powers(m["scalars"])), vk=vk.verify_many([m["io"]], [proof]))

        before = outputs()
        assert before["vk"] == [True]
        # every violation is collected, so that one run names them all; the calls that free come last
        problems = [("same range", a, b) for a in num for b in num if a < b and num[a] >> 32 == num[b] >> 32]
        for name, call, own in FOREIGN_CALLS:
            for kind, h in num.items():
                if kind not in own:
                    rc = call(L, h)
                    if rc != ZK_ERR_HANDLE:
                        problems.append((name, "called with the live %s handle 0x%x" % (kind, h), "returned %d" % rc))
        assert problems == []
        assert outputs() == before                                             # nothing was touched
        with pytest.raises(_lib.ZkError):
            _lib.set_device_list([0] if len(devs) > 1 else [0, 0])             # four live handles pin the device list
        for kind, obj in objs.items():
            free = getattr(L, FREE[kind])
            assert free(H(num[kind])) == 0, kind
            assert free(H(num[kind])) == ZK_ERR_HANDLE, kind
            obj.handle = None                                                  # freed here: nothing is left for close()
    finally:
        for obj in objs.values():                                              # a failed check: nothing stays alive behind it, and the
            try:                                                               # assertion that failed is the one that is reported
                obj.close()
            except Exception:
                pass
    _lib.set_device_list([0])                                              # the live count is back at 0
    assert _lib.device_list() == [0]
    return before


def test_no_table_answers_a_handle_of_another_kind(material):
    try:
        single = _phase(material, [0])                                     # single-device keys
        multi = _phase(material, physical([0, 0]))                         # multi-device keys: the other two key tables
        assert multi == single                                             # the sums do not depend on how the pools are cut
    finally:
        _lib.set_device_list([0])
