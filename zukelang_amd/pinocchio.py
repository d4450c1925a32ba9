"""Host-side mirror of `Pinocchio.Make(C).{NonZK, ZK} : Protocol.S` (src/pinocchio/pinocchio.mli:3-15)
for the prove path, backed by the HIP library.

  keygen rng circuit  -> (pkey, vkey)   pinocchio.ml:530-534 -> KeyGen.generate :77-189
                                         (rng draws rv, rw, s, av, aw, ay, b, gm in that order, :83-91)
  ZK.prove rng sol    -> proof           :559-561 -> ZKCompute.f :427-514 (draws dv, dw, dy, :428-430)
  NonZK.prove _ sol   -> proof           :536-538 -> Compute.f :210-248 (no randomness)

Key and proof layouts are those of include/zkmi355x.h.  An unsatisfied witness raises AssertionError
(QAP.ml:134).  `verify` (13 pairings, :254-420) is outside the accelerated path (scope row f1).
"""
import ctypes as C
import secrets
from dataclasses import dataclass

import numpy as np

from . import _lib
from .curve import G1, G2
from .groth16 import _csr, _lagrange_at, _many_witnesses, _p, _prove_many, columns_at, ResidentVKey, ZK_ERR_REMAINDER
from .r1cs import FR_MODULUS, R1CS, fr_bytes


@dataclass
class PKey:
    g1: np.ndarray   # vv | yy | vav | yay | bvwy | si | v_all | w_all | vt | yt | vavt | yayt | vbt | wbt | ybt
    g2: np.ndarray   # ww | waw | si2 | wt | wawt


def _draw_rho_row():
    """Five times 16 bytes from the operating system's generator as little-endian integers; a zero is drawn again"""
    row = []
    while len(row) < 5:
        r = int.from_bytes(secrets.token_bytes(16), "little")
        if r:
            row.append(r)
    return row


class PinocchioResidentVKey(ResidentVKey):
    """What VKey.resident() returns: the resident key of groth16.ResidentVKey with the folded check of zk_pinocchio_verify_folded.  A proof is a Proof
    or its 960 bytes; with compressed=True a Proof or its 480 wire bytes."""

    def __init__(self, handle, n_io):
        super().__init__(handle, n_io, lambda p: bytes(p if isinstance(p, (bytes, bytearray)) else p.to_bytes()), 960, "zk_pinocchio_verify_resident")

    def verify_all(self, input_outputs, proofs, rho=None, return_status=False, compressed=False):
        """Are ALL of these proofs good?  One folded pairing equation for the batch (zk_pinocchio_verify_folded) instead of five per proof: True, or
        False when any proof is bad -- verify_many then says which.  rho: one row of FIVE coefficients 0 < rho < 2^128 per proof, one per equation of
        Verify.f.  Leave it None: the rows are then drawn from `secrets` here, after the proofs are fixed.  A caller that passes its own takes over the
        contract of include/zkmi355x.h -- drawn after the proofs are fixed, unpredictable to whoever made them, five independent ones per proof --
        without which a bad batch, or a single bad proof, can be made to pass."""
        count, io_all, pr_all = self._batch("verify_all", input_outputs, proofs, compressed)
        if rho is None:
            rho = [_draw_rho_row() for _ in range(count)]
        try:
            rho = [[int(r) for r in row] for row in rho]
        except TypeError:
            raise ValueError("verify_all: need one row of five coefficients per proof") from None
        if len(rho) != count or any(len(row) != 5 or any(not 0 < r < 1 << 128 for r in row) for row in rho):
            raise ValueError("verify_all: need one row of five coefficients 0 < rho < 2^128 per proof")
        rho_all = np.frombuffer(b"".join(r.to_bytes(16, "little") for row in rho for r in row), dtype=np.uint8)
        all_ok = C.c_int(0)
        status = np.zeros(max(count, 1), dtype=np.int32)
        call = _lib.lib().zk_pinocchio_verify_folded_compressed if compressed else _lib.lib().zk_pinocchio_verify_folded
        _lib.check(call(C.c_uint64(self.handle), _p(io_all) if self.n_io and count else None, _p(pr_all) if count else None,
                        _p(rho_all) if count else None, C.c_uint32(count), C.byref(all_ok), status.ctypes.data_as(C.POINTER(C.c_int32))))
        return (bool(all_ok.value), [int(x) for x in status[:count]]) if return_status else bool(all_ok.value)

    def verify_many(self, input_outputs, proofs, return_status=False, fold_first=False, compressed=False):
        """fold_first: ask verify_all first (rho drawn here) and answer all-true when it says so; only a batch that holds a bad proof pays for the
        per-proof call as well.  Off by default: the call is then exactly the per-proof one."""
        proofs, input_outputs = list(proofs), list(input_outputs)
        if fold_first and self.verify_all(input_outputs, proofs, compressed=compressed):
            return ([True] * len(proofs), [0] * len(proofs)) if return_status else [True] * len(proofs)
        return super().verify_many(input_outputs, proofs, return_status=return_status, compressed=compressed)


@dataclass
class VKey:
    g1: np.ndarray   # one | aw | bgm | vv_io | yy_io
    g2: np.ndarray   # one2 | av | ay | gm2 | bgm2 | yt | ww_io

    def resident(self):
        """This key on the device (zk_pinocchio_vk_upload): its points decoded and checked once, then verify_many(input_outputs, proofs) per batch."""
        g1 = np.ascontiguousarray(self.g1, dtype=np.uint8).reshape(-1)
        g2 = np.ascontiguousarray(self.g2, dtype=np.uint8).reshape(-1)
        n_io = len(g2) // 192 - 6
        if n_io < 0 or len(g1) != 96 * (3 + 2 * n_io) or len(g2) != 192 * (6 + n_io):
            raise AssertionError("Variable not found")
        h = C.c_uint64(0)
        _lib.check(_lib.lib().zk_pinocchio_vk_upload(_p(g1), _p(g2), C.c_size_t(n_io), C.byref(h)))
        return PinocchioResidentVKey(h.value, n_io)


@dataclass
class Proof:
    """Compute.proof (pinocchio.ml:195-208), fields in declaration order."""
    vv: bytes
    ww: bytes
    yy: bytes
    h: bytes
    vavv: bytes
    waww: bytes
    yayy: bytes
    bvwy: bytes

    def to_bytes(self):
        return self.vv + self.ww + self.yy + self.h + self.vavv + self.waww + self.yayy + self.bvwy

    def to_compressed(self):
        c1, c2 = G1.to_compressed_bytes, G2.to_compressed_bytes
        return c1(self.vv) + c2(self.ww) + c1(self.yy) + c1(self.h) + c1(self.vavv) + c2(self.waww) + c1(self.yayy) + c1(self.bvwy)


def _uks(circuit, s):
    """v_k(s), w_k(s), y_k(s) for every variable and t(s), through the Lagrange basis of 0..n-1."""
    lag, t = _lagrange_at(circuit.n, s)
    vk, wk, yk = columns_at(circuit, lag)          # three sparse products M^T x on the GPU (zk_fr_spmv)
    return vk, wk, yk, t


def generate(rng, circuit: R1CS, form="lagrange", zk=True):
    """(prover, pkey, vkey) from one library call: ZK.generate / NonZK.generate (zk_pinocchio_keygen)."""
    return (ZK if zk else NonZK).generate(rng, circuit, form)


def keygen(rng, circuit: R1CS):
    """KeyGen.generate (pinocchio.ml:77-189): exponents on the host, points from the fixed-base kernel."""
    P = FR_MODULUS
    rv, rw, s, av, aw, ay, b, gm = (rng() % P for _ in range(8))
    ry = rv * rw % P
    vk_, wk_, yk_, t = _uks(circuit, s)
    mids = [k for k in range(circuit.m) if circuit.mid[k]]
    ios = [k for k in range(circuit.m) if not circuit.mid[k]]
    n = circuit.n
    si = [pow(s, i, P) for i in range(n + 1)]
    vt, wt, yt = rv * t % P, rw * t % P, ry * t % P
    e1 = ([rv * vk_[k] % P for k in mids] + [ry * yk_[k] % P for k in mids] + [rv * vk_[k] * av % P for k in mids]
          + [ry * yk_[k] * ay % P for k in mids] + [(rv * vk_[k] + rw * wk_[k] + ry * yk_[k]) * b % P for k in mids]
          + si + vk_ + wk_ + [vt, yt, vt * av % P, yt * ay % P, vt * b % P, wt * b % P, yt * b % P])
    e2 = [rw * wk_[k] % P for k in mids] + [rw * wk_[k] * aw % P for k in mids] + si + [wt, wt * aw % P]
    v1 = [1, aw, gm * b % P] + [rv * vk_[k] % P for k in ios] + [ry * yk_[k] % P for k in ios]
    v2 = [1, av, ay, gm, gm * b % P, yt] + [rw * wk_[k] % P for k in ios]
    return (PKey(G1.of_Fr(fr_bytes(e1)), G2.of_Fr(fr_bytes(e2))), VKey(G1.of_Fr(fr_bytes(v1)), G2.of_Fr(fr_bytes(v2))))


def _generate(cls, rng, circuit: R1CS, form="lagrange"):
    """KeyGen.generate and upload in ONE library call (zk_pinocchio_keygen): returns (prover, pkey, vkey).  Draws rv, rw, s, av, aw, ay, b, gm from
    `rng` in keygen's order, so the same rng gives the same key bytes.  pkey is the reference's evaluation key whatever `form` says;
    form = "lagrange" | "tau_powers" chooses the prover's h pool -- "lagrange": as after derive_lagrange(), without the derivation."""
    P = FR_MODULUS
    toxic = fr_bytes([rng() % P for _ in range(8)])
    n, m = circuit.n, circuit.m
    mid = np.ascontiguousarray(circuit.mid, dtype=np.uint8)
    n_mid = int(np.count_nonzero(mid))
    n_io = m - n_mid
    g1 = np.zeros(96 * (5 * n_mid + (n + 1) + 2 * m + 7), dtype=np.uint8)
    g2 = np.zeros(192 * (2 * n_mid + (n + 1) + 2), dtype=np.uint8)
    v1 = np.zeros(96 * (3 + 2 * n_io), dtype=np.uint8)
    v2 = np.zeros(192 * (6 + n_io), dtype=np.uint8)
    L, R, O = _csr(circuit.L), _csr(circuit.R), _csr(circuit.O)
    h = C.c_uint64()
    _lib.check(_lib.lib().zk_pinocchio_keygen(n, m, C.byref(L), C.byref(R), C.byref(O), _p(mid), _p(toxic), _lib.KEY_FORMS[form],
                                              _p(g1), len(g1) // 96, _p(g2), len(g2) // 192, _p(v1), _p(v2), C.byref(h)))
    self = cls.__new__(cls)
    self.circuit, self._keep, self.handle = circuit, (circuit,), h
    return self, PKey(g1, g2), VKey(v1, v2)


class _Prover:
    def __init__(self, circuit: R1CS, pkey: PKey, lagrange=None):
        """Uploads the evaluation key and the circuit once.  lagrange = the n points [lambda_t(s)] (n-1) | [Z(s)] (the first n points of pool 5 of a
        derived key, or of a keygen that knew s): the key then starts in its derived form (zk_pinocchio_pk_upload_lagrange) -- that the points belong
        to this key is the caller's promise."""
        self.circuit = circuit
        self._keep = (circuit, pkey)
        L, R, O = _csr(circuit.L), _csr(circuit.R), _csr(circuit.O)
        h = C.c_uint64()
        g1 = np.ascontiguousarray(pkey.g1, dtype=np.uint8)
        g2 = np.ascontiguousarray(pkey.g2, dtype=np.uint8)
        mid = np.ascontiguousarray(circuit.mid, dtype=np.uint8)
        if lagrange is not None:
            hl = np.ascontiguousarray(lagrange, dtype=np.uint8).reshape(-1)
            if len(hl) != 96 * circuit.n:
                raise ValueError("lagrange: n points [lambda_t(s)] (n-1) | [Z(s)] of 96 bytes each")
            _lib.check(_lib.lib().zk_pinocchio_pk_upload_lagrange(circuit.n, circuit.m, C.byref(L), C.byref(R), C.byref(O), _p(mid),
                                                                 _p(g1), len(g1) // 96, _p(g2), len(g2) // 192, _p(hl), C.byref(h)))
        else:
            _lib.check(_lib.lib().zk_pinocchio_pk_upload(C.c_uint32(circuit.n), C.c_uint32(circuit.m), C.byref(L), C.byref(R), C.byref(O),
                                                        _p(mid), _p(g1), C.c_size_t(len(g1) // 96), _p(g2), C.c_size_t(len(g2) // 192), C.byref(h)))
        self.handle = h

    generate = classmethod(_generate)

    @classmethod
    def from_lagrange(cls, circuit: R1CS, pkey: PKey, h_lagrange):
        """A prover whose key starts in its derived form: pkey plus the stored h bases (see `lagrange` above)."""
        return cls(circuit, pkey, lagrange=h_lagrange)

    @classmethod
    def from_compressed(cls, circuit: R1CS, g1_wire, g2_wire, h_lagrange=None):
        """A prover from the evaluation key's WIRE bytes (zk_pinocchio_pk_upload_compressed): the pools of zk_pinocchio_pk_upload with every point as the
        reference's JSON holds it, 48 / 96 bytes (wire.pinocchio_pkey_bytes_of_json); h_lagrange = the stored h bases of a derived key, n points of 48
        bytes (the first n of pool_points(5, compressed=True)).  Decoded and checked on the device; the identity is C0 00 .. 00 only.  A refused point
        raises the JSON readers' ValueError."""
        g1 = np.ascontiguousarray(np.frombuffer(bytes(g1_wire), dtype=np.uint8))
        g2 = np.ascontiguousarray(np.frombuffer(bytes(g2_wire), dtype=np.uint8))
        if len(g1) % 48 or len(g2) % 96:
            raise ValueError("from_compressed: G1 points are 48 bytes, G2 points 96")
        hl = None
        if h_lagrange is not None:
            hl = np.ascontiguousarray(np.frombuffer(bytes(h_lagrange), dtype=np.uint8))
            if len(hl) != 48 * circuit.n:
                raise ValueError("h_lagrange: n points [lambda_t(s)] (n-1) | [Z(s)] of 48 bytes each")
        mid = np.ascontiguousarray(circuit.mid, dtype=np.uint8)
        L, R, O = _csr(circuit.L), _csr(circuit.R), _csr(circuit.O)
        h = C.c_uint64()
        _lib.check_points(_lib.lib().zk_pinocchio_pk_upload_compressed(circuit.n, circuit.m, C.byref(L), C.byref(R), C.byref(O), _p(mid), _p(g1), len(g1) // 48,
                                                                       _p(g2), len(g2) // 96, None if hl is None else _p(hl), C.byref(h)))
        self = cls.__new__(cls)
        self.circuit, self._keep, self.handle = circuit, (circuit,), h
        return self

    def derive_lagrange(self):
        """zk_pinocchio_pk_derive_lagrange: the h pool rewritten for the values of h (bases derived from the key's own powers si on the
        device, once); afterwards every proof skips the basis conversion.  Proof bytes do not change.  Pool 5 becomes
        [lambda_t(s)] (n-1) | [Z(s)] | [1] | [s^(n-1)] (compact, the default) or [lambda_t(s)] | [Z(s)] | [1] | v_all | w_all."""
        _lib.check(_lib.lib().zk_pinocchio_pk_derive_lagrange(self.handle))

    def pool_points(self, pool, compressed=False):
        """A resident base pool as uncompressed bytes, in pool order: 0..5 the G1 products (5 = the h pool), 6..7 the G2 products; compressed=True: in
        wire form (48 / 96 B per point, encoded on the device)."""
        fn = _lib.lib().zk_pinocchio_pool_points_compressed if compressed else _lib.lib().zk_pinocchio_pool_points
        cnt = C.c_size_t()
        _lib.check(fn(self.handle, C.c_int(pool), None, C.c_size_t(0), C.byref(cnt)))
        out = np.zeros(cnt.value * (96 if pool < 6 else 192) // (2 if compressed else 1), dtype=np.uint8)
        _lib.check(fn(self.handle, C.c_int(pool), _p(out), C.c_size_t(cnt.value), C.byref(cnt)))
        return out

    def pool_size(self, pool):
        """Points in a resident pool.  Pool 5 tells the key's form: n + 1 + 2m = si | v_all | w_all as pinocchio.ml:481-486 reads them, n + 1 = the
        compact h pool (v_all | w_all passed the upload's consistency check and ride on si: csrc/pinocchio.hip), n + 2 = its derived form."""
        cnt = C.c_size_t()
        _lib.check(_lib.lib().zk_pinocchio_pool_points(self.handle, C.c_int(pool), None, C.c_size_t(0), C.byref(cnt)))
        return cnt.value

    def close(self):
        if getattr(self, "handle", None) is not None:
            _lib.lib().zk_pinocchio_pk_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prove_with(self, sol, dv, dw, dy):
        w = np.ascontiguousarray(sol, dtype=np.uint8).reshape(-1) if isinstance(sol, np.ndarray) else (
            np.frombuffer(bytes(sol), dtype=np.uint8) if isinstance(sol, (bytes, bytearray)) else fr_bytes(sol))
        if len(w) != 32 * self.circuit.m:
            raise AssertionError("Variable not found")          # var.ml:75-77
        out = np.zeros(960, dtype=np.uint8)
        d = [fr_bytes([x]) for x in (dv, dw, dy)]
        rc = _lib.lib().zk_pinocchio_prove(self.handle, _p(w), _p(d[0]), _p(d[1]), _p(d[2]), _p(out))
        if rc == ZK_ERR_REMAINDER:
            raise AssertionError("Polynomial.is_zero rem")      # QAP.ml:134
        _lib.check(rc)
        b = bytes(out)
        return Proof(b[:96], b[96:288], b[288:384], b[384:480], b[480:576], b[576:768], b[768:864], b[864:960])


    # ---- pipelined form (several proofs in flight on one key, witness resident in HBM)
    @staticmethod
    def _proof_of(out):
        b = bytes(out)
        return Proof(b[:96], b[96:288], b[288:384], b[384:480], b[480:576], b[576:768], b[768:864], b[864:960])

    def set_witness(self, sol):
        w = np.ascontiguousarray(sol, dtype=np.uint8).reshape(-1) if isinstance(sol, np.ndarray) else (
            np.frombuffer(bytes(sol), dtype=np.uint8) if isinstance(sol, (bytes, bytearray)) else fr_bytes(sol))
        if len(w) != 32 * self.circuit.m:
            raise AssertionError("Variable not found")          # var.ml:75-77
        _lib.check(_lib.lib().zk_pinocchio_set_witness(self.handle, _p(w)))

    def reserve_slots(self, count):
        _lib.check(_lib.lib().zk_pinocchio_reserve_slots(self.handle, C.c_uint32(count)))

    def _draw(self, rng):
        """the blinding scalars of one proof: ZK draws dv, dw, dy in this order (pinocchio.ml:428-430), NonZK takes zeros and draws nothing"""
        return (0, 0, 0)

    def prove_many(self, rng_or_rs, sols, in_flight=0, return_status=False):
        """A batch of proofs in ONE call, each as its 480 wire bytes, the eight points in declaration order (zk_pinocchio_prove_many_compressed): what
        wire.pinocchio_proof_json_of_bytes writes as the proof record and verify_many(..., compressed=True) of a resident key takes.  sols: the
        witnesses, or an int: that many proofs of the witness set_witness made resident.  rng_or_rs: a callable, drawn per proof in proof order as
        `prove` draws, or the (dv, dw, dy) triples.  in_flight: proofs kept in flight, 1..15 (0: the library's default).  The first failed proof
        raises what `prove` raises; with return_status (proofs, statuses) comes back and a failed proof's bytes are zeros."""
        to_bytes = lambda sol: np.ascontiguousarray(sol, dtype=np.uint8).reshape(-1) if isinstance(sol, np.ndarray) else (
            np.frombuffer(bytes(sol), dtype=np.uint8) if isinstance(sol, (bytes, bytearray)) else fr_bytes(sol))
        ws, count = _many_witnesses(to_bytes, sols, self.circuit.m)
        ds = [self._draw(rng_or_rs) for _ in range(count)] if callable(rng_or_rs) or rng_or_rs is None else [tuple(x) for x in rng_or_rs]
        if len(ds) != count or any(len(x) != 3 for x in ds):
            raise ValueError("prove_many: need one (dv, dw, dy) triple per proof")
        rnd = fr_bytes([x for t in ds for x in t])
        return _prove_many(_lib.lib().zk_pinocchio_prove_many_compressed, self.handle, ws, rnd, count, in_flight, 480, return_status)

    def prove_async(self, dv, dw, dy, slot):
        d = [fr_bytes([x]) for x in (dv, dw, dy)]
        _lib.check(_lib.lib().zk_pinocchio_prove_async(self.handle, None, _p(d[0]), _p(d[1]), _p(d[2]), C.c_uint32(slot)))

    def prove_wait(self, slot):
        out = np.zeros(960, dtype=np.uint8)
        rc = _lib.lib().zk_pinocchio_prove_wait(self.handle, C.c_uint32(slot), _p(out))
        if rc == ZK_ERR_REMAINDER:
            raise AssertionError("Polynomial.is_zero rem")      # QAP.ml:134
        _lib.check(rc)
        return self._proof_of(out)


def verify(input_output, vkey: VKey, proof: Proof):
    """Verify.f (pinocchio.ml:254-420): the four knowledge-of-coefficient checks and the divisibility check,
    13 pairings on the host (verify_many checks a batch on the device).  input_output: the public coefficients c_k in the key's variable order."""
    io = input_output if isinstance(input_output, (bytes, bytearray, np.ndarray)) else fr_bytes(list(input_output))
    io = np.ascontiguousarray(np.frombuffer(bytes(io), dtype=np.uint8))
    n_io = len(io) // 32
    g1 = np.ascontiguousarray(vkey.g1, dtype=np.uint8).reshape(-1)
    g2 = np.ascontiguousarray(vkey.g2, dtype=np.uint8).reshape(-1)
    if len(g1) != 96 * (3 + 2 * n_io) or len(g2) != 192 * (6 + n_io):
        raise AssertionError("Variable not found")          # domains of the key maps and of the public inputs must agree
    ok = C.c_int(0)
    _lib.check(_lib.lib().zk_pinocchio_verify(_p(g1), _p(g2), _p(io) if n_io else None, C.c_size_t(n_io), proof.to_bytes(), C.byref(ok)))
    return bool(ok.value)


def verify_many(input_outputs, vkey: VKey, proofs, return_status=False):
    """`verify` for many proofs under one key in ONE call, on the DEVICE (zk_pinocchio_verify_many, csrc/pairing_dev.hip; no host fallback).
    input_outputs[i]: the public coefficients of proofs[i].  Returns a list of bool; with return_status also the list of codes the single-proof
    call would return for each proof.  A defective proof is False, it does not raise; a defective KEY raises, as in `verify`."""
    proofs = list(proofs)
    input_outputs = list(input_outputs)
    if len(input_outputs) != len(proofs):
        raise ValueError("verify_many: need one list of public inputs per proof")
    g1 = np.ascontiguousarray(vkey.g1, dtype=np.uint8).reshape(-1)
    g2 = np.ascontiguousarray(vkey.g2, dtype=np.uint8).reshape(-1)
    n_io = len(g2) // 192 - 6
    if n_io < 0 or len(g1) != 96 * (3 + 2 * n_io) or len(g2) != 192 * (6 + n_io):
        raise AssertionError("Variable not found")
    ios = []
    for io in input_outputs:
        io = bytes(io if isinstance(io, (bytes, bytearray, np.ndarray)) else fr_bytes(list(io)))
        if len(io) != 32 * n_io:
            raise AssertionError("Variable not found")          # domains of the key maps and of the public inputs must agree
        ios.append(io)
    count = len(proofs)
    ok = np.zeros(max(count, 1), dtype=np.uint8)
    status = np.zeros(max(count, 1), dtype=np.int32)
    io_all = np.frombuffer(b"".join(ios), dtype=np.uint8)
    pr_all = np.frombuffer(b"".join(bytes(p.to_bytes()) for p in proofs), dtype=np.uint8)
    if len(pr_all) != 960 * count:
        raise ValueError("verify_many: a proof is not 960 bytes")
    _lib.check(_lib.lib().zk_pinocchio_verify_many(_p(g1), _p(g2), C.c_size_t(n_io), _p(io_all) if n_io and count else None, _p(pr_all) if count else None,
                                                   C.c_uint32(count), _p(ok), status.ctypes.data_as(C.POINTER(C.c_int32))))
    res = [bool(x) for x in ok[:count]]
    return (res, [int(x) for x in status[:count]]) if return_status else res


class ZK(_Prover):
    keygen = staticmethod(keygen)
    verify = staticmethod(verify)
    verify_many = staticmethod(verify_many)

    def _draw(self, rng):
        dv = rng() % FR_MODULUS     # pinocchio.ml:428-430: dv, dw, dy in this order
        dw = rng() % FR_MODULUS
        dy = rng() % FR_MODULUS
        return dv, dw, dy

    def prove(self, rng, sol):
        return self.prove_with(sol, *self._draw(rng))


class NonZK(_Prover):
    keygen = staticmethod(keygen)
    verify = staticmethod(verify)
    verify_many = staticmethod(verify_many)

    def prove(self, _rng, sol):
        return self.prove_with(sol, 0, 0, 0)
