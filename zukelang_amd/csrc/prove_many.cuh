// zk_groth16_prove_many_compressed / zk_pinocchio_prove_many_compressed (include/zkmi355x.h): the loop over a batch of proofs that both protocols share.
// The reference proves one witness per call (groth16.ml:123-161,235-237; pinocchio.ml:427-514) and writes the proof as a record of compressed points
// (groth16.ml:110-114, pinocchio.ml:195-208).  Here proof i runs in its raw form on slot i mod in_flight of the key -- the slot's products leave XYZZ sums
// on the device -- and its sums are copied, on the slot's own stream, into row i of a slab; when the last slot has finished, ONE launch per group
// (k_proofs_to_wire, msm_points.hip) turns the whole slab into wire records and ONE copy brings them to the host.  Per proof the host waits for one event
// and nothing else: no conversion launch, no copy to the host.
//
// The protocol describes itself in a struct P:
//   ROW_BYTES, WIRE_BYTES            a proof's row of XYZZ sums (G1 sums, then G2 sums) and its wire record
//   wire1(), wire2()                 where the G1 / G2 points of a row go in the record (ProofWire, msm.cuh)
//   enqueue(i, slot, d_row)          proof i on `slot` in raw form, then its sums into d_row on the slot's stream; the slot is busy afterwards
//   finish(slot)                     waits for the slot, frees it, returns the proof's status (what the single call returns)
#pragma once
#include "msm.cuh"

#include <string.h>

namespace zk {

static constexpr uint32_t PROVE_MANY_SLAB = 8192;               // proofs per slab, as the batched verifiers cut theirs
static constexpr uint32_t PROVE_MANY_MAX = 1u << 24;
static constexpr uint32_t PROVE_MANY_MAX_IN_FLIGHT = 15;        // the slots of a key
static constexpr uint32_t PROVE_MANY_IN_FLIGHT = 14;            // in_flight = 0: what the headline rate is measured with (bench.py --inflight)

// a proof's own failure is its status; anything else ends the batch
static inline bool prove_status_is_per_proof(int rc) { return rc == ZK_OK || rc == ZK_ERR_REMAINDER || rc == ZK_ERR_SCALAR_RANGE; }

// the slots a batch uses: the caller's number, or the library's default; never more than there are proofs
static inline uint32_t prove_many_in_flight(uint32_t in_flight, uint32_t count) {
    if (in_flight == 0) in_flight = PROVE_MANY_IN_FLIGHT;
    return in_flight > count ? count : in_flight;
}
// what both calls refuse before anything else (the handle's own checks follow in the caller)
static inline int prove_many_check_args(const void* rnd, const void* proofs, const void* status, uint32_t count, uint32_t in_flight, const char* who) {
    if (!rnd || !proofs || !status) return set_error(ZK_ERR_ARG, who, __FILE__, __LINE__);
    if (in_flight > PROVE_MANY_MAX_IN_FLIGHT) ZK_FAIL(ZK_ERR_ARG, "prove_many_compressed: at most 15 proofs in flight");
    if (count > PROVE_MANY_MAX) ZK_FAIL(ZK_ERR_ARG, "prove_many_compressed: more than 2^24 proofs in one call");
    return ZK_OK;
}

template <class P> int prove_many_run(P& p, uint32_t count, uint32_t in_flight, uint8_t* proofs, int32_t* status, hipStream_t s) {
    in_flight = prove_many_in_flight(in_flight, count);
    const uint32_t slab = count < PROVE_MANY_SLAB ? count : PROVE_MANY_SLAB;
    DevBuf rows, wire;
    ZKCHK(rows.alloc((size_t)P::ROW_BYTES * slab));
    ZKCHK(wire.alloc((size_t)P::WIRE_BYTES * slab));
    for (uint32_t base = 0; base < count; base += slab) {
        const uint32_t cnt = count - base < slab ? count - base : slab;
        int64_t pending[PROVE_MANY_MAX_IN_FLIGHT];          // the proof a slot is working on
        for (uint32_t t = 0; t < in_flight; t++) pending[t] = -1;
        int rc = ZK_OK;
        auto collect = [&](uint32_t t) {
            const int st = p.finish(t);
            status[pending[t]] = st;
            pending[t] = -1;
            if (rc == ZK_OK && !prove_status_is_per_proof(st)) rc = st;
        };
        for (uint32_t j = 0; j < cnt && rc == ZK_OK; j++) {
            const uint32_t t = j % in_flight;
            if (pending[t] >= 0) collect(t);               // the status of proof j - in_flight
            if (rc != ZK_OK) break;
            rc = p.enqueue(base + j, t, rows.as<char>() + (size_t)P::ROW_BYTES * j);
            if (rc == ZK_OK) pending[t] = base + j;
        }
        // in the order the proofs were enqueued; after a failure this drains what is still in flight
        for (uint32_t j = 0; j < in_flight; j++) {
            const uint32_t t = (cnt + j) % in_flight;
            if (pending[t] >= 0) collect(t);
        }
        if (rc != ZK_OK) return rc;
        // every row has landed (each slot's event stands behind its row copy): one conversion per group, one copy
        ZKCHK(proofs_to_wire_dev(CURVE_G1, rows.p, cnt, p.wire1(), wire.p, s));
        ZKCHK(proofs_to_wire_dev(CURVE_G2, rows.p, cnt, p.wire2(), wire.p, s));
        uint8_t* out = proofs + (size_t)P::WIRE_BYTES * base;
        HIPCHK(hipMemcpyAsync(out, wire.p, (size_t)P::WIRE_BYTES * cnt, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (uint32_t j = 0; j < cnt; j++)
            if (status[base + j] != ZK_OK) memset(out + (size_t)P::WIRE_BYTES * j, 0, P::WIRE_BYTES);          // no flag bits: no verifier takes it for a proof
    }
    return ZK_OK;
}

}  // namespace zk
