// Multi-device keys: N GPUs of one node behind ONE handle of ONE process -- the part Groth16 (groth16_multi.hip) and Pinocchio (pinocchio.hip) share.
//
// With a device list of N entries (zk_set_devices / zk_set_device_list) an upload builds one SHARD of the key per entry -- contiguous slices of every
// base pool, each with its own window tables, slots and streams on its device -- and returns one handle.  A proof on slot t then runs
//   * the Fr stage and the scalar vectors over the FULL pools ONCE, on the slot's owner device (t mod N: proofs in flight rotate over the devices);
//   * on every device: a device-to-device copy of ITS slices of the vectors out of the owner's memory (hipMemcpyPeerAsync over xGMI; a plain device
//     copy where two shards share a card), enqueued on the device's own slot stream behind an event of the owner's stream, then the multi-scalar
//     products over the slices and a copy of the raw XYZZ partial sums (one block of P::G1 + P::G2 points) to the list's first device;
//   * on the first device: the sum of the N blocks per product (EC addition: exact, so the bytes do not depend on N or on the cuts), the affine
//     conversion and the copy of the proof to pinned host memory.
// Everything is enqueued by the calling thread and nothing synchronises before prove_wait: the per-device streams are chained by events only, so up
// to 15 proofs stay in flight exactly as on one GPU.  No collective library is involved -- the exchange is N - 1 peer copies per vector, the pattern
// xGMI's point-to-point links serve directly.
//
// The protocol describes itself in a traits struct P:
//   Key, Slot                         a shard and its per-proof slot (Key has slots[], wit_resident, m, have_witness)
//   MAX_SLOTS, G1, G2, PROOF_BYTES    slot limit, products per group in a partial block (G1 first), bytes of a proof
//   OFF1[G1], OFF2[G2]                where each product lands in the proof (proof_points_to_bytes_dev)
//   slot_get(Key&, idx, Slot**)       the shard's slot, built on demand on the current device
//   stream(Slot&), results(Slot&)     the slot's one stream; its block of raw partial sums
//   flags(Slot&)                      the pinned word the Fr stage's flags land in (frstage.cuh: status_of_flags)
//   BROKEN, SLOT_RANGE, SLOT_BUSY, WAIT_NEVER_USED, SET_WITNESS_BUSY     the message texts that differ
// and hands prove_async the two halves of a proof as callables (template parameters: no indirect call on the path that enqueues a proof).
#pragma once
#include "frstage.cuh"
#include "msm.cuh"

#include <memory>
#include <string.h>
#include <vector>

namespace zk {

template <class P> struct DeviceGroup {
    using Key = typename P::Key;
    using Slot = typename P::Slot;
    static constexpr size_t G1_BYTES = P::G1 * 192, G2_BYTES = P::G2 * 384, PARTIAL_BYTES = G1_BYTES + G2_BYTES;          // raw XYZZ: msm.cuh, xyzz_bytes

    struct GroupSlot {
        DevBuf parts, g1p, g2p, sum, out;          // on the list's first device: [device][PARTIAL_BYTES] landing area of the partial sums, the combine's scratch
        uint8_t* host = nullptr;                   // pinned: the proof
        hipEvent_t ev_scal = nullptr;              // the owner's scalar vectors are complete
        std::vector<hipEvent_t> ev_part;           // per device: its block has landed on the first device
        hipEvent_t done = nullptr;
        bool busy = false;
        int owner = 0;
        ~GroupSlot() {
            if (ev_scal) (void)hipEventDestroy(ev_scal);
            for (hipEvent_t e : ev_part)
                if (e) (void)hipEventDestroy(e);
            if (done) (void)hipEventDestroy(done);
            if (host) (void)hipHostFree(host);
        }
    };

    bool broken = false;                               // a derivation failed between the shards' installs
    std::vector<std::unique_ptr<Key>> sub;             // sub[v]: the shard on virtual device v (rank v of world N)
    std::unique_ptr<GroupSlot> slots[P::MAX_SLOTS];

    // slots first (events, pinned memory, buffers of the first device), then the shards, each with its own device current
    void destroy() {
        drop_slots();
        for (size_t v = 0; v < sub.size(); v++) {
            DeviceScope ds((int)v);
            sub[v].reset();
        }
    }
    void drop_slots() {
        DeviceScope ds(0);
        for (auto& sl : slots) sl.reset();
    }
    int sync_all() {
        for (size_t v = 0; v < sub.size(); v++) {
            DeviceScope ds((int)v);
            HIPCHK(hipDeviceSynchronize());
        }
        return ZK_OK;
    }
    int check_idle(const char* who) {
        if (broken) ZK_FAIL(ZK_ERR_HIP, P::BROKEN);
        for (auto& sl : slots)
            if (sl && sl->busy) ZK_FAIL(ZK_ERR_ARG, who);
        return ZK_OK;
    }
    int slot_get(uint32_t idx, GroupSlot** out) {
        if (idx >= P::MAX_SLOTS) ZK_FAIL(ZK_ERR_ARG, P::SLOT_RANGE);
        const size_t N = sub.size();
        if (!slots[idx]) {
            for (size_t v = 0; v < N; v++) {          // the slot's share on every device: Fr scratch, scalar vectors, workspaces, one stream
                DeviceScope ds((int)v);
                Slot* sl;
                ZKCHK(P::slot_get(*sub[v], idx, &sl));
            }
            DeviceScope ds(0);
            auto gs = std::make_unique<GroupSlot>();
            ZKCHK(gs->parts.alloc(PARTIAL_BYTES * N));
            ZKCHK(gs->g1p.alloc(G1_BYTES * N));
            ZKCHK(gs->g2p.alloc(G2_BYTES * N));
            ZKCHK(gs->sum.alloc(PARTIAL_BYTES));
            ZKCHK(gs->out.alloc(P::PROOF_BYTES));
            HIPCHK(hipHostMalloc((void**)&gs->host, P::PROOF_BYTES, hipHostMallocDefault));
            HIPCHK(hipEventCreateWithFlags(&gs->done, hipEventDisableTiming));
            gs->ev_part.assign(N, nullptr);
            // the owner records ev_scal, device v records ev_part[v]: events live on the device whose stream records them
            gs->owner = (int)(idx % N);
            {
                DeviceScope dso(gs->owner);
                HIPCHK(hipEventCreateWithFlags(&gs->ev_scal, hipEventDisableTiming));
            }
            for (size_t v = 0; v < N; v++) {
                DeviceScope dsv((int)v);
                HIPCHK(hipEventCreateWithFlags(&gs->ev_part[v], hipEventDisableTiming));
            }
            slots[idx] = std::move(gs);
        }
        *out = slots[idx].get();
        return ZK_OK;
    }
    int reserve_slots(uint32_t count) {
        for (uint32_t i = 0; i < count; i++) {
            GroupSlot* gs;
            ZKCHK(slot_get(i, &gs));
        }
        return ZK_OK;
    }
    int set_witness(const uint8_t* sol) {
        ZKCHK(check_idle(P::SET_WITNESS_BUSY));
        for (size_t v = 0; v < sub.size(); v++) {          // any device may own a proof's Fr stage
            DeviceScope ds((int)v);
            Key& k = *sub[v];
            HIPCHK(hipMemcpyAsync(k.wit_resident.p, sol, 32 * (size_t)k.m, hipMemcpyHostToDevice, ctx().stream));
            HIPCHK(hipStreamSynchronize(ctx().stream));
            k.have_witness = true;
        }
        return ZK_OK;
    }

    // scalars(Key& owner_shard, Slot& owner_slot): enqueues the Fr stage and the scalar vectors over the FULL pools on the owner's slot stream.
    // products(int v, Key& shard, Slot& sv, int owner, Slot& owner_slot), with device v current: where v != owner, copies this shard's slices of the
    // vectors out of the owner's slot (copy_between on sv's stream, which already waits for the owner's vectors); then enqueues the shard's products,
    // raw XYZZ partial sums in P::results(sv).
    template <class Scalars, class Products> int prove_async(uint32_t slot, Scalars scalars, Products products) {
        if (broken) ZK_FAIL(ZK_ERR_HIP, P::BROKEN);
        GroupSlot* gsp;
        ZKCHK(slot_get(slot, &gsp));
        GroupSlot& gs = *gsp;
        if (gs.busy) ZK_FAIL(ZK_ERR_ARG, P::SLOT_BUSY);
        const int N = (int)sub.size(), owner = gs.owner;
        Slot& so = *sub[owner]->slots[slot];
        {   // ---- Fr stage on the owner: the scalar vectors over the FULL pools, in the owner's slot buffers
            DeviceScope ds(owner);
            ZKCHK(scalars(*sub[owner], so));
            HIPCHK(hipEventRecord(gs.ev_scal, P::stream(so)));
        }
        // from here on the slot is in flight whatever happens: a failed enqueue below leaves work on some streams, and _wait drains it
        gs.busy = true;
        int rc = ZK_OK;
        for (int v = 0; v < N && rc == ZK_OK; v++) {
            DeviceScope ds(v);
            Key& k = *sub[v];
            Slot& sv = *k.slots[slot];
            auto body = [&]() -> int {
                // this device's slices out of the owner's memory travel on this device's stream, behind the owner's Fr stage
                if (v != owner) HIPCHK(hipStreamWaitEvent(P::stream(sv), gs.ev_scal, 0));
                ZKCHK(products(v, k, sv, owner, so));
                ZKCHK(copy_between(gs.parts.template as<char>() + PARTIAL_BYTES * v, 0, P::results(sv), v, PARTIAL_BYTES, P::stream(sv)));
                HIPCHK(hipEventRecord(gs.ev_part[v], P::stream(sv)));
                return ZK_OK;
            };
            rc = body();
        }
        {   // ---- first device: add the N blocks per product, convert, land the proof in pinned memory.  On ONE stream for all slots (the context's second
            // stream): the Fp2 column sum carries 3 KiB of private memory per lane, i.e. 1.6 GiB of scratch for every QUEUE it is dispatched on -- on the
            // slots' own streams a handful of proofs in flight exhausted the device's scratch aperture (HSA_STATUS_ERROR_OUT_OF_RESOURCES, the runtime aborts
            // the process).  A combine is ~50 us of work behind its N events; the slots' combines queue up in the order the proofs were enqueued.
            DeviceScope ds(0);
            hipStream_t cs = ctx().stream2;
            auto body = [&]() -> int {
                for (int v = 0; v < N; v++) HIPCHK(hipStreamWaitEvent(cs, gs.ev_part[v], 0));
                if (rc != ZK_OK) return rc;
                char* sum = gs.sum.template as<char>();
                HIPCHK(hipMemcpy2DAsync(gs.g1p.p, G1_BYTES, gs.parts.p, PARTIAL_BYTES, G1_BYTES, N, hipMemcpyDeviceToDevice, cs));                                      // [device][G1 sums]
                HIPCHK(hipMemcpy2DAsync(gs.g2p.p, G2_BYTES, gs.parts.template as<char>() + G1_BYTES, PARTIAL_BYTES, G2_BYTES, N, hipMemcpyDeviceToDevice, cs));         // [device][G2 sums]
                ZKCHK(xyzz_sum_columns(CURVE_G1, sum, gs.g1p.p, N, P::G1, cs));
                ZKCHK(xyzz_sum_columns(CURVE_G2, sum + G1_BYTES, gs.g2p.p, N, P::G2, cs));
                ZKCHK(proof_points_to_bytes_dev(sum, P::G1, P::OFF1, sum + G1_BYTES, P::G2, P::OFF2, gs.out.p, cs));
                HIPCHK(hipMemcpyAsync(gs.host, gs.out.p, P::PROOF_BYTES, hipMemcpyDeviceToHost, cs));
                return ZK_OK;
            };
            const int rc0 = body();
            if (rc == ZK_OK) rc = rc0;
            (void)hipEventRecord(gs.done, cs);
        }
        if (rc != ZK_OK) {          // nothing of a half-enqueued proof may stay in flight behind the caller's back
            (void)sync_all();
            gs.busy = false;
        }
        return rc;
    }
    // the sums of the proof that last finished on `slot`, P::G1 then P::G2 raw XYZZ points on the list's first device: what proof_points_to_bytes_dev read
    const void* sums(uint32_t slot) const { return slots[slot]->sum.p; }
    int prove_wait(uint32_t slot, uint8_t* proof) {
        if (slot >= P::MAX_SLOTS || !slots[slot]) ZK_FAIL(ZK_ERR_ARG, P::WAIT_NEVER_USED);
        GroupSlot& gs = *slots[slot];
        if (!gs.busy) ZK_FAIL(ZK_ERR_ARG, "no proof in flight on this slot");
        {
            DeviceScope ds(0);
            HIPCHK(hipEventSynchronize(gs.done));          // behind every device's block, which is behind the owner's Fr stage and its flag copy
        }
        gs.busy = false;
        ZKCHK(status_of_flags(P::flags(*sub[gs.owner]->slots[slot])));
        memcpy(proof, gs.host, P::PROOF_BYTES);
        return ZK_OK;
    }
};

}  // namespace zk
