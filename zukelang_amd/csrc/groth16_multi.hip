// Multi-device Groth16 keys: N GPUs of one node behind ONE handle of ONE process (what an OCaml host reaches through the ctypes
// shim -- `Groth16.Make(C).prove`, src/groth16/groth16.ml:235-237, is one call on one key and knows nothing of ranks).
//
// With a device list of N entries (zk_set_devices / zk_set_device_list), zk_groth16_pk_upload builds one SHARD of the key per entry -- the contiguous
// slices of both base pools that zk_groth16_shard_range cuts for equal work -- and returns one handle.  How a proof then runs over the devices --
// the Fr stage (QAP.eval, QAP.ml:120-135) once on the slot's owner, the three products (groth16.ml:116-161) over every device's slices, the sum of the
// 768-byte blocks on the first device -- is device_group.cuh, shared with Pinocchio; this file holds what is Groth16's own: the upload, the two
// callables of a proof, the pools' read-back and the derivation.  The one-process-per-GPU path (torch.distributed / RCCL: bench.py --gpus N) is unchanged.
// The derivation of the key's Lagrange form (zk_groth16_pk_derive_lagrange) gathers the tau-power pools on up to three devices, derives one of
// the three independent sets on each (one host thread per device), copies every set to every device and installs the shards.
#include "device_group.cuh"
#include "groth16_key.cuh"
#include "handle_table.h"
#include "prove_many.cuh"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <functional>
#include <thread>
#include <vector>

namespace zk {

struct Groth16GroupTraits {
    using Key = Groth16Key;
    using Slot = zk::Slot;
    static constexpr uint32_t MAX_SLOTS = zk::MAX_SLOTS, G1 = 2, G2 = 1, PROOF_BYTES = 384;
    static constexpr uint32_t OFF1[G1] = {0, 288}, OFF2[G2] = {96};          // sums: A | C | B;  proof: a | b | c
    static int slot_get(Key& k, uint32_t idx, Slot** out) { return groth16_slot_get(k, idx, out); }
    static hipStream_t stream(Slot& sl) { return sl.s0; }
    static void* results(Slot& sl) { return sl.results.p; }
    static const uint8_t* flags(Slot& sl) { return sl.host + 384; }
    static constexpr const char* BROKEN = "multi-device key is inconsistent after a failed derivation: free it";
    static constexpr const char* SLOT_RANGE = "slot index out of range (max 15 proofs in flight)";
    static constexpr const char* SLOT_BUSY = "slot still has a proof in flight: call the matching _wait first";
    static constexpr const char* WAIT_NEVER_USED = "zk_groth16_prove_wait: slot never used";
    static constexpr const char* SET_WITNESS_BUSY = "zk_groth16_set_witness: a proof is in flight on this key";
};
struct GroupKey : DeviceGroup<Groth16GroupTraits> {
    uint32_t n = 0, m = 0, n_mid = 0;
    uint64_t p1 = 0, p2 = 0;                   // the whole pools
    bool lagrange = false;
};
static_assert(GroupKey::PARTIAL_BYTES == ZK_GROTH16_PARTIAL_BYTES, "partial block = A | C | B raw XYZZ");

static HandleTable<GroupKey>& g_groups = *new HandleTable<GroupKey>(HANDLES_GROTH16_GROUP, "unknown Groth16 key handle");

GroupKey* group_lookup(uint64_t handle) { return g_groups.find(handle); }
void group_release_all() {
    g_groups.release_all([](GroupKey& g) { g.destroy(); });
}

// runs f(v) for every virtual device of the key, one host thread each (the set-up paths synchronise their streams internally); the worst code wins
template <class F> static int on_every_device(size_t count, F f) {
    std::vector<int> rc(count, ZK_OK);
    // One host thread per PHYSICAL device; list entries that share a card ("virtual devices") take their turns on that card's thread.  Besides being
    // all the parallelism one card has to give, this bounds what the set-up kernels ask of the card at once: k_subgroup_check and the window-table
    // builders carry 1-2 KiB of private memory per lane, i.e. > 1 GiB of scratch per QUEUE they run on, and a handful of them on different queues of ONE
    // device exhaust its scratch aperture (HSA_STATUS_ERROR_OUT_OF_RESOURCES: the runtime aborts the process).
    std::vector<std::vector<int>> groups;
    for (size_t v = 0; v < count; v++) {
        size_t gi = 0;
        while (gi < groups.size() && ctx_at(groups[gi][0]).device != ctx_at((int)v).device) gi++;
        if (gi == groups.size()) groups.emplace_back();
        groups[gi].push_back((int)v);
    }
    // f allocates (std::vector, make_unique, device buffers): an exception that left a thread function would be std::terminate for the host process --
    // it becomes a return code like every other failure
    auto run_group = [&rc, &f](const std::vector<int>& vs) {
        for (int v : vs) {
            DeviceScope ds(v);
            try {
                rc[v] = f(v);
            } catch (const std::bad_alloc&) {
                rc[v] = set_error(ZK_ERR_HIP, "out of host memory while setting a device of the key up", __FILE__, __LINE__);
            } catch (const std::exception& e) {
                rc[v] = set_error(ZK_ERR_HIP, e.what(), __FILE__, __LINE__);
            } catch (...) {
                rc[v] = set_error(ZK_ERR_HIP, "exception while setting a device of the key up", __FILE__, __LINE__);
            }
        }
    };
    // A host thread that cannot be started (the process is at its thread limit) must not take the process down: std::thread's constructor throws,
    // and a joinable thread destroyed during the unwinding would call std::terminate.  Whatever could not be started runs on the calling thread.
    std::vector<std::thread> th;
    size_t started = 1;          // group 0 runs on the calling thread
    for (size_t gi = 1; gi < groups.size(); gi++) {
        try {
            th.emplace_back(run_group, std::cref(groups[gi]));
            started = gi + 1;
        } catch (...) {
            break;
        }
    }
    run_group(groups[0]);
    for (size_t gi = started; gi < groups.size(); gi++) run_group(groups[gi]);
    for (auto& t : th) t.join();
    int worst = ZK_OK;
    for (int r : rc)
        if (r < worst) worst = r;
    return worst;
}

static void trace(const char* what) {
    if (trace_on()) {          // diagnostics: environment only
        fprintf(stderr, "[zk multi] %s\n", what);
        fflush(stderr);
    }
}
int group_upload(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t* pk_g1, size_t pk_g1_points,
                 const uint8_t* pk_g2, size_t pk_g2_points, bool lagrange, uint64_t* handle, bool wire) {
    if (!handle || !mid || !pk_g1 || !pk_g2 || !L || !R || !O) ZK_FAIL(ZK_ERR_ARG, "pk_upload: null argument");
    const size_t N = (size_t)ctx_count();
    auto key = std::make_unique<GroupKey>();
    GroupKey& g = *key;
    g.sub.resize(N);
    // every shard checks its own slice of the key points and builds the Fr-stage tables (any device may own a proof's Fr stage)
    const int rc = on_every_device(N, [&](int v) {
        return groth16_key_build(g.sub[v], n, m, L, R, O, mid, pk_g1, pk_g1_points, pk_g2, pk_g2_points, (uint32_t)v, (uint32_t)N, lagrange, true, nullptr, nullptr, wire);
    });
    if (rc != ZK_OK) {
        g.destroy();
        return rc;
    }
    g.n = n; g.m = m; g.n_mid = g.sub[0]->n_mid; g.p1 = g.sub[0]->p1; g.p2 = g.sub[0]->p2; g.lagrange = lagrange;
    *handle = g_groups.add(std::move(key));
    return ZK_OK;
}
int group_free(uint64_t handle) {
    std::unique_ptr<GroupKey> g = g_groups.take(handle);
    if (!g) ZK_FAIL(ZK_ERR_HANDLE, g_groups.unknown());
    (void)g->sync_all();
    g->destroy();
    return ZK_OK;
}

int group_reserve_slots(GroupKey& g, uint32_t count) {
    if (count > MAX_SLOTS) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_reserve_slots: at most 15 slots");
    if (g.broken) ZK_FAIL(ZK_ERR_HIP, Groth16GroupTraits::BROKEN);
    return g.reserve_slots(count);
}
int group_set_witness(GroupKey& g, const uint8_t* sol) {
    if (!sol) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_set_witness: null");
    return g.set_witness(sol);
}
int group_prove_async(GroupKey& g, const uint8_t* sol, const uint8_t* r, const uint8_t* s, uint32_t slot) {
    return g.prove_async(
        slot,
        [&](Groth16Key& ko, Slot& so) { return groth16_scalars_enqueue(ko, so, sol, r, s, so.scalA.p, so.scalC.p, so.scalB.p); },
        [](int v, Groth16Key& k, Slot& sv, int owner, Slot& so) -> int {
            char *a = sv.scalA.as<char>() + 32 * k.lo1, *c = sv.scalC.as<char>() + 32 * k.lo1, *b = sv.scalB.as<char>() + 32 * k.lo2;
            if (v != owner) {
                // The A vector is zero beyond a | d1 | b1 | the tau basis (groth16.ml:128-134 touches no other key point): only that part of the
                // slice travels, the rest is cleared in place
                const uint64_t nzA = k.p2 + 1, a_hi = k.hi1 < nzA ? k.hi1 : (k.lo1 > nzA ? k.lo1 : nzA);
                ZKCHK(copy_between(a, v, so.scalA.as<char>() + 32 * k.lo1, owner, 32 * (a_hi - k.lo1), sv.s0));
                if (k.hi1 > a_hi) HIPCHK(hipMemsetAsync(a + 32 * (a_hi - k.lo1), 0, 32 * (k.hi1 - a_hi), sv.s0));
                ZKCHK(copy_between(c, v, so.scalC.as<char>() + 32 * k.lo1, owner, 32 * (k.hi1 - k.lo1), sv.s0));
                ZKCHK(copy_between(b, v, so.scalB.as<char>() + 32 * k.lo2, owner, 32 * (k.hi2 - k.lo2), sv.s0));
            }
            return groth16_msms_enqueue(k, sv, a, c, b, true, 1);          // raw XYZZ partial sums A | C | B in sv.results, one stream
        });
}
int group_prove_wait(GroupKey& g, uint32_t slot, uint8_t proof[384]) { return g.prove_wait(slot, proof); }
// zk_groth16_prove_many_compressed on a multi-device key (prove_many.cuh with one proof in flight): each proof runs the per-proof path above on slot 0
// to its end; the sums the first device added up for it are the proof's row, and the batch's conversion and copy are those of the one-device key.
struct GroupMany {
    static constexpr uint32_t ROW_BYTES = ZK_GROTH16_PARTIAL_BYTES, WIRE_BYTES = 192;
    GroupKey& g;
    const uint8_t *sols, *rs;
    int last = ZK_OK;
    static ProofWire wire1() { return groth16_wire_g1(); }
    static ProofWire wire2() { return groth16_wire_g2(); }
    int enqueue(uint32_t i, uint32_t, void* d_row) {
        uint8_t proof[384];
        ZKCHK(group_prove_async(g, sols ? sols + 32 * (size_t)g.m * i : nullptr, rs + 64 * (size_t)i, rs + 64 * (size_t)i + 32, 0));
        last = g.prove_wait(0, proof);
        if (!prove_status_is_per_proof(last)) return last;
        DeviceScope ds(0);
        hipStream_t cs = ctx().stream2;          // the stream the sums were written on
        HIPCHK(hipMemcpyAsync(d_row, g.sums(0), ROW_BYTES, hipMemcpyDeviceToDevice, cs));
        HIPCHK(hipStreamSynchronize(cs));
        return ZK_OK;
    }
    int finish(uint32_t) { return last; }
};
int group_prove_many(GroupKey& g, const uint8_t* sols, const uint8_t* rs, uint32_t count, uint8_t* proofs, int32_t* status) {
    if (!sols && !g.sub[0]->have_witness) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_prove_many_compressed: no witness: pass sols or call zk_groth16_set_witness first");
    ZKCHK(g.check_idle("zk_groth16_prove_many_compressed: a proof is in flight on this key: call the matching _wait first"));
    GroupMany many{g, sols, rs};
    DeviceScope ds(0);
    return prove_many_run(many, count, 1, proofs, status, ctx().stream2);
}

int group_lagrange_pool_sizes(GroupKey& g, uint64_t* g1_points, uint64_t* g2_points) {
    if (g1_points) *g1_points = 3 + (uint64_t)g.n + (g.n - 1) + g.n_mid;
    if (g2_points) *g2_points = 2 + (uint64_t)g.n;
    return ZK_OK;
}
int group_pool_layout(GroupKey& g, uint64_t* p1, uint64_t* p2) {
    *p1 = g.p1;
    *p2 = g.p2;
    return ZK_OK;
}
int group_pool_points(GroupKey& g, int group, uint8_t* out, size_t capacity_points, size_t* count, bool wire) {
    if (group != 1 && group != 2) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_pool_points: group must be 1 or 2");
    const uint64_t total = group == 1 ? g.p1 : g.p2;
    if (count) *count = total;
    if (!out) return ZK_OK;
    if (capacity_points < total) ZK_FAIL(ZK_ERR_ARG, "zk_groth16_pool_points: buffer too small");
    ZKCHK(g.check_idle("zk_groth16_pool_points: a proof is in flight on this key"));
    const size_t pb = (group == 1 ? 96 : 192) / (wire ? 2 : 1);
    for (size_t v = 0; v < g.sub.size(); v++) {          // the shards are the pool in order
        DeviceScope ds((int)v);
        Groth16Key& k = *g.sub[v];
        const uint64_t lo = group == 1 ? k.lo1 : k.lo2, hi = group == 1 ? k.hi1 : k.hi2;
        ZKCHK(single_pool_points(k, group, out + pb * lo, hi - lo, nullptr, wire));
    }
    return ZK_OK;
}
int group_qap_eval(GroupKey& g, const uint8_t* sol, uint8_t* v_out, uint8_t* w_out, uint8_t* h_out) {
    ZKCHK(g.check_idle("zk_groth16_qap_eval: a proof is in flight on this key"));
    DeviceScope ds(0);
    return single_qap_eval(*g.sub[0], sol, v_out, w_out, h_out);          // every shard holds the whole circuit and the Fr-stage tables
}

// zk_groth16_pk_derive_lagrange on a multi-device key: the three derived sets -- [l_i(tau)]_1, [l_i(tau)]_2, the h bases -- are
// independent, so each is derived on ONE device (devices 0, 1, 2 of the list; 0, 1, 0 on two), from a copy of the whole tau-power pools gathered out
// of the shards; every set then travels to every device and each device installs its shard of the Lagrange-form pools (own window tables).
int group_derive_lagrange(GroupKey& g) {
    if (g.lagrange) return ZK_OK;
    ZKCHK(g.check_idle("zk_groth16_pk_derive_lagrange: a proof is in flight on this key"));
    trace("derive: sync");
    ZKCHK(g.sync_all());
    trace("derive: synced");
    const int N = (int)g.sub.size();
    const uint64_t n = g.n, p1o = g.p1, p2o = g.p2, p1n = 3 + n + (n - 1) + g.n_mid, p2n = 2 + n;
    int owner[3] = {0, N > 1 ? 1 : 0, N > 2 ? 2 : 0};
    std::vector<uint32_t> sets(N, 0);
    for (int sidx = 0; sidx < 3; sidx++) sets[owner[sidx]] |= 1u << sidx;
    std::vector<DevBuf> in1(N), in2(N), full1(N), full2(N);
    for (int v = 0; v < N; v++) {
        DeviceScope ds(v);
        ZKCHK(full1[v].alloc(96 * p1n));
        ZKCHK(full2[v].alloc(192 * p2n));
        if (sets[v]) {
            ZKCHK(in1[v].alloc(96 * p1o));
            ZKCHK(in2[v].alloc(192 * p2o));
        }
    }
    trace("derive: gather");
    // ---- gather: every shard's slice of the pools, dense affine, to every deriving device (window 0 of a shard's tables IS its slice in pool order)
    for (int v = 0; v < N; v++) {
        DeviceScope ds(v);
        Groth16Key& k = *g.sub[v];
        Ctx& c = ctx();
        DevBuf t1, t2;
        ZKCHK(t1.alloc(96 * (k.hi1 - k.lo1)));
        ZKCHK(t2.alloc(192 * (k.hi2 - k.lo2)));
        ZKCHK(msm_bases_dense(k.g1, 0, k.hi1 - k.lo1, t1.p, c.stream));
        ZKCHK(msm_bases_dense(k.g2, 0, k.hi2 - k.lo2, t2.p, c.stream));
        for (int d = 0; d < N; d++) {
            if (!sets[d]) continue;
            ZKCHK(copy_between(in1[d].as<char>() + 96 * k.lo1, d, t1.p, v, 96 * (k.hi1 - k.lo1), c.stream));
            ZKCHK(copy_between(in2[d].as<char>() + 192 * k.lo2, d, t2.p, v, 192 * (k.hi2 - k.lo2), c.stream));
        }
        HIPCHK(hipStreamSynchronize(c.stream));
    }
    trace("derive: derive sets");
    // ---- derive: one host thread per deriving device (the derivation synchronises its stream between phases)
    int rc = on_every_device((size_t)N, [&](int v) -> int {
        if (!sets[v]) return ZK_OK;
        Ctx& c = ctx();
        ZKCHK(groth16_derive_lagrange_pools(g.sub[v]->fr, in1[v].as<uint8_t>(), g.n_mid, in2[v].as<uint8_t>(), full1[v].as<uint8_t>(), full2[v].as<uint8_t>(), sets[v], c.stream));
        HIPCHK(hipStreamSynchronize(c.stream));
        return ZK_OK;
    });
    if (rc != ZK_OK) return rc;          // nothing of the key has changed yet
    trace("derive: copy sets");
    // ---- every set (and the copied parts a | d1 | b1, ltd_mid, b2 | d2, which every derivation writes) to every other device
    struct Region { int src; int pool; uint64_t lo, hi; };
    const Region regions[6] = {{owner[0], 1, 3, 3 + n}, {owner[1], 2, 2, 2 + n}, {owner[2], 1, 3 + n, 3 + n + (n - 1)},
                               {owner[0], 1, 0, 3}, {owner[0], 1, 3 + n + (n - 1), p1n}, {owner[0], 2, 0, 2}};
    for (int v = 0; v < N; v++) {
        DeviceScope ds(v);
        Ctx& c = ctx();
        for (const Region& rg : regions) {
            if (rg.src == v || rg.hi <= rg.lo) continue;
            const size_t pb = rg.pool == 1 ? 96 : 192;
            char* dst = (rg.pool == 1 ? full1[v] : full2[v]).as<char>();
            const char* src = (rg.pool == 1 ? full1[rg.src] : full2[rg.src]).as<char>();
            ZKCHK(copy_between(dst + pb * rg.lo, v, src + pb * rg.lo, rg.src, pb * (rg.hi - rg.lo), c.stream));
        }
        HIPCHK(hipStreamSynchronize(c.stream));
    }
    for (int v = 0; v < N; v++) { in1[v].release(); in2[v].release(); }
    trace("derive: install");
    // ---- install: each device builds the window tables of ITS slice of the new pools and flips its Fr stage.  From the first commit on the key
    // is only consistent once every device has succeeded.
    g.drop_slots();          // group slots refer to the shards' slots, which the install replaces
    rc = on_every_device((size_t)N, [&](int v) { return groth16_install_lagrange(*g.sub[v], full1[v].p, full2[v].p, (uint32_t)v, (uint32_t)N); });
    if (rc != ZK_OK) {
        g.broken = true;
        return rc;
    }
    trace("derive: done");
    g.lagrange = true;
    g.p1 = p1n;
    g.p2 = p2n;
    return ZK_OK;
}

}  // namespace zk
