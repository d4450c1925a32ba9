// Internal interface of the Groth16 prover (groth16.hip) that the multi-device form (groth16_multi.hip) builds on: the key and slot records and the
// two halves of a proof -- Fr stage -> scalar vectors, multi-scalar products over a slice of the pools -- as enqueue-only functions.
#pragma once
#include "contribute_scalar.h"
#include "frstage.cuh"
#include "msm.cuh"

#include <memory>
#include <vector>

namespace zk {

// Everything one proof in flight owns: scratch of the Fr stage, the three scalar vectors, one MSM
// workspace and one stream per product, pinned host landing buffers.  Several slots let the shallow
// single-wave tails of one proof (bucket reduction, affine conversion) run under the bulk kernels
// of the next.
struct Slot {
    FrScratch fs;
    DevBuf scalA, scalC, scalB, wit_raw, rs, results, out_dev;
    MsmWorkspace wsA, wsC, wsB;
    hipStream_t s0 = nullptr, s1 = nullptr, s2 = nullptr;     // C + Fr stage | B (G2) | A
    hipEvent_t fork = nullptr, join1 = nullptr, join2 = nullptr, done = nullptr;
    uint8_t* host = nullptr;            // pinned: proof 384 B | flag 4 B | r 32 B | s 32 B
    uint8_t* host_partial = nullptr;    // pinned: 768 B of raw partial sums (sharded mode)
    uint8_t* wit_pinned = nullptr;      // pinned staging copy of a witness handed over as a host buffer (allocated at first use): the caller's
                                        // buffer is read before the call returns, as the header promises, whatever memory it lives in
    bool busy = false, serial = false;
    // ZK_GRAPH=1: the whole proof of this slot captured ONCE per shape (streams forked or not | raw partial sums | witness from the host) and replayed
    hipGraphExec_t graph[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint64_t graph_forms = 0;           // hash of the kernel-form switches the graphs were captured under (test mode only)
    ~Slot() {
        for (hipGraphExec_t g : graph)
            if (g) (void)hipGraphExecDestroy(g);
        if (s0) { (void)hipStreamDestroy(s0); if (!serial) { (void)hipStreamDestroy(s1); (void)hipStreamDestroy(s2); } }
        if (fork) { (void)hipEventDestroy(fork); (void)hipEventDestroy(join1); (void)hipEventDestroy(join2); (void)hipEventDestroy(done); }
        if (host) (void)hipHostFree(host);
        if (wit_pinned) (void)hipHostFree(wit_pinned);
    }
};
static constexpr uint32_t MAX_SLOTS = 15;      // + the context stream = the 16 hardware queues the chip runs side by side

struct Groth16Key {
    uint32_t n = 0, m = 0, n_mid = 0;
    uint32_t rank = 0, world = 1;
    uint64_t p1 = 0, p2 = 0;            // full pool sizes (points)
    uint64_t lo1 = 0, hi1 = 0;          // this rank's slice of the G1 pool
    uint64_t lo2 = 0, hi2 = 0;
    FrStage fr;
    MsmBases g1, g2;
    DevBuf mid_idx;                     // variable index of the j-th mid variable
    DevBuf wit_resident;                // zk_groth16_set_witness
    bool have_witness = false;
    bool lagrange = false;              // key holds [l_i(tau)] and the shifted-domain h bases instead of tau powers (row f4)
    std::unique_ptr<Slot> slots[MAX_SLOTS];
    bool one_stream_slots = false;      // shard of a multi-device key: its products always run on the slot's one stream (no extra streams for slot 0)
    int vdev = 0;                       // virtual device (context) the key was built under; every call on it runs with that context current
};


// Builds a key (whole: rank 0 of world 1, or rank's shard) on the CURRENT virtual device; nothing is registered under a handle.
int groth16_key_build(std::unique_ptr<Groth16Key>& out, uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid,
                      const uint8_t* pk_g1, size_t pk_g1_points, const uint8_t* pk_g2, size_t pk_g2_points, uint32_t rank, uint32_t world, bool lagrange,
                      bool shard_of_group = false, const void* d_g1 = nullptr, const void* d_g2 = nullptr, bool wire = false, bool device_in_subgroup = true);
// keygen.hip, specialize.hip: a whole key from pools the library computed on the device (dense affine points, pool order), registered under a new
// handle.  in_subgroup = false: the pools are a linear image of outside points that were not tested (ZK_KEY_SUBGROUP_CHECK=0), and the handle says so
int groth16_key_from_device(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const void* d_g1, size_t g1_points,
                            const void* d_g2, size_t g2_points, bool lagrange, uint64_t* handle, bool in_subgroup = true);
int groth16_slot_get(Groth16Key& k, uint32_t idx, Slot** out);
// host half of a proof's inputs (witness handed over as a host buffer, r, s) into the slot's pinned staging memory; fails when the slot is busy
int groth16_stage_inputs(Groth16Key& k, Slot& sl, const uint8_t* sol, const uint8_t* r, const uint8_t* s);
// Fr stage -> the three scalar vectors over the FULL pools (p1, p1, p2 canonical Fr) at dA / dC / dB; enqueue only (slot stream s0)
int groth16_scalars_enqueue(Groth16Key& k, Slot& sl, const uint8_t* sol, const uint8_t* r, const uint8_t* s, void* dA, void* dC, void* dB, bool staged = false);
// the three products over this key's slice; dA / dC / dB point at the scalars OF THAT SLICE; raw: XYZZ partial sums stay in sl.results (A | C | B)
int groth16_msms_enqueue(Groth16Key& k, Slot& sl, const void* dA, const void* dC, const void* dB, bool raw, int force_serial = -1);
int groth16_prove_finish(Slot& sl);          // waits for sl.done, frees the slot, maps the Fr stage's flags to ZK_ERR_REMAINDER / ZK_ERR_SCALAR_RANGE (status_of_flags)
// replaces the key's pools by rank's slice of the complete Lagrange-form pools at d_g1 / d_g2 (device memory of the key's device) and flips its Fr stage
int groth16_install_lagrange(Groth16Key& k, const void* d_g1, const void* d_g2, uint32_t rank, uint32_t world);
int groth16_derive_lagrange_pools(const FrStage& f, const uint8_t* d_g1, uint64_t n_mid, const uint8_t* d_g2, uint8_t* out_g1, uint8_t* out_g2, uint32_t sets, hipStream_t s);   // lagrange_derive.hip
// lagrange_derive.hip: dst[i] <- k[i] * src[i], dense affine points and canonical scalars on the device (dst may be src), through the derivation's three
// passes k_aff_to_raw, k_g_tabmul, k_raw_to_aff; waits for the stream
int points_scale_tabmul(Curve curve, void* d_dst, const void* d_src, const void* d_k, uint64_t n, hipStream_t s);
// keygen.hip: M (n rows, m columns) -> its transpose as CSR over m rows, a counting pass on the host; ZK_ERR_ARG for a malformed M
int transpose_csr(const zk_csr* M, uint32_t n, uint32_t m, std::vector<uint32_t>& ptr, std::vector<uint32_t>& col, std::vector<uint8_t>& val);
// keygen.hip: out[i] = scale * x^i for i < cnt (k_power_run; x, scale and out in Montgomery form on the device, scale == nullptr: 1); enqueues only
int power_run(void* d_out, const void* d_x, const void* d_scale, uint64_t cnt, hipStream_t s, const char* family = "keygen_powers");
// lagrange_derive.hip, for zk_groth16_pk_specialize: [l_i]_1, [alpha l_i]_1, [beta l_i]_1 from the three G1 lists of a phase-1 string (dst[q] <- the
// derivation of src[q], n points each) and tiztd (n - 1 points) from the 2n-1 points at d_tau1 by one correlation with Z's coefficients; waits
int specialize_g1_bases(const FrStage& f, const uint8_t* const d_src[3], uint8_t* const d_dst[3], const uint8_t* d_tau1, uint8_t* d_tiztd, hipStream_t s);
// pts[i] <- k[i] * pts[i] on raw XYZZ G1 points (k_g_tabmul in slabs; waits), and raw XYZZ -> dense affine (k_raw_to_aff; enqueues only)
int g1_raw_tabmul(void* d_raw, const void* d_k, uint64_t total, hipStream_t s);
int g1_raw_to_affine(void* d_aff, const void* d_raw, uint64_t count, hipStream_t s);
// contribute.hip: pts[i] <- k * pts[i] in place for n dense affine G1 points (device) and ONE canonical scalar (little-endian words), through
// points_scale_tabmul over a table of equal scalars, `slab` points per chain of launches (0 = the default); waits for the stream
int g1_scale_points(void* d_pts, uint64_t n, const uint64_t k[4], uint32_t slab, hipStream_t s);
// key_check.hip: the whole of zk_groth16_key_check behind its argument checks (a tau-power key held whole on one device, no proof in flight); vk_g1 and
// vk_g2 both given or both null; seed: 32 bytes or null (drawn here)
int groth16_key_check(Groth16Key& k, const uint8_t* vk_g1, size_t n_io, const uint8_t* vk_g2, const uint8_t* seed, uint32_t* failed);
// the same for zk_groth16_key_check_lagrange: a Lagrange-form key held whole on one device
int groth16_key_check_lagrange(Groth16Key& k, const uint8_t* vk_g1, size_t n_io, const uint8_t* vk_g2, const uint8_t* seed, uint32_t* failed);
// key_check.hip: product q = the pairs lens[0] + .. + lens[q-1] onwards, lens[q] of them, of P (96 B each) and Q (192 B each), host bytes of points the
// caller has checked or summed itself -> gt: 576 B per product (pairing_products_device); waits.  The key checks and zk_groth16_srs_check compare them.
int keychk_pairing_products(const std::vector<uint8_t>& P, const std::vector<uint8_t>& Q, const std::vector<uint64_t>& lens, std::vector<uint8_t>& gt, hipStream_t s);
void groth16_shard_range(uint64_t points, uint64_t heavy, uint32_t rank, uint32_t world, uint64_t* lo, uint64_t* hi);

// ---- multi-device keys (groth16_multi.hip): one shard per entry of the device list behind ONE handle
struct GroupKey;
GroupKey* group_lookup(uint64_t handle);
void group_release_all();
int group_upload(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid, const uint8_t* pk_g1, size_t pk_g1_points,
                 const uint8_t* pk_g2, size_t pk_g2_points, bool lagrange, uint64_t* handle, bool wire = false);
int group_free(uint64_t handle);
int group_reserve_slots(GroupKey& g, uint32_t count);
int group_set_witness(GroupKey& g, const uint8_t* sol);
int group_prove_async(GroupKey& g, const uint8_t* sol, const uint8_t* r, const uint8_t* s, uint32_t slot);
int group_prove_wait(GroupKey& g, uint32_t slot, uint8_t proof[384]);
int group_derive_lagrange(GroupKey& g);
int group_pool_points(GroupKey& g, int group, uint8_t* out, size_t capacity_points, size_t* count, bool wire = false);
int group_pool_layout(GroupKey& g, uint64_t* p1, uint64_t* p2);
int group_qap_eval(GroupKey& g, const uint8_t* sol, uint8_t* v_out, uint8_t* w_out, uint8_t* h_out);
int group_lagrange_pool_sizes(GroupKey& g, uint64_t* g1_points, uint64_t* g2_points);
// zk_groth16_prove_many_compressed on a multi-device key: proof by proof through the group's slot 0, the sums the first device added up as the proof's row
int group_prove_many(GroupKey& g, const uint8_t* sols, const uint8_t* rs, uint32_t count, uint8_t* proofs, int32_t* status);
// where the sums of a proof (A | C | B, the slot's results) go in its wire record A 48 | B 96 | C 48 (groth16.ml:110-114)
static inline ProofWire groth16_wire_g1() { return {2, ZK_GROTH16_PARTIAL_BYTES, 0, 192, {0, 144, 0, 0, 0, 0}}; }
static inline ProofWire groth16_wire_g2() { return {1, ZK_GROTH16_PARTIAL_BYTES, 384, 192, {48, 0, 0, 0, 0, 0}}; }
int single_qap_eval(Groth16Key& k, const uint8_t* sol, uint8_t* v_out, uint8_t* w_out, uint8_t* h_out);
int single_pool_points(Groth16Key& k, int group, uint8_t* out, size_t capacity_points, size_t* count, bool wire = false);

}  // namespace zk
