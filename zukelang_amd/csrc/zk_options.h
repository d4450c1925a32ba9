// The options of libzkmi355x.so: every ZK_* name the library reads, in ONE table -- its name, WHEN it is read and WHO may set it -- and the only
// code that reads one.  Host-only, plain C++17 (no HIP include): tests/host/options_main.cpp builds it alone under AddressSanitizer + UBSan and under
// ThreadSanitizer.  tests/test_option_cases.py parses the table below and holds tests/option_cases.py (how the suite exercises each public name) to it.
//
// A value comes from zk_set_option (the C-ABI's own configuration call: a host that cannot set the process environment reliably after dlopen -- an
// OCaml program -- uses that), else from the environment variable of the same name, else the option is unset.
//
// kind -- when a read looks:
//   CACHED  the first read, at whichever site, fixes the value for the process: zk_set_option acts on what has not run yet (set options before the first
//           key is uploaded).  Afterwards a read is one atomic load and a branch: no lock, no getenv, no string compare on a proof's path.
//   LIVE    read at every use (key set-up paths; the GPU suite runs several values in one process).
//   FORM    a kernel-form switch of a proof: CACHED, unless the process was started with ZK_TEST_FORMS=1 (tests/conftest.py sets it): then LIVE, so that
//           the GPU suite can hold every form to the oracle inside one process.  Every form computes the same bytes.
// visibility -- who may set it:
//   PUBLIC    zk_set_option accepts it, with or without its "ZK_" prefix, in either case (include/zkmi355x.h documents these)
//   INTERNAL  tuning experiments: environment only, zk_set_option refuses the name
//   ENV_ONLY  diagnostics and test mode: environment only, zk_set_option refuses the name
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "zk_err.h"

// clang-format off
#define ZK_OPTIONS(ZK_OPTION) \
    ZK_OPTION(MSM_WINDOW,            "ZK_MSM_WINDOW",            LIVE,   PUBLIC)   /* Pippenger window bits of keys uploaded afterwards (default: per key size, msm_auto_window / groth16.hip key_window) */ \
    ZK_OPTION(KEY_SUBGROUP_CHECK,    "ZK_KEY_SUBGROUP_CHECK",    LIVE,   PUBLIC)   /* 0: skip the [r] P = O test of key points at upload (keys checked before); folded 17-bit windows are then not used */ \
    ZK_OPTION(SLOT_STREAMS,          "ZK_SLOT_STREAMS",          CACHED, PUBLIC)   /* 3: three streams for every proof slot, 1: one (unset: slot 0 alone forks, while it is the only proof in flight) */ \
    ZK_OPTION(SERIAL_STREAMS,        "ZK_SERIAL_STREAMS",        CACHED, PUBLIC)   /* set to anything: a lone proof stays on one stream, Groth16 and Pinocchio */ \
    ZK_OPTION(GRAPH,                 "ZK_GRAPH",                 FORM,   PUBLIC)   /* 1: capture each slot's Groth16 proof into a hipGraph and replay it */ \
    ZK_OPTION(MSM_CHUNK_MIN,         "ZK_MSM_CHUNK_MIN",         CACHED, PUBLIC)   /* accumulate chunking: the shortest chunk, in sorted entries (16) */ \
    ZK_OPTION(MSM_TARGET_THREADS,    "ZK_MSM_TARGET_THREADS",    CACHED, PUBLIC)   /* accumulate chunking: lanes a product is cut for (256 Ki) */ \
    ZK_OPTION(SORT_TWO_LEVEL,        "ZK_SORT_TWO_LEVEL",        LIVE,   PUBLIC)   /* 0: never sort in two levels (A/B; above 2^15 buckets that is the global-atomic sort) */ \
    ZK_OPTION(SORT_TWO_LEVEL_MIN,    "ZK_SORT_TWO_LEVEL_MIN",    LIVE,   PUBLIC)   /* log2 of the (scalar, window) pairs from which a sort takes two levels (20, or 22 above 2^16 buckets) */ \
    ZK_OPTION(SORT_MIN_WGS,          "ZK_SORT_MIN_WGS",          CACHED, PUBLIC)   /* workgroups below which the single-level LDS sort yields to the global atomics (8) */ \
    ZK_OPTION(SORT_SCALAR_MAJOR,     "ZK_SORT_SCALAR_MAJOR",     CACHED, PUBLIC)   /* 0: window-major ranges in the LDS sorts */ \
    ZK_OPTION(SORT_FINE_STAGED,      "ZK_SORT_FINE_STAGED",      FORM,   PUBLIC)   /* 0 / 1: second level of the two-level sort with plain stores / staged through LDS (default: by pairs per coarse bin) */ \
    ZK_OPTION(SORT_COARSE_STAGED,    "ZK_SORT_COARSE_STAGED",    FORM,   PUBLIC)   /* 1: the first level of the two-level sort staged the same way (off) */ \
    ZK_OPTION(TAIL_SLOTS,            "ZK_TAIL_SLOTS",            FORM,   PUBLIC)   /* 0 / 1: digit sums one lane per point / on slots (default: by window width) */ \
    ZK_OPTION(TAIL_FIXUP_SLOTS,      "ZK_TAIL_FIXUP_SLOTS",      FORM,   PUBLIC)   /* 1: the chunk fix-up on slots (default: lanes) */ \
    ZK_OPTION(FIXUP_BY_CHUNK,        "ZK_FIXUP_BY_CHUNK",        FORM,   PUBLIC)   /* 0: the fix-up always takes one worker per bucket */ \
    ZK_OPTION(DS_WIDE_GROUP,         "ZK_DS_WIDE_GROUP",         FORM,   PUBLIC)   /* 16 / 32 / 64: points per digit value in the digit-sum kernels of windows above 16 bits (32) */ \
    ZK_OPTION(RED_WAVES,             "ZK_RED_WAVES",             FORM,   PUBLIC)   /* 1 / 2: waves per SIMD the reduction kernels are compiled for (2) */ \
    ZK_OPTION(ACC_G1_GLDS,           "ZK_ACC_G1_GLDS",           FORM,   PUBLIC)   /* 0: the register look-ahead of the G1 accumulate instead of the LDS-DMA one */ \
    ZK_OPTION(ACC_G1_MMADD,          "ZK_ACC_G1_MMADD",          FORM,   PUBLIC)   /* 1: the 6-product second step of the G1 accumulate */ \
    ZK_OPTION(ACC_G2_INLINE,         "ZK_ACC_G2_INLINE",         FORM,   PUBLIC)   /* 0: the G2 accumulate with its field products out of line */ \
    ZK_OPTION(MSM_BA_CURVES,         "ZK_MSM_BA_CURVES",         LIVE,   PUBLIC)   /* automatic batch-affine rounds for bit 0: G1, bit 1: G2 (default: neither) */ \
    ZK_OPTION(MSM_BA_ROUNDS,         "ZK_MSM_BA_ROUNDS",         LIVE,   PUBLIC)   /* 0: no batch-affine rounds, k > 0: exactly k, on both curves */ \
    ZK_OPTION(MSM_API_PRECOMP,       "ZK_MSM_API_PRECOMP",       LIVE,   PUBLIC)   /* 1: zk_msm_g1 / zk_msm_g2 run through the resident-key machinery */ \
    ZK_OPTION(DERIVE_SIDE_BY_SIDE,   "ZK_DERIVE_SIDE_BY_SIDE",   LIVE,   PUBLIC)   /* 0 / 1: the pools of a Lagrange derivation one after another / side by side (default: by size) */ \
    ZK_OPTION(FR_RNS,                "ZK_FR_RNS",                FORM,   PUBLIC)   /* 1: the Fr stage's convolutions through the residue number system of rns_ntt.hip (off) */ \
    ZK_OPTION(PIN_SHARED_SORT,       "ZK_PIN_SHARED_SORT",       LIVE,   PUBLIC)   /* 0: every Pinocchio product sorts its own scalar vector (default: vv / vav, yy / yay, ww / waw share one sort each) */ \
    ZK_OPTION(PIN_COMPACT_H,         "ZK_PIN_COMPACT_H",         LIVE,   PUBLIC)   /* 0: Pinocchio keys uploaded afterwards keep v_all | w_all in the h pool (pinocchio.hip: the compact h pool is the default) */ \
    ZK_OPTION(EXPERIMENT_TABLE_ALIAS, "ZK_EXPERIMENT_TABLE_ALIAS", CACHED, INTERNAL) /* builds with -DZK_EXPERIMENTS only (msm_digits.cuh: alias_windows; results WRONG by design) */ \
    ZK_OPTION(BA_TARGET_LANES,       "ZK_BA_TARGET_LANES",       CACHED, INTERNAL) /* batch-affine rounds: lanes per round (16384) */ \
    ZK_OPTION(BA_LMIN,               "ZK_BA_LMIN",               CACHED, INTERNAL) /* batch-affine rounds: fewest additions that share an inversion (16) */ \
    ZK_OPTION(BA_LMAX,               "ZK_BA_LMAX",               CACHED, INTERNAL) /* batch-affine rounds: most additions that share an inversion (128) */ \
    ZK_OPTION(TRACE,                 "ZK_TRACE",                 CACHED, ENV_ONLY) /* set: fatal-signal backtraces, one stderr line per table growth and per multi-device step */ \
    ZK_OPTION(TEST_FORMS,            "ZK_TEST_FORMS",            CACHED, ENV_ONLY) /* 1: FORM rows are read at every use */
// clang-format on

namespace zk {

enum class OptKind { CACHED, LIVE, FORM };
enum class OptVisibility { PUBLIC, INTERNAL, ENV_ONLY };
enum OptId {
#define ZK_OPTION_ID(id, name, kind, vis) OPT_##id,
    ZK_OPTIONS(ZK_OPTION_ID)
#undef ZK_OPTION_ID
    OPT_COUNT
};
struct OptRow {
    const char* name;
    OptKind kind;
    OptVisibility vis;
};
inline constexpr OptRow OPT_ROWS[OPT_COUNT] = {
#define ZK_OPTION_ROW(id, name, kind, vis) {name, OptKind::kind, OptVisibility::vis},
    ZK_OPTIONS(ZK_OPTION_ROW)
#undef ZK_OPTION_ROW
};

// Per row: what zk_set_option gave (nullptr: nothing, the environment decides) and, once a CACHED read has happened, the value it found.  The strings
// are never freed or overwritten in place: a call site, or the state a captured graph was made under, may keep the pointer for the life of the process.
inline const char OPT_UNREAD[1] = {0};          // `fixed` before the first cached read (a value may well be nullptr: unset)
struct OptSlot {
    std::atomic<const char*> set{nullptr};
    std::atomic<const char*> fixed{OPT_UNREAD};
};
inline OptSlot opt_slots[OPT_COUNT];
struct OptWriters {          // what only zk_set_option and a FIRST cached read touch
    std::mutex mu;
    std::vector<std::unique_ptr<std::string>> arena;
};
inline OptWriters& opt_writers() {
    static OptWriters* w = new OptWriters;          // never destroyed: reads may outlive the static destructors
    return *w;
}

inline bool forms_live();
inline const char* opt_str(OptId id) {
    OptSlot& s = opt_slots[id];
    const char* v = s.fixed.load(std::memory_order_acquire);
    if (v != OPT_UNREAD) return v;
    const OptKind kind = OPT_ROWS[id].kind;
    if (kind == OptKind::LIVE || (kind == OptKind::FORM && forms_live())) {
        v = s.set.load(std::memory_order_acquire);
        return v ? v : getenv(OPT_ROWS[id].name);
    }
    std::lock_guard<std::mutex> g(opt_writers().mu);          // the first read of a cached row: concurrent first reads agree on one value
    v = s.fixed.load(std::memory_order_relaxed);
    if (v != OPT_UNREAD) return v;
    v = s.set.load(std::memory_order_relaxed);
    if (!v) v = getenv(OPT_ROWS[id].name);
    s.fixed.store(v, std::memory_order_release);
    return v;
}
// The parse rules.  Every site that tells "set" from "unset", or "0" from anything else, goes through one of these:
inline bool opt_is_set(OptId id) { return opt_str(id) != nullptr; }          // set to anything, "" and "0" included
inline int opt_int(OptId id, int dflt) {                                     // atoi of the value ("" and "x" are 0), dflt when unset
    const char* e = opt_str(id);
    return e ? atoi(e) : dflt;
}
inline uint64_t opt_u64(OptId id, uint64_t dflt) {
    const char* e = opt_str(id);
    return e ? (uint64_t)atoll(e) : dflt;
}
// A switch: off when set and atoi == 0, on when set and atoi != 0, dflt when unset.  (id, true) is "off only when set to 0", (id, false) "on iff atoi != 0".
inline bool opt_on(OptId id, bool dflt) { return opt_int(id, dflt ? 1 : 0) != 0; }

inline bool forms_live() { return opt_on(OPT_TEST_FORMS, false); }          // test mode, fixed when the first FORM row is read
inline bool trace_on() { return opt_is_set(OPT_TRACE); }                    // ZK_TRACE diagnostics
// Key points from outside are checked like the reference checks them on the way in (of_bytes_exn, curve.ml:199-212: encoding, curve, prime-order
// subgroup); ZK_KEY_SUBGROUP_CHECK=0 skips the subgroup part -- [r] P = O per point: 0.3 s at 2^20 constraints, 1.4 s at 2^22 -- for keys that were
// checked before.  Read per key (set-up paths).  A pool uploaded without the check never gets folded windows (msm.cuh: msm_fold).
inline bool key_subgroup_check() { return opt_on(OPT_KEY_SUBGROUP_CHECK, true); }

// The kernel forms a proof would be enqueued with now: a hash over the values of every FORM row but GRAPH (which decides whether to capture, not what),
// unset told from empty.  groth16.hip drops a slot's captured graphs when it changes (test mode only: otherwise the rows cannot change).
inline uint64_t opt_form_fingerprint() {
    uint64_t h = 1469598103934665603ull;
    for (int id = 0; id < OPT_COUNT; id++) {
        if (OPT_ROWS[id].kind != OptKind::FORM || id == OPT_GRAPH) continue;
        const char* v = opt_str((OptId)id);
        for (const char* q = v ? v : "\x01"; *q; q++) h = (h ^ (uint8_t)*q) * 1099511628211ull;
        h = (h ^ 0xff) * 1099511628211ull;
    }
    return h;
}

// zk_set_option.  value == nullptr hands the option back to the environment.
inline int opt_set(const char* name, const char* value) {
    if (!name || !*name) ZK_FAIL(ZK_ERR_ARG, "zk_set_option: no name");
    std::string up;
    for (const char* q = name; *q; q++) up.push_back((char)((*q >= 'a' && *q <= 'z') ? *q - 32 : *q));
    if (up.compare(0, 3, "ZK_") != 0) up = "ZK_" + up;
    int id = 0;
    while (id < OPT_COUNT && !(OPT_ROWS[id].vis == OptVisibility::PUBLIC && up == OPT_ROWS[id].name)) id++;
    if (id == OPT_COUNT) ZK_FAIL(ZK_ERR_ARG, "zk_set_option: unknown option name");
    OptWriters& w = opt_writers();
    std::lock_guard<std::mutex> g(w.mu);
    const char* stored = nullptr;
    if (value) {
        w.arena.push_back(std::make_unique<std::string>(value));
        stored = w.arena.back()->c_str();
    }
    opt_slots[id].set.store(stored, std::memory_order_release);
    return ZK_OK;
}

}  // namespace zk
