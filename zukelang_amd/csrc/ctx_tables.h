// Context-owned device tables that grow after their first use: what is kept, what is handed out, and when anything may be released.
// Host-only, plain C++17 (no HIP include): tests/host/ctx_tables_main.cpp builds it alone under AddressSanitizer + UBSan with malloc / free as the
// allocator.  The library is called from one host thread (include/zkmi355x.h): no locking.
//
// THE RULE (include/zkmi355x.h, next to ZK_GRAPH; DESIGN.md "Context-owned tables"): a device pointer to a context table, once handed to an enqueue or
// a capture, stays valid and keeps its values until zk_shutdown.  The holders are kernels queued on any stream of the device (a proof in flight on a
// slot stream of ANOTHER key) and the kernel arguments frozen into a captured graph (ZK_GRAPH=1: groth16.hip prove_enqueue), which nobody can reach
// from here.  So a table that has to grow RETIRES its buffer instead of freeing it: the new buffer becomes the live one, the old one stays allocated,
// untouched, until release_all -- the owner's cleanup hook, which zk_shutdown runs after every handle (and so every graph) is gone.
// The tables grow geometrically (each growth at least doubles: grow refuses anything else), so all retired buffers together cost less than the live one.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "zk_options.h"

namespace zk {

// The capacity a request is served with: the table's floor, or the request itself.
static inline uint32_t ctx_table_log_cap(uint32_t want_log, uint32_t floor_log) { return want_log < floor_log ? floor_log : want_log; }

// ZK_TRACE=1 (diagnostics, environment only): one line on stderr per growth, "[zk tables] <what>: 2^<from> -> 2^<to>, <n> retired" (from 0: the first
// table).  tests/test_gpu_live_together.py reads the lines of its child processes: a scenario that is meant to move a table shows that it did.
static inline void ctx_table_trace(const char* what, uint32_t from_log, uint32_t to_log, size_t retired) {
    if (trace_on()) {
        fprintf(stderr, "[zk tables] %s: 2^%u -> 2^%u, %zu retired\n", what, from_log, to_log, retired);
        fflush(stderr);
    }
}

class GrowingTable {
  public:
    GrowingTable() = default;
    GrowingTable(const GrowingTable&) = delete;
    GrowingTable& operator=(const GrowingTable&) = delete;

    void* live() const { return live_.p; }                    // what an enqueue or a capture is handed; nullptr before the first growth
    uint32_t log_cap() const { return live_.log_cap; }        // the live buffer serves sizes up to 2^log_cap
    size_t bytes() const { return live_.bytes; }
    bool covers(uint32_t log_n) const { return live_.p && live_.log_cap >= log_n; }
    size_t retired() const { return retired_.size(); }
    size_t retired_bytes() const {
        size_t n = 0;
        for (const Buf& b : retired_) n += b.bytes;
        return n;
    }

    // A new live buffer of `bytes` bytes for sizes up to 2^log_cap, from alloc(bytes, &p) -> 0 on success (any other value is returned as it is and
    // nothing changes: the old buffer stays the live one).  The old live buffer is retired, not freed.  The caller fills the new buffer and makes
    // that visible to every stream before it returns the pointer to anybody (ntt.hip, rns_ntt.hip).  Returns -1, and allocates nothing, for a request
    // the live buffer already covers: a table never shrinks and never moves without need.
    template <class Alloc> int grow(uint32_t log_cap, size_t bytes, Alloc alloc) {
        if (covers(log_cap)) return -1;
        void* p = nullptr;
        const int rc = alloc(bytes, &p);
        if (rc != 0) return rc;
        if (live_.p) retired_.push_back(live_);
        live_ = Buf{p, bytes, log_cap};
        return 0;
    }
    // Every buffer this table ever got, live and retired, goes to dealloc(p) exactly once; the table is empty afterwards and may grow again.
    // Only where nothing can hold a pointer any more: zk_shutdown's cleanup hooks (handles released, device idle).
    template <class Free> void release_all(Free dealloc) {
        for (const Buf& b : retired_) dealloc(b.p);
        retired_.clear();
        if (live_.p) dealloc(live_.p);
        live_ = Buf{};
    }

  private:
    struct Buf {
        void* p = nullptr;
        size_t bytes = 0;
        uint32_t log_cap = 0;
    };
    Buf live_;
    std::vector<Buf> retired_;
};

}  // namespace zk
