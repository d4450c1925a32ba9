// Stand-alone check of csrc/ctx_tables.h (tests/test_ctx_tables.py builds it with g++ under AddressSanitizer + UBSan and runs it): a context table
// that grows 2^12 -> 2^13 -> 2^15 with malloc / free as the allocator, read through EVERY pointer it ever handed out after every growth.
// Exit status 0 and "ctx_tables ok" on stdout: every check held.  A policy that frees on growth ends in an AddressSanitizer report at the first read.
#include "../../zukelang_amd/csrc/ctx_tables.h"

#include <map>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace zk;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

// the allocator the policy is handed: every buffer it gave and how often each came back
static std::map<void*, int> g_freed;          // pointer -> times released
static int g_allocs = 0, g_fail_next = 0;
static int test_alloc(size_t bytes, void** p) {
    if (g_fail_next) { g_fail_next = 0; return -5; }
    *p = malloc(bytes);
    if (!*p) return -5;
    g_allocs++;
    CHECK(g_freed.find(*p) == g_freed.end() || g_freed[*p] == 1);          // malloc may hand a released address out again
    g_freed[*p] = 0;
    return 0;
}
static void test_free(void* p) {
    CHECK(g_freed.count(p));
    g_freed[p]++;
    free(p);
}

// what the heaps of ntt.hip hold, in small: entry i depends on i alone (level and index within the level), never on the table's size
static uint32_t entry(uint64_t i) { return (uint32_t)(i * 2654435761u) ^ (uint32_t)(i >> 7) ^ 0x5eed0000u; }
static void fill(void* p, uint32_t log_cap) {
    uint32_t* w = (uint32_t*)p;
    for (uint64_t i = 0; i < ((uint64_t)1 << log_cap); i++) w[i] = entry(i);
}

struct Held {          // a pointer as an enqueue or a captured graph holds it: the address and the size it was handed out with
    const uint32_t* p;
    uint32_t log_cap;
};

int main() {
    CHECK(ctx_table_log_cap(0, 12) == 12 && ctx_table_log_cap(12, 12) == 12 && ctx_table_log_cap(13, 12) == 13 && ctx_table_log_cap(3, 14) == 14);

    GrowingTable t;
    CHECK(!t.live() && t.log_cap() == 0 && !t.covers(0) && !t.covers(12) && t.retired() == 0 && t.retired_bytes() == 0);

    std::vector<Held> held;
    const uint32_t steps[3] = {12, 13, 15};
    for (int s = 0; s < 3; s++) {
        const uint32_t k = ctx_table_log_cap(steps[s], 12);
        CHECK(!t.covers(k));
        CHECK(t.grow(k, (size_t)4 << k, test_alloc) == 0);
        CHECK(t.live() && t.log_cap() == k && t.bytes() == (size_t)4 << k && t.covers(k) && t.covers(1) && !t.covers(k + 1));
        fill(t.live(), k);
        held.push_back(Held{(const uint32_t*)t.live(), k});
        // every pointer handed out so far: still readable, its values untouched, and equal to the prefix of the new table
        const uint32_t* now = (const uint32_t*)t.live();
        for (const Held& h : held) {
            CHECK(h.log_cap <= k);
            for (uint64_t i = 0; i < ((uint64_t)1 << h.log_cap); i++) {
                CHECK(h.p[i] == entry(i));
                CHECK(h.p[i] == now[i]);
            }
        }
        // the bookkeeping comes after the reads: they are what a kernel does.  The retired buffers together cost less than the live one
        CHECK(t.retired() == (size_t)s);
        CHECK(t.retired_bytes() < t.bytes());
        // a request the live buffer covers allocates nothing and moves nothing
        const int before = g_allocs;
        CHECK(t.grow(k, (size_t)4 << k, test_alloc) == -1 && t.grow(k - 1, (size_t)4 << (k - 1), test_alloc) == -1);
        CHECK(g_allocs == before && t.live() == (void*)held.back().p && t.retired() == (size_t)s);
    }
    CHECK(held.size() == 3 && held[0].p != held[1].p && held[1].p != held[2].p && held[0].p != held[2].p);

    // a failed allocation changes nothing: the live buffer stays, nothing is retired, the code comes back as it is
    g_fail_next = 1;
    CHECK(t.grow(16, (size_t)4 << 16, test_alloc) == -5);
    CHECK(t.live() == (void*)held[2].p && t.log_cap() == 15 && t.retired() == 2 && g_allocs == 3);
    for (const Held& h : held)
        for (uint64_t i = 0; i < ((uint64_t)1 << h.log_cap); i += 97) CHECK(h.p[i] == entry(i));

    // nothing was released so far; release: every buffer exactly once, the table empty
    for (auto& kv : g_freed) CHECK(kv.second == 0);
    t.release_all(test_free);
    CHECK(g_freed.size() == 3);
    for (auto& kv : g_freed) CHECK(kv.second == 1);
    CHECK(!t.live() && t.log_cap() == 0 && t.bytes() == 0 && t.retired() == 0 && !t.covers(0));
    t.release_all(test_free);          // a second release finds nothing
    for (auto& kv : g_freed) CHECK(kv.second == 1);

    // a released table starts again at its floor (zk_shutdown, then zk_init)
    CHECK(t.grow(12, (size_t)4 << 12, test_alloc) == 0 && t.covers(12) && t.retired() == 0);
    fill(t.live(), 12);
    CHECK(((const uint32_t*)t.live())[4095] == entry(4095));
    t.release_all(test_free);
    for (auto& kv : g_freed) CHECK(kv.second == 1);
    printf("ctx_tables ok\n");
    return 0;
}
