// Stand-alone check of csrc/handle_table.h (tests/test_handle_table.py builds it with g++ under AddressSanitizer + UBSan and runs it).
// Exit status 0 and "handle_table ok" on stdout: every check held.
#include "../../zukelang_amd/csrc/handle_table.h"

#include <stdio.h>
#include <stdlib.h>

using namespace zk;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static int g_destroyed = 0;
struct Obj {
    int tag;
    int visits = 0;
    explicit Obj(int t) : tag(t) {}
    ~Obj() { g_destroyed++; }
};

int main() {
    // ---- the ranges: six kinds, each starting at 1 within its own 2^32 numbers, the documented values
    CHECK(HANDLE_KINDS == 6);
    for (size_t i = 0; i < HANDLE_KINDS; i++) {
        CHECK((HANDLE_RANGES[i] & 0xffffffffull) == 1);
        for (size_t j = 0; j < HANDLE_KINDS; j++) {
            if (i == j) continue;
            const uint64_t lo_i = HANDLE_RANGES[i], hi_i = (HANDLE_RANGES[i] | 0xffffffffull), lo_j = HANDLE_RANGES[j], hi_j = (HANDLE_RANGES[j] | 0xffffffffull);
            CHECK(hi_i < lo_j || hi_j < lo_i);
        }
    }
    CHECK(HANDLES_GROTH16 == 1 && HANDLES_PINOCCHIO == 0x5000000001ull && HANDLES_GROTH16_GROUP == 0x6000000001ull);
    CHECK(HANDLES_PINOCCHIO_GROUP == 0x7000000001ull && HANDLES_VERIFICATION_KEY == 0x7100000001ull && HANDLES_RESIDENT_BASES == 0x7200000001ull);

    // three tables, never destroyed, as in the library
    auto& a = *new HandleTable<Obj>(HANDLES_PINOCCHIO_GROUP, "unknown a");
    auto& b = *new HandleTable<Obj>(HANDLES_RESIDENT_BASES, "unknown b");
    auto& c = *new HandleTable<Obj>(HANDLES_GROTH16, "unknown c");
    CHECK(HandleTableBase::live_in_all_tables() == 0);
    CHECK(a.unknown()[8] == 'a' && b.unknown()[8] == 'b');

    // ---- add / find / take round trip; the first numbers are the ranges' first numbers
    const uint64_t a1 = a.add(std::make_unique<Obj>(11)), a2 = a.add(std::make_unique<Obj>(12));
    const uint64_t b1 = b.add(std::make_unique<Obj>(21));
    const uint64_t c1 = c.add(std::make_unique<Obj>(31)), c2 = c.add(std::make_unique<Obj>(32)), c3 = c.add(std::make_unique<Obj>(33));
    CHECK(a1 == HANDLES_PINOCCHIO_GROUP && a2 == a1 + 1 && b1 == HANDLES_RESIDENT_BASES && c1 == 1 && c2 == 2 && c3 == 3);
    CHECK(a.find(a1) && a.find(a1)->tag == 11 && a.find(a2)->tag == 12 && b.find(b1)->tag == 21 && c.find(c3)->tag == 33);
    CHECK(a.size() == 2 && b.size() == 1 && c.size() == 3);
    CHECK(HandleTableBase::live_in_all_tables() == 6);

    // ---- another table's live number, 0, and a number never handed out: null from find and from take, and nothing changes
    CHECK(!a.find(b1) && !a.find(c1) && !b.find(a1) && !b.find(c2) && !c.find(a2) && !c.find(b1));
    CHECK(!a.find(0) && !b.find(0) && !c.find(0) && !c.find(4) && !a.find(a2 + 1));
    CHECK(!a.take(b1) && !a.take(c1) && !b.take(a1) && !c.take(b1) && !a.take(0) && !c.take(0));
    CHECK(g_destroyed == 0 && HandleTableBase::live_in_all_tables() == 6);

    // ---- take: the object leaves the table alive, dies exactly once with the returned pointer, and its number is unknown afterwards
    {
        std::unique_ptr<Obj> o = a.take(a1);
        CHECK(o && o->tag == 11 && g_destroyed == 0);
        CHECK(!a.find(a1) && a.size() == 1 && HandleTableBase::live_in_all_tables() == 5);
    }
    CHECK(g_destroyed == 1);
    CHECK(!a.take(a1) && !a.find(a1) && g_destroyed == 1);
    c.take(c2);          // the temporary dies at the end of the statement
    CHECK(g_destroyed == 2 && !c.find(c2) && c.find(c1) && c.find(c3) && HandleTableBase::live_in_all_tables() == 4);
    // numbers are not reused
    const uint64_t a3 = a.add(std::make_unique<Obj>(13)), c4 = c.add(std::make_unique<Obj>(34));
    CHECK(a3 == a2 + 1 && c4 == 4 && HandleTableBase::live_in_all_tables() == 6);

    // ---- release: every live entry once, in ascending handle order, each destroyed; the registry follows
    int order[8], visited = 0;
    c.release_all([&](Obj& o) {
        o.visits++;
        CHECK(o.visits == 1);
        order[visited++] = o.tag;
    });
    CHECK(visited == 3 && order[0] == 31 && order[1] == 33 && order[2] == 34);
    CHECK(g_destroyed == 5 && c.size() == 0 && !c.find(c1) && !c.find(c4) && HandleTableBase::live_in_all_tables() == 3);
    a.release_all();
    CHECK(g_destroyed == 7 && a.size() == 0 && HandleTableBase::live_in_all_tables() == 1);
    b.release_all();
    CHECK(g_destroyed == 8 && HandleTableBase::live_in_all_tables() == 0);
    // a released table goes on counting where it stopped
    CHECK(c.add(std::make_unique<Obj>(35)) == 5 && HandleTableBase::live_in_all_tables() == 1);
    c.release_all();
    CHECK(g_destroyed == 9);
    printf("handle_table ok\n");
    return 0;
}
