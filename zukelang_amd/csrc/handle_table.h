// The library's handle tables: one type for every kind of object the C-ABI hands out as a uint64_t, and the number ranges of all kinds in one place.
// Host-only, plain C++17 (no HIP include): tests/host/handle_table_main.cpp builds it alone under AddressSanitizer + UBSan.
// The library is called from one host thread (include/zkmi355x.h): no locking.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <map>
#include <memory>
#include <vector>

namespace zk {

// First handle number of every kind.  A kind owns the 2^32 numbers that share the upper half of its first one (handle >> 32 names the kind; the lower half
// counts from 1, so 0 is never a handle): a number of one kind is never a number of another, and a table answers a foreign handle "unknown".  The values
// are what hosts and tests have seen since each kind appeared -- all but the resident bases', which shared the Pinocchio groups' range until they moved.
enum HandleRange : uint64_t {
    HANDLES_GROTH16 = 0x0000000001ull,                // Groth16 keys and shards (groth16.hip)
    HANDLES_PINOCCHIO = 0x5000000001ull,              // Pinocchio keys (pinocchio.hip)
    HANDLES_GROTH16_GROUP = 0x6000000001ull,          // multi-device Groth16 keys (groth16_multi.hip)
    HANDLES_PINOCCHIO_GROUP = 0x7000000001ull,        // multi-device Pinocchio keys (pinocchio.hip)
    HANDLES_VERIFICATION_KEY = 0x7100000001ull,       // resident verification keys (verify_resident.hip)
    HANDLES_RESIDENT_BASES = 0x7200000001ull,         // resident MSM bases (msm_resident.hip)
};
static constexpr uint64_t HANDLE_RANGES[] = {HANDLES_GROTH16,           HANDLES_PINOCCHIO,        HANDLES_GROTH16_GROUP,
                                             HANDLES_PINOCCHIO_GROUP,   HANDLES_VERIFICATION_KEY, HANDLES_RESIDENT_BASES};
static constexpr size_t HANDLE_KINDS = sizeof HANDLE_RANGES / sizeof HANDLE_RANGES[0];
static constexpr bool handle_ranges_disjoint() {
    for (size_t i = 0; i < HANDLE_KINDS; i++) {
        if ((HANDLE_RANGES[i] & 0xffffffffull) != 1) return false;
        for (size_t j = 0; j < i; j++)
            if ((HANDLE_RANGES[i] >> 32) == (HANDLE_RANGES[j] >> 32)) return false;
    }
    return true;
}
static_assert(handle_ranges_disjoint(), "every handle kind starts at 1 within a 2^32 range of its own");

// What the registry sees of a table: how many handles are alive.  A table joins the registry when it is constructed; a new kind needs no entry anywhere else.
// size() is the one virtual call of this header; it serves the registry's sum (zk_set_device_list), never the path that enqueues a proof.
class HandleTableBase {
  public:
    virtual size_t size() const = 0;
    // handles alive in every table of the process: the device list may only change at 0 (zk_set_device_list)
    static uint64_t live_in_all_tables() {
        uint64_t n = 0;
        for (const HandleTableBase* t : registry()) n += t->size();
        return n;
    }

  protected:
    HandleTableBase() { registry().push_back(this); }
    HandleTableBase(const HandleTableBase&) = delete;
    HandleTableBase& operator=(const HandleTableBase&) = delete;
    ~HandleTableBase() = default;          // tables are never destroyed, and never through the base

  private:
    static std::vector<const HandleTableBase*>& registry() {
        static auto& r = *new std::vector<const HandleTableBase*>;          // never destroyed, like the tables in it
        return r;
    }
};

// The objects of one kind under their handles.  Tables are heap-allocated and never destroyed (`static HandleTable<T>& g = *new HandleTable<T>(...)`):
// the objects own device memory, and a static destructor must not call into a HIP runtime that is already gone (see ntt.hip) -- zk_shutdown releases
// them through the cleanup hooks instead.
template <class T> class HandleTable : public HandleTableBase {
  public:
    HandleTable(HandleRange first, const char* unknown) : next_(first), unknown_(unknown) {}
    const char* unknown() const { return unknown_; }          // the text of the kind's ZK_ERR_HANDLE
    size_t size() const override { return map_.size(); }
    uint64_t add(std::unique_ptr<T> obj) {
        const uint64_t h = next_++;          // 2^32 - 1 numbers per kind, never reused: a stale handle stays unknown
        map_[h] = std::move(obj);
        return h;
    }
    T* find(uint64_t handle) const {
        auto it = map_.find(handle);
        return it == map_.end() ? nullptr : it->second.get();
    }
    // the object leaves the table and dies with the returned pointer, i.e. where the caller has made its device current and drained its streams
    std::unique_ptr<T> take(uint64_t handle) {
        auto it = map_.find(handle);
        if (it == map_.end()) return nullptr;
        std::unique_ptr<T> obj = std::move(it->second);
        map_.erase(it);
        return obj;
    }
    // release hooks: f(object) for every live handle in ascending order, each object destroyed right after its call; the table is empty afterwards
    template <class F> void release_all(F f) {
        for (auto& kv : map_) {
            f(*kv.second);
            kv.second.reset();
        }
        map_.clear();
    }
    void release_all() { release_all([](T&) {}); }

  private:
    std::map<uint64_t, std::unique_ptr<T>> map_;
    uint64_t next_;
    const char* unknown_;
};

}  // namespace zk
