// The caching device allocator of libctg.so over a raw allocate / free back
// end.  Plain C++17 -- no HIP: ctg_workspace.hip passes hipMalloc / hipFree, a
// host program passes a fake that refuses on demand, so the size classes and
// every failure path run under sanitizers without a GPU (tools/pool_check.cpp,
// tests/test_pool.py).
#pragma once
#include <cstddef>
#include <map>
#include <mutex>

namespace ctg {

// size classes: 256 B doubling to 1 MiB, then x1.25 (idempotent)
inline size_t pool_round_up(size_t b) {
    size_t r = 256;
    while (r < b) r = r < (1u << 20) ? r * 2 : r + (r >> 2);
    return r;
}

// Results and scratch are recycled between calls, so steady-state calls reach
// the back end for nothing: free() only files the block under the device that
// allocated it, alloc() takes a cached block of the request's class up to
// twice its size.  The back end's functions return 0 for success.
class DevicePool {
public:
    static constexpr int MAX_DEVICES = 64;
    static constexpr size_t SLACK = 64;   // bytes past the class size of every raw allocation
    using RawAlloc = int (*)(void** p, size_t bytes);
    using RawFree = int (*)(void* p);
    DevicePool(RawAlloc a, RawFree f) : raw_alloc_(a), raw_free_(f) {}

    // null: the back end refused, and refused again after a purge of the device's cached blocks
    void* alloc(int device, size_t bytes) {
        bytes = pool_round_up(bytes);
        std::unique_lock<std::mutex> g(mu_);
        auto& cache = cache_[device & (MAX_DEVICES - 1)];
        auto it = cache.lower_bound(bytes);
        if (it != cache.end() && it->first <= bytes * 2) {
            void* p = it->second;
            cache.erase(it);
            return p;
        }
        g.unlock();   // other threads keep recycling while the back end works
        void* p = nullptr;
        const int rc = raw_alloc_(&p, bytes + SLACK);
        g.lock();
        if (rc != 0) {
            purge_locked(device);
            if (raw_alloc_(&p, bytes + SLACK) != 0) return nullptr;
        }
        blocks_[p] = Block{bytes, device & (MAX_DEVICES - 1)};
        return p;
    }

    // back to the pool (a pointer that is not a block of this pool is ignored)
    void free(void* p) {
        if (!p) return;
        std::lock_guard<std::mutex> g(mu_);
        auto it = blocks_.find(p);
        if (it != blocks_.end()) cache_[it->second.device].emplace(it->second.bytes, p);
    }

    // hand the device's cached blocks to the back end; a block leaves the pool
    // as it is freed, one whose free fails stays cached.  The first failure's
    // status, or 0.
    int purge(int device) {
        std::lock_guard<std::mutex> g(mu_);
        return purge_locked(device);
    }

    template <class F>   // f(bytes, pointer) for every cached block of the device
    void for_each_cached(int device, F&& f) {
        std::lock_guard<std::mutex> g(mu_);
        for (auto& kv : cache_[device & (MAX_DEVICES - 1)]) f(kv.first, kv.second);
    }

private:
    struct Block {
        size_t bytes;   // class size
        int device;
    };
    int purge_locked(int device) {
        auto& cache = cache_[device & (MAX_DEVICES - 1)];
        int first = 0;
        for (auto it = cache.begin(); it != cache.end();) {
            const int rc = raw_free_(it->second);
            if (rc != 0) {
                if (!first) first = rc;
                ++it;
                continue;
            }
            blocks_.erase(it->second);
            it = cache.erase(it);
        }
        return first;
    }
    RawAlloc raw_alloc_;
    RawFree raw_free_;
    std::mutex mu_;
    std::multimap<size_t, void*> cache_[MAX_DEVICES];
    std::map<void*, Block> blocks_;   // every block the back end holds for us, handed out or cached
};

}  // namespace ctg
