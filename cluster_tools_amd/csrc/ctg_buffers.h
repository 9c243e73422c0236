// Device buffers that own themselves, over dev_alloc / dev_free alone.  Plain
// C++17 -- no HIP -- so a host program runs their failure paths against a fake
// allocator (tools/pool_check.cpp, tests/test_pool.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

namespace ctg {

// the library's caching device allocator (ctg_pool.h, ctg_workspace.hip).
// dev_free only returns the block to the host-side pool: kernels already
// queued on the stream still use it, and a later user of the block runs after
// them ("stream-ordered reuse").  That holds for later users on the same
// stream only, and the pool knows nothing of streams: a block may be freed
// with work queued on it only inside a call that waits for its stream before
// it returns (the device lock keeps other streams' calls out until then).
// Every return path does: a scope that frees blocks with work queued on them
// holds a StreamWait below its buffers (include/ctg.h, "Streams").
void* dev_alloc(size_t bytes);
void dev_free(void* p);
// blocks until everything queued on the stream (a hipStream_t) is done
void stream_wait(void* stream);

// Waits for the stream when its scope ends.  Declared after every pool-drawing
// object of the scope (as a member: the last one), so it is destroyed first
// and every return path, a failed one included, waits before a block goes
// back to the pool.  disarm(): the success path has just waited itself.
// on = false with arm(): a scope that queues work only once a buffer exists.
struct StreamWait {
    void* stream;
    bool armed;
    explicit StreamWait(void* s, bool on = true) : stream(s), armed(on) {}
    StreamWait(const StreamWait&) = delete;
    ~StreamWait() {
        if (armed) stream_wait(stream);
    }
    void arm() { armed = true; }
    void disarm() { armed = false; }
};

// A block of the caching allocator that goes back to the pool when its scope
// ends (every early return included); reset() returns it sooner, release()
// hands it to a result.  Sizes are in bytes.
template <class T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    explicit DevBuf(size_t bytes) : p((T*)dev_alloc(bytes)) {}
    DevBuf(DevBuf&& o) noexcept : p(o.release()) {}   // (move-only: no copy is declared)
    ~DevBuf() { dev_free(p); }
    T* alloc(size_t bytes) { return reset((T*)dev_alloc(bytes)); }
    T* reset(T* q = nullptr) {
        dev_free(std::exchange(p, q));
        return p;
    }
    T* release() { return std::exchange(p, nullptr); }
    operator T*() const { return p; }
};

// A workspace buffer that grows to the largest request so far and lives until
// free() (ctg_trim).  A refused growth leaves it empty: null, 0 bytes.
struct GrowBuf {
    void* p = nullptr;
    size_t bytes = 0;
    void* reserve(size_t need) {
        if (need <= bytes && p) return p;
        const size_t n = std::max(need, bytes + bytes / 2);
        free();
        p = dev_alloc(n);
        bytes = p ? n : 0;
        return p;
    }
    void free() {
        dev_free(std::exchange(p, nullptr));
        bytes = 0;
    }
};

// Sort / reduce scratch of the record back half (ctg_records.hip): nine arrays
// of cap elements each.  All or nothing: cap > 0 exactly when all nine exist.
struct SortScratch {
    uint64_t *sk_in = nullptr, *sk_out = nullptr;     // sort keys in / out
    uint32_t *idx_in = nullptr, *idx_out = nullptr;   // record slots in / out
    uint64_t* uniq = nullptr;                         // run table: keys, lengths, offsets
    uint32_t *runs = nullptr, *offs = nullptr;
    uint32_t *keep = nullptr, *pos = nullptr;         // rows kept by the reduce, their output positions
    int64_t cap = 0;

    bool reserve(int64_t n) {
        if (n <= cap) return true;
        const int64_t c = std::max(n, cap + cap / 2);
        free();
        const bool ok = each([c](auto*& a) {
            a = static_cast<std::remove_reference_t<decltype(a)>>(dev_alloc((size_t)c * sizeof(*a)));
            return a != nullptr;
        });
        if (ok) cap = c;
        else free();
        return ok;
    }
    void free() {
        each([](auto*& a) {
            dev_free(std::exchange(a, nullptr));
            return true;
        });
        cap = 0;
    }

private:
    template <class F>   // f on every array, in allocation order, until one returns false
    bool each(F&& f) {
        return f(sk_in) && f(sk_out) && f(idx_in) && f(idx_out) && f(uniq) && f(runs) && f(offs) && f(keep) && f(pos);
    }
};

}  // namespace ctg
