// The sparse assignment of ctg_take.hip (nt.takeDict): an open-addressing hash
// table of (key, value) uint64 pairs with linear probing.  Hash, insert and
// lookup are written once, for the device and for the host: plain C++17 with
// the HIP qualifiers only where hipcc compiles it, so a host program runs the
// same code on the CPU (tools/take_check.cpp, tests/test_take_host.py).
//
// Layout: 2 * cap + 2 words.  Slot h is words (2h, 2h + 1) = (key, value); a
// free slot's key is TAKE_FREE.  The one key that equals TAKE_FREE lives in the
// two side words behind the slots (the tile tables' empty-key escape): word
// 2 cap counts its inserts, word 2 cap + 1 holds its value.  cap is a power of
// two of at least 2 n (ctg_plan.h: take_capacity), so a probe sequence always
// meets a free slot.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define CTG_HD __host__ __device__
#else
#define CTG_HD
#endif

namespace ctg {

constexpr uint64_t TAKE_FREE = ~0ull;

// murmur3's 64-bit finaliser: every input bit reaches the low bits the mask keeps
CTG_HD inline uint64_t take_hash(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// words of a table of `cap` slots, side words included
CTG_HD inline uint64_t take_table_words(uint64_t cap) { return 2 * cap + 2; }

// (key, value) into the table.  cas(p, expected, desired) returns what *p held
// (atomicCAS on the device, a plain compare and store on the host); add(p)
// returns *p and adds 1 to it.  Returns 0, or 1 for a key that is there already
// (the table keeps the first value).
template <class Cas, class Add>
CTG_HD inline int take_insert(uint64_t* t, uint64_t cap, uint64_t key, uint64_t value, Cas&& cas, Add&& add) {
    if (key == TAKE_FREE) {
        if (add(&t[2 * cap]) != 0) return 1;
        t[2 * cap + 1] = value;
        return 0;
    }
    uint64_t h = take_hash(key) & (cap - 1);
    for (;;) {
        uint64_t cur = t[2 * h];
        if (cur == TAKE_FREE) cur = cas(&t[2 * h], TAKE_FREE, key);
        if (cur == TAKE_FREE) {
            t[2 * h + 1] = value;
            return 0;
        }
        if (cur == key) return 1;
        h = (h + 1) & (cap - 1);
    }
}

// the value of key into *value; false where the table does not hold it
CTG_HD inline bool take_lookup(const uint64_t* t, uint64_t cap, uint64_t key, uint64_t* value) {
    if (key == TAKE_FREE) {
        if (t[2 * cap] == 0) return false;
        *value = t[2 * cap + 1];
        return true;
    }
    uint64_t h = take_hash(key) & (cap - 1);
    for (;;) {
        const uint64_t cur = t[2 * h], val = t[2 * h + 1];   // (one 16-byte load)
        if (cur == key) {
            *value = val;
            return true;
        }
        if (cur == TAKE_FREE) return false;
        h = (h + 1) & (cap - 1);
    }
}

}  // namespace ctg
