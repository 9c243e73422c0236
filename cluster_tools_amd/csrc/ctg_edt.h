// The exact Euclidean distance transform (include/ctg.h: ctg_distance_transform):
// what the kernels of ctg_edt.hip and a host program share (tools/edt_check.cpp
// renders the three passes serially with these functions, as tools/cc_check.cpp
// does with ctg_uf.h).  Plain C++17 -- no HIP.
//
// The passes carry integer index offsets to the chosen seed, never rounded
// distances: the x pass writes |dx| (u16), the y pass (|dy|, |dx|) (two u16 in
// a u32), and the last pass evaluates edt_d2 on the final triple.  The written
// value is then a pure function of the chosen seed.
#pragma once
#include <cmath>
#include <cstdint>

#include "ctg_plan.h"

namespace ctg {

constexpr uint32_t EDT_NONE16 = 0xFFFFu;        // x pass: no seed in the row
constexpr uint32_t EDT_NONE32 = 0xFFFFFFFFu;    // y pass: no seed in the slice

// D2 of the offset (dz, dy, dx) under the pitch p (z, y, x): float64, the
// three squares added in this order, no contraction (-ffp-contract=off)
CTG_HD inline double edt_d2(uint32_t dz, uint32_t dy, uint32_t dx, const double* p) {
    const double a = (double)dz * p[0], b = (double)dy * p[1], c = (double)dx * p[2];
    return a * a + b * b + c * c;
}
// the square of the domain's diagonal: what a voxel without a seed in its
// domain (the box; in 2-D mode the slice, so no z term) gets
CTG_HD inline double edt_diag2(const int64_t* n, const double* p, bool two_d) {
    const double a = two_d ? 0.0 : (double)n[0] * p[0], b = (double)n[1] * p[1], c = (double)n[2] * p[2];
    return a * a + b * b + c * c;
}

// ---------------------------------------------------------------------------
// x pass: the row's seeds as 64-bit words (bit b of word w: voxel 64 w + b; no
// bit past the row's end) and, over them, one bit per nonzero word (`sup`,
// EDT_ROW_SUPER words).  The nearest seed at or before / at or after x is two
// count-leading / count-trailing-zero steps, and a walk over the at most
// EDT_ROW_SUPER top words where a gap is longer than 4096 voxels.
// ---------------------------------------------------------------------------
CTG_HD inline int edt_prev_seed(const uint64_t* words, const uint64_t* sup, int x) {
    const int w = x >> 6;
    const uint64_t m = words[w] & (~0ull >> (63 - (x & 63)));
    if (m) return (w << 6) + 63 - __builtin_clzll(m);
    int sw = w >> 6;
    uint64_t sm = (w & 63) ? (sup[sw] & ((1ull << (w & 63)) - 1ull)) : 0ull;
    while (!sm) {
        if (sw == 0) return -1;
        sm = sup[--sw];
    }
    const int ww = (sw << 6) + 63 - __builtin_clzll(sm);
    return (ww << 6) + 63 - __builtin_clzll(words[ww]);
}
// n_sup: the top words of the row ((words + 63) / 64)
CTG_HD inline int edt_next_seed(const uint64_t* words, const uint64_t* sup, int n_sup, int x) {
    const int w = x >> 6;
    const uint64_t m = words[w] & (~0ull << (x & 63));
    if (m) return (w << 6) + __builtin_ctzll(m);
    int sw = w >> 6;
    uint64_t sm = (w & 63) == 63 ? 0ull : (sup[sw] & (~0ull << ((w & 63) + 1)));
    while (!sm) {
        if (++sw >= n_sup) return -1;
        sm = sup[sw];
    }
    const int ww = (sw << 6) + __builtin_ctzll(sm);
    return (ww << 6) + __builtin_ctzll(words[ww]);
}
// |dx| to the nearest seed of the row, or EDT_NONE16
CTG_HD inline uint32_t edt_row_distance(const uint64_t* words, const uint64_t* sup, int n_sup, int x) {
    const int l = edt_prev_seed(words, sup, x), r = edt_next_seed(words, sup, n_sup, x);
    if (l < 0) return r < 0 ? EDT_NONE16 : (uint32_t)(r - x);
    return r < 0 || x - l <= r - x ? (uint32_t)(x - l) : (uint32_t)(r - x);
}

// ---------------------------------------------------------------------------
// y and z pass: the lower envelope of the parabolas F_q(t) = f(q) + w (t - q)^2
// over the line's integer positions t in [0, n), w the square of the line
// axis' pitch, f(q) the squared distance the earlier passes found at q
// (Felzenszwalb & Huttenlocher 2012; Meijster et al. 2000 for the integer
// starts).  One stack entry per parabola on the envelope, 8 bytes: the line
// index q, the first integer position `start` at which it is the minimum, and
// the two offsets (a, b) = (|dy|, |dx|) it carries (a is 0 in the y pass), so
// no pass reads its input twice.
// ---------------------------------------------------------------------------
typedef uint64_t EdtEntry;
CTG_HD inline EdtEntry edt_entry(uint32_t q, uint32_t start, uint32_t a, uint32_t b) {
    return (uint64_t)q | ((uint64_t)start << 16) | ((uint64_t)a << 32) | ((uint64_t)b << 48);
}
CTG_HD inline uint32_t edt_q(EdtEntry e) { return (uint32_t)e & 0xFFFFu; }
CTG_HD inline uint32_t edt_start(EdtEntry e) { return (uint32_t)(e >> 16) & 0xFFFFu; }
CTG_HD inline uint32_t edt_a(EdtEntry e) { return (uint32_t)(e >> 32) & 0xFFFFu; }
CTG_HD inline uint32_t edt_b(EdtEntry e) { return (uint32_t)(e >> 48); }

struct EdtAxis {
    double pa, pb;   // the pitches of the offsets a and b
    double w;        // the line axis' pitch, squared
    int n;           // the line's length
};
// f(q) of the offsets (a, b), and f(q) + w q^2
CTG_HD inline double edt_f(uint32_t a, uint32_t b, const EdtAxis& A) {
    const double u = (double)a * A.pa, v = (double)b * A.pb;
    return u * u + v * v;
}
CTG_HD inline double edt_height(uint32_t q, uint32_t a, uint32_t b, const EdtAxis& A) {
    return edt_f(a, b, A) + A.w * ((double)q * (double)q);
}
// F_q(t) of the parabola at q with f(q) = f
CTG_HD inline double edt_at(uint32_t q, double f, uint32_t t, const EdtAxis& A) {
    const double d = (double)t - (double)q;
    return f + A.w * (d * d);
}
// The first integer position in [0, n] from which the parabola at q (height
// hq) lies strictly below the one of entry e, q > edt_q(e); n: nowhere on the
// line.  F_q(t) < F_v(t) exactly where t > s, s = (hq - hv) / (2 w (q - v)).
//
// Why the floor is right: with integer pitches hq, hv and the denominator are
// integers, exact in float64 while they stay below 2^53.  The quotient is then
// either an integer, and the division returns it exactly, or it lies at least
// 1 / (2 w (q - v)) >= 1 / (2 w n) from every integer.  Only quotients in
// [0, n) decide anything (the others are clamped), and the division's rounding
// moves those by less than n 2^-53 -- far less than that gap while
// 2 w n^2 < 2^53.  So floor(s) is the true floor and the pass picks a true
// nearest seed.  With other pitches a near-tie may fall to either parabola,
// whose D2 then differ by a few units of 2^-53 relative.
CTG_HD inline int edt_takeover(EdtEntry e, uint32_t q, double hq, const EdtAxis& A) {
    const uint32_t v = edt_q(e);
    const double s = (hq - edt_height(v, edt_a(e), edt_b(e), A)) / (2.0 * A.w * (double)(q - v));
    if (s < 0.0) return 0;
    if (!(s < (double)A.n)) return A.n;
    return (int)s + 1;   // (s >= 0: the cast is the floor)
}
// Push the parabola of position q (offsets a, b) onto the stack S (S.get(k),
// S.set(k, e)) whose top entry k is mirrored in `top`; k = -1: empty.  Entries
// the new parabola hides at every integer position are popped first: the top
// entry goes where the new parabola is strictly below it at the entry's own
// start already (the takeover is then at or before that start) -- two
// evaluations, exact with integer pitches, and no division; the one division
// of a push finds the start of the entry that stays.
template <class Stack>
CTG_HD inline void edt_push(Stack& S, int& k, EdtEntry& top, uint32_t q, uint32_t a, uint32_t b, const EdtAxis& A) {
    const double fq = edt_f(a, b, A);
    while (k >= 0) {
        const uint32_t t = edt_start(top);
        if (!(edt_at(q, fq, t, A) < edt_at(edt_q(top), edt_f(edt_a(top), edt_b(top), A), t, A))) break;
        if (--k >= 0) top = S.get(k);
    }
    uint32_t st = 0;
    if (k >= 0) {
        // (past the top's start in exact arithmetic; the maximum keeps the starts ascending under rounding too)
        st = (uint32_t)edt_takeover(top, q, fq + A.w * ((double)q * (double)q), A);
        if (st <= edt_start(top)) st = edt_start(top) + 1;
        if (st >= (uint32_t)A.n) return;   // never the minimum on the line
    }
    top = edt_entry(q, st, a, b);
    S.set(++k, top);
}
// The entry that holds position t, walking up from entry j (cur = S.get(j),
// nxt = edt_next(S, k, j)); t visits 0 .. n-1 in order.  Starts ascend
// strictly, so at most one step.
constexpr EdtEntry EDT_NO_ENTRY = (EdtEntry)0xFFFFu << 16;   // a start no position reaches
template <class Stack>
CTG_HD inline EdtEntry edt_next(const Stack& S, int k, int j) {
    return j < k ? S.get(j + 1) : EDT_NO_ENTRY;
}
template <class Stack>
CTG_HD inline void edt_seek(const Stack& S, int k, int& j, EdtEntry& cur, EdtEntry& nxt, uint32_t t) {
    while (edt_start(nxt) <= t) {
        cur = nxt;
        nxt = edt_next(S, k, ++j);
    }
}

}  // namespace ctg
