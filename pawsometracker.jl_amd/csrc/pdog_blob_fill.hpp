// pdog_blob_fill.hpp — the row-word operations of the blob rule's region fill (include/pawsome_blob.h, step 5b), for the
// host and the device alike: no HIP header, nothing of the library.  dog_blob.hpp's two fills are made of these and of
// nothing else; tests/blob_fill_main.cpp holds them to a pixel flood fill under the host compiler and its sanitizers.
//
// A mask row is D <= 255 bits, bit x of word x / 64 for column x; the bits past D are 0.  One SWEEP replaces every row F_r of
// the reached set (F_r a subset of the mask row M_r) by
//      run_fill(M_r, M_r & (F_r | N)),   N = the rows above and below, for connectivity 8 also shifted by one bit each way
// — every candidate bit extended to the whole horizontal run of M_r it lies in —, all rows from the SAME old state.  A
// sweep never removes a bit, F stays inside the seed's component (a candidate is a mask pixel next to a reached one, and a
// run is connected), and a sweep that changes nothing has reached a fixed point, which is the whole component: a component
// pixel outside F with a neighbour in F would have been a candidate.  So the sweeps end after at most (pixels of the
// component) + 1 rounds.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDOG_BLOB_HD __host__ __device__ inline
#else
#define PDOG_BLOB_HD inline
#endif

namespace pdog {
namespace blobfill {

struct Row4 {
    uint64_t w[4];
};

PDOG_BLOB_HD uint64_t reverse64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bitreverse64(v);
#else
    v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
    v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
    v = ((v >> 4) & 0x0f0f0f0f0f0f0f0full) | ((v & 0x0f0f0f0f0f0f0f0full) << 4);
    v = ((v >> 8) & 0x00ff00ff00ff00ffull) | ((v & 0x00ff00ff00ff00ffull) << 8);
    v = ((v >> 16) & 0x0000ffff0000ffffull) | ((v & 0x0000ffff0000ffffull) << 16);
    return (v >> 32) | (v << 32);
#endif
}

// The bits of m from every bit of s (a subset of m) UPWARDS to the end of its run: the carry of m + s runs through the ones
// above a seed bit and clears them (a seed bit that receives a carry stays set), so they are the bits of m the sum lost, and s.
PDOG_BLOB_HD uint64_t fill_up1(uint64_t m, uint64_t s) { return (((m + s) ^ m) & m) | s; }

// run_fill for one word: every bit of s (a subset of m) extended to its whole run of m.
PDOG_BLOB_HD uint64_t run_fill1(uint64_t m, uint64_t s)
{
    return fill_up1(m, s) | reverse64(fill_up1(reverse64(m), reverse64(s)));
}

// the same upwards over four words, the carry handed from word to word
PDOG_BLOB_HD Row4 fill_up4(const Row4 &m, const Row4 &s)
{
    Row4 o;
    uint64_t carry = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const uint64_t a = m.w[k] + s.w[k];          // s is a subset of m: this overflows exactly when bit 63 of both is set
        const uint64_t x = a + carry;
        const uint64_t out = (uint64_t)(a < m.w[k]) | (uint64_t)(x < a);
        o.w[k] = ((x ^ m.w[k]) & m.w[k]) | s.w[k];
        // a carry INTO bit 0 of a word whose bit 0 is a mask bit without a seed clears it in x: the xor above reports it
        // like every other bit the carry ran through
        carry = out;
    }
    return o;
}

PDOG_BLOB_HD Row4 reverse4(const Row4 &v)
{
    Row4 o;
    o.w[0] = reverse64(v.w[3]);
    o.w[1] = reverse64(v.w[2]);
    o.w[2] = reverse64(v.w[1]);
    o.w[3] = reverse64(v.w[0]);
    return o;
}

// run_fill for four words (a row of up to 256 bits)
PDOG_BLOB_HD Row4 run_fill4(const Row4 &m, const Row4 &s)
{
    const Row4 up = fill_up4(m, s), dn = reverse4(fill_up4(reverse4(m), reverse4(s)));
    Row4 o;
    for (int k = 0; k < 4; ++k) o.w[k] = up.w[k] | dn.w[k];
    return o;
}

// The candidates of a row of one word: the mask bits that are reached already or have a reached neighbour in the row above
// (up) or below (dn).  The horizontal neighbours need no term: run_fill extends a reached bit along its run anyway.
PDOG_BLOB_HD uint64_t candidates1(uint64_t m, uint64_t f, uint64_t up, uint64_t dn, bool eight)
{
    uint64_t n = up | dn;
    if (eight) n |= (n << 1) | (n >> 1);
    return m & (f | n);
}

PDOG_BLOB_HD Row4 candidates4(const Row4 &m, const Row4 &f, const Row4 &up, const Row4 &dn, bool eight)
{
    Row4 n, o;
    for (int k = 0; k < 4; ++k) n.w[k] = up.w[k] | dn.w[k];
    for (int k = 0; k < 4; ++k) {
        uint64_t v = n.w[k];
        if (eight) {
            v |= (n.w[k] << 1) | (k > 0 ? n.w[k - 1] >> 63 : 0);
            v |= (n.w[k] >> 1) | (k < 3 ? n.w[k + 1] << 63 : 0);
        }
        o.w[k] = m.w[k] & (f.w[k] | v);
    }
    return o;
}

// one row of one sweep
PDOG_BLOB_HD uint64_t sweep_row1(uint64_t m, uint64_t f, uint64_t up, uint64_t dn, bool eight)
{
    return run_fill1(m, candidates1(m, f, up, dn, eight));
}

PDOG_BLOB_HD Row4 sweep_row4(const Row4 &m, const Row4 &f, const Row4 &up, const Row4 &dn, bool eight)
{
    return run_fill4(m, candidates4(m, f, up, dn, eight));
}

PDOG_BLOB_HD bool differ4(const Row4 &a, const Row4 &b)
{
    return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3])) != 0;
}

} // namespace blobfill
} // namespace pdog
