// dog_prune_publish.hpp — the word through which the workgroups of one pre-pass launch (dog_prune.hpp) meet, free of HIP so
// that a host program can run the arrivals in any order (tests/prune_publish_main.cpp).
//
// stat[2] of the tracker's counters is zero when a batch starts.  Every workgroup adds ONE increment to it, once, with a
// returning atomic, and the word holds three running sums side by side:
//     bits  0 … 19   workgroups that have arrived
//     bits 20 … 39   jobs (kept strips) they have appended to the list
//     bits 40 … 63   (slot, sub-chunk) pairs they have kept
// What the add returns is the state before this workgroup: its job field is the place of the window's entries in the list,
// and the workgroup whose arrival field reads n − 1 is the last one.  The returned fields plus its own contribution are the
// batch's sums: the last arriver needs to read nobody else's memory.
//
// FIT.  No field may carry into its neighbour, at any moment of the batch.  The sums only grow, so the final values decide:
// n arrivals, at most n · nstrips jobs, at most n · nslots · nsub pairs.  pp_fits asks each to lie below its field's range;
// a batch that does not fit is published the older way (LaunchGeo::prune, PRUNE_FENCED_PUBLISH).  cfg3 (4096 windows, 4
// strips, 5 slots, 41 sub-chunks) needs 13, 15 and 20 bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PP_HD __host__ __device__ inline
#else
#define PP_HD inline
#endif

namespace pdog {

constexpr int PP_ARRIVAL_BITS = 20, PP_JOB_BITS = 20, PP_KEPT_BITS = 24;
static_assert(PP_ARRIVAL_BITS + PP_JOB_BITS + PP_KEPT_BITS == 64, "the three fields fill the word");
constexpr int PP_JOB_SHIFT = PP_ARRIVAL_BITS, PP_KEPT_SHIFT = PP_ARRIVAL_BITS + PP_JOB_BITS;

PP_HD uint64_t pp_pack(uint64_t arrivals, uint64_t jobs, uint64_t kept) { return arrivals | (jobs << PP_JOB_SHIFT) | (kept << PP_KEPT_SHIFT); }
PP_HD uint32_t pp_arrivals(uint64_t w) { return (uint32_t)(w & ((1ull << PP_ARRIVAL_BITS) - 1)); }
PP_HD uint32_t pp_jobs(uint64_t w) { return (uint32_t)((w >> PP_JOB_SHIFT) & ((1ull << PP_JOB_BITS) - 1)); }
PP_HD uint32_t pp_kept(uint64_t w) { return (uint32_t)(w >> PP_KEPT_SHIFT); }

// what one workgroup adds: itself, its window's jobs, its window's kept pairs
PP_HD uint64_t pp_increment(uint32_t njobs, uint32_t kept) { return pp_pack(1u, njobs, kept); }

// true: a batch of n windows of this geometry can be counted in the packed word
PP_HD bool pp_fits(long long n, long long nstrips, long long nslots, long long nsub)
{
    return n > 0 && n < (1ll << PP_ARRIVAL_BITS) && n * nstrips < (1ll << PP_JOB_BITS) && n * nslots * nsub < (1ll << PP_KEPT_BITS);
}

// What a workgroup learns from the word its add returned.  base: the list position of its first entry.  last: it is the
// batch's last arriver, and then jobs / kept are the sums over the whole batch.
struct PpArrival {
    uint32_t base;
    bool last;
    uint32_t jobs, kept;
};
PP_HD PpArrival pp_arrive(uint64_t returned, uint32_t njobs, uint32_t kept, uint32_t n)
{
    return PpArrival{pp_jobs(returned), pp_arrivals(returned) == n - 1u, pp_jobs(returned) + njobs, pp_kept(returned) + kept};
}

// Mailbox::prune_pub from the cumulative counts: the low half of the kept pairs, the total pairs above it
PP_HD uint64_t pp_host_word(uint64_t kept_cum, uint64_t total_cum) { return (kept_cum & 0xffffffffull) | (total_cum << 32); }

} // namespace pdog
