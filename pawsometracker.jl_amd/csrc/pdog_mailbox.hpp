// pdog_mailbox.hpp — the tracker's mailbox: one pinned, host-coherent, device-mapped block that the host and the kernels both
// read and write without a copy command.  Plain C++, shared by the kernels (dog_kernels.hpp) and the host (pawsome_dog.hip,
// tests/policy_main.cpp); every access to the block goes through these names.
#pragma once
#include <stdint.h>

namespace pdog {

// What kernels raise or publish while they run (ExactCtl::range_err points here), all with relaxed system-scope stores.
struct KernelWords {
    // 1: a device-resident guess lay where the reference raises BoundsError (src/PawsomeTracker.jl:45-46; range_check);
    // 2: a device-side wait between resident workgroups gave up (wait_counter).  Every entry point that drains the stream
    // reads and clears it (drain_and_check).
    int32_t raised;
    // The finishing kernel, once per batch: windows flagged for refinement so far, out of how many windows finished so far
    // (the low 32 bits of cumulative counts; MapPolicy, pdog_policy.hpp, takes differences).  TWO stores, read by the host
    // with TWO loads, where the pre-pass deliberately publishes one 64-bit word: the pair can be seen torn, across batches
    // (one batch's `flagged` beside another's `finished`).  The policy's estimate of a rate is then off by one batch.
    uint32_t flagged;
    uint32_t finished;
};

struct Mailbox {
    // the host functor (pdog_detect_host): the window's guess as the host writes it, the kernels' answer, and the completion
    // ticket that the single-window kernels publish right after the answer (system-scope release); the host polls for it
    int32_t guess[2];
    int32_t result[2];
    int32_t ticket;
    KernelWords kernel;
    // the pre-pass (dog_prune.hpp), once per batch and in ONE 64-bit store, so never torn: kept (low half) and total (high
    // half) (slot, sub-chunk) pairs so far, the low 32 bits of each (PrunePolicy, pdog_policy.hpp)
    uint64_t prune_pub;
};

static_assert(sizeof(Mailbox) == 40 && alignof(Mailbox) == 8, "the mailbox is ten 32-bit words, 8-byte aligned for prune_pub");
static_assert(__builtin_offsetof(Mailbox, guess) == 0 && __builtin_offsetof(Mailbox, result) == 8 && __builtin_offsetof(Mailbox, ticket) == 16 &&
                  __builtin_offsetof(Mailbox, kernel) == 20 && __builtin_offsetof(Mailbox, prune_pub) == 32,
              "mailbox layout");
static_assert(sizeof(KernelWords) == 12 && __builtin_offsetof(KernelWords, flagged) == 4 && __builtin_offsetof(KernelWords, finished) == 8, "the kernels' words");

} // namespace pdog
