// rt_ring_level.h — the fill level of the PRETRACE variant's ring (rt_trace_pool_kernel.hip: pretrace_batch and the
// hand-out) and the rule that says when a camera batch is due.  Integer arithmetic on values that are the same in all
// 64 lanes: on the device it belongs to the scalar unit, which every wave of a CU queues for, and it runs in every
// path-loop iteration.  So the level is a COUNTER — a batch adds the entries it queues, the hand-out subtracts what it
// takes — and "a batch is due" is one comparison of that counter with a threshold which the item's last batch puts out
// of reach.  Plain C++17: the host compiles it too (tests/ring_level_driver.cpp, which holds both rules to the
// expressions they replace).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_RING_FN __host__ __device__ inline
#else
#define RT_RING_FN inline
#endif

namespace rt_ring {

enum : uint32_t { BATCH = 64u }; // entries a camera batch draws, and the free slots it needs behind the ring's entries

// ---- the counter rule
// The level a batch leaves: its `lives` entries queue up behind the ring's (the others ended in the batch).
RT_RING_FN uint32_t after_batch(uint32_t level, uint32_t lives) { return level + lives; }
// What a hand-out takes with `idle` lanes free, and the level it leaves.
RT_RING_FN uint32_t taken(uint32_t idle, uint32_t level) { return idle < level ? idle : level; }
RT_RING_FN uint32_t after_hand_out(uint32_t level, uint32_t n_take) { return level - n_take; }
// Slot `offset` behind `head`, head < slots and offset <= slots: one conditional subtraction.
RT_RING_FN uint32_t slot_at(uint32_t head, uint32_t offset, uint32_t slots) {
    const uint32_t s = head + offset;
    return s >= slots ? s - slots : s;
}

// ---- the batch rule: a batch runs while the item has one left and at most slots - BATCH entries wait, i.e. with BATCH
// free slots behind them.  As ONE comparison: level < batch_below, where batch_below is slots - BATCH + 1 while batches
// are left and 0 — below every level — from the item's last batch on (and for an item without a pixel).  A batch is
// left while the batches drawn so far cover fewer entries than the pool has (`drawn` = batches_done * BATCH, which the
// next batch needs anyway as its first entry; with n_batches = ceil(total / BATCH) that is batches_done < n_batches).
RT_RING_FN uint32_t batch_below_of(uint32_t drawn, uint32_t total, uint32_t slots) {
    return drawn < total ? slots - BATCH + 1u : 0u;
}
RT_RING_FN bool batch_is_due(uint32_t level, uint32_t batch_below) { return level < batch_below; }
// Every batch drawn and the ring empty: each entry of the pool has ended in its batch or been handed out (what
// `next >= total` says of the pool's index).
RT_RING_FN bool pool_is_dry(uint32_t level, uint32_t batch_below) { return (level | batch_below) == 0u; }

// ---- the expressions both rules replace (the kernel no longer runs them; the host test does, beside the rules above):
// the level re-formed from the pool's index `next` — entries ended or handed out — and the count of batches drawn
RT_RING_FN uint32_t level_recomputed(uint32_t batches_done, uint32_t total, uint32_t next) {
    const uint32_t drawn = batches_done << 6;
    return (drawn < total ? drawn : total) - next;
}
RT_RING_FN bool batch_is_due_recomputed(uint32_t batches_done, uint32_t n_batches, uint32_t total, uint32_t next, uint32_t slots) {
    return batches_done < n_batches && level_recomputed(batches_done, total, next) <= slots - BATCH;
}

} // namespace rt_ring
