// ring_level_driver.cpp — a model of the PRETRACE item loop of rt_trace_pool_kernel.hip, run over seeded items with both
// statements of the ring's bookkeeping side by side (racer-tracer_amd/csrc/rt_ring_level.h):
//   * the RECOMPUTED level, min(batches_done << 6, total) - next, with `next` kept up by every batch and every hand-out,
//     and the two-part test in front of a batch (what the kernel ran before), and
//   * the COUNTER and the one comparison with batch_below (what it runs now).
// An item: `total` pool entries in batches of 64; a batch queues `lives` of its entries behind the ring's and ends the
// others; the hand-out gives min(idle lanes, level) entries to lanes; lanes end at random; the loop is left when no lane
// has a path after a hand-out.  At every step: equal levels, equal slots, equal batch decisions, equal "the pool is dry",
// never more than `slots` entries, no slot written while it holds an entry, entries handed out in pool order; at the end
// of the item next == total.  Any difference prints a line and ends the program with status 1.
//
//   ring_level_driver <slots> <items> <seed>     prints one summary line
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rt_ring_level.h"

namespace {

struct Rng { // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return n == 0 ? 0u : (uint32_t)(next() % n); }
};

struct Tally {
    uint64_t items = 0, batches = 0, hand_outs = 0, wraps = 0, empty_batches = 0, full_batches = 0, one_batch_items = 0,
             short_items = 0, ragged_items = 0, full_ring = 0, most_wraps = 0, steps = 0;
};

[[noreturn]] void fail(const char *what, uint64_t item, uint32_t total, uint32_t a, uint32_t b) {
    printf("MISMATCH %s: item %llu total %u: %u vs %u\n", what, (unsigned long long)item, total, a, b);
    exit(1);
}

// how a batch's `lives` are drawn: 0 none (a depth limit of 0 or 1, a camera outside that sees nothing), 1 all (the camera
// inside the box), 2 uniform, 3 mostly ending, 4 each batch all or none
uint32_t draw_lives(Rng &rng, int mode, uint32_t in_pool) {
    switch (mode) {
    case 0: return 0u;
    case 1: return in_pool;
    case 2: return rng.below(in_pool + 1u);
    case 3: return rng.below(4u) == 0u ? rng.below(in_pool + 1u) : rng.below(in_pool / 8u + 1u);
    default: return rng.below(2u) ? in_pool : 0u;
    }
}

void run_item(Rng &rng, uint32_t slots, uint32_t total, int mode, uint32_t end_one_in, uint64_t item, Tally &t) {
    const uint32_t n_batches = (total + 63u) >> 6;
    // the statement the kernel ran before
    uint32_t next = 0, batches_done = 0, head_old = 0;
    // the statement it runs now (batches_done is shared: the batch needs it for its first entry)
    uint32_t level = 0, head_new = 0, batch_below = rt_ring::batch_below_of(0u, total, slots);
    std::vector<int64_t> ring(slots, -1); // the pool entry a slot holds
    uint32_t held = 0, alive = 0, handed = 0;
    uint64_t wraps = 0;
    uint32_t next_to_queue = 0; // (pool order: entries enter the ring with rising index and leave it the same way)
    int64_t last_out = -1;
    for (;;) {
        ++t.steps;
        for (;;) {
            const uint32_t level_old = rt_ring::level_recomputed(batches_done, total, next);
            if (level_old != level) fail("level in front of a batch", item, total, level_old, level);
            const bool due_old = rt_ring::batch_is_due_recomputed(batches_done, n_batches, total, next, slots);
            const bool due_new = rt_ring::batch_is_due(level, batch_below);
            if (due_old != due_new) fail("batch decision", item, total, due_old, due_new);
            if (!due_new) break;
            if (level + rt_ring::BATCH > slots) fail("a batch without 64 free slots", item, total, level, slots);
            // ---- batch b
            const uint32_t b = batches_done++;
            const uint32_t in_pool = total - b * 64u < 64u ? total - b * 64u : 64u;
            const uint32_t lives = draw_lives(rng, mode, in_pool);
            t.empty_batches += lives == 0u;
            t.full_batches += lives == 64u;
            ++t.batches;
            const uint32_t in_ring_old = rt_ring::level_recomputed(b, total, next); // (what the batch formed: its own b)
            const uint32_t in_ring_new = level;
            if (in_ring_old != in_ring_new) fail("level inside a batch", item, total, in_ring_old, in_ring_new);
            for (uint32_t rank = 0; rank < lives; ++rank) {
                uint32_t slot_old = head_old + in_ring_old + rank;
                if (slot_old >= slots) slot_old -= slots;
                const uint32_t slot_new = rt_ring::slot_at(head_new, in_ring_new + rank, slots);
                if (slot_old != slot_new) fail("slot of a batch entry", item, total, slot_old, slot_new);
                if (slot_new >= slots) fail("slot out of the ring", item, total, slot_new, slots);
                if (ring[slot_new] >= 0) fail("slot written while it holds an entry", item, total, slot_new, (uint32_t)ring[slot_new]);
                ring[slot_new] = (int64_t)(b * 64u + rank); // (which of the batch's entries live does not matter here)
                ++held;
            }
            next_to_queue = b * 64u + in_pool;
            next += in_pool - lives; // the entries that ended in the batch
            level = rt_ring::after_batch(in_ring_new, lives);
            batch_below = rt_ring::batch_below_of(batches_done << 6, total, slots);
            if (held != level) fail("entries held", item, total, held, level);
            if (level > slots) fail("more entries than slots", item, total, level, slots);
            t.full_ring += level == slots;
        }
        // ---- hand-out
        {
            const uint32_t in_ring_old = rt_ring::level_recomputed(batches_done, total, next);
            if (in_ring_old != level) fail("level at the hand-out", item, total, in_ring_old, level);
            if (level != 0u) {
                const uint32_t idle = 64u - alive;
                const uint32_t take_old = idle < in_ring_old ? idle : in_ring_old;
                const uint32_t take_new = rt_ring::taken(idle, level);
                if (take_old != take_new) fail("entries taken", item, total, take_old, take_new);
                for (uint32_t r = 0; r < take_new; ++r) {
                    uint32_t slot_old = head_old + r;
                    if (slot_old >= slots) slot_old -= slots;
                    const uint32_t slot_new = rt_ring::slot_at(head_new, r, slots);
                    if (slot_old != slot_new) fail("slot of a hand-out", item, total, slot_old, slot_new);
                    if (ring[slot_new] < 0) fail("empty slot handed out", item, total, slot_new, 0u);
                    if (ring[slot_new] <= last_out) fail("entries out of pool order", item, total, (uint32_t)ring[slot_new], (uint32_t)last_out);
                    last_out = ring[slot_new];
                    ring[slot_new] = -1;
                    --held;
                }
                next += take_old;
                head_old += take_old;
                if (head_old >= slots) head_old -= slots, ++wraps;
                level = rt_ring::after_hand_out(level, take_new);
                head_new = rt_ring::slot_at(head_new, take_new, slots);
                if (head_old != head_new) fail("ring head", item, total, head_old, head_new);
                alive += take_new;
                handed += take_new;
                t.hand_outs += take_new != 0u;
            }
        }
        const bool dry_old = next >= total, dry_new = rt_ring::pool_is_dry(level, batch_below);
        if (dry_old != dry_new) fail("the pool is dry", item, total, dry_old, dry_new);
        if (alive == 0u) break;
        // ---- some of the lanes' paths end
        uint32_t ending = 0;
        for (uint32_t l = 0; l < alive; ++l) ending += rng.below(end_one_in) == 0u;
        alive -= ending;
    }
    // the loop's only exit: every batch drawn, the ring empty — the pool is dry, and the new statement sets next = total
    if (batches_done != n_batches) fail("batches drawn at the exit", item, total, batches_done, n_batches);
    if (level != 0u || held != 0u) fail("entries left at the exit", item, total, level, held);
    if (batch_below != 0u) fail("batch_below at the exit", item, total, batch_below, 0u);
    if (next != total) fail("next at the exit", item, total, next, total);
    if (next_to_queue != total && total != 0u) fail("entries drawn", item, total, next_to_queue, total);
    if (handed > total) fail("more hand-outs than entries", item, total, handed, total);
    ++t.items;
    t.wraps += wraps;
    if (wraps > t.most_wraps) t.most_wraps = wraps;
    t.one_batch_items += n_batches == 1u;
    t.short_items += total < 64u;
    t.ragged_items += (total & 63u) != 0u;
}

} // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: ring_level_driver <slots> <items> <seed>\n");
        return 2;
    }
    const uint32_t slots = (uint32_t)strtoul(argv[1], nullptr, 10);
    const uint64_t items = strtoull(argv[2], nullptr, 10);
    if (slots < rt_ring::BATCH || slots > 4096u) {
        fprintf(stderr, "slots out of range\n");
        return 2;
    }
    Rng rng{strtoull(argv[3], nullptr, 10)};
    Tally t;
    // the fixed cases first: every total around the batch size, in every mode, with lanes that end fast and slowly
    const uint32_t fixed[] = {0u, 1u, 2u, 31u, 63u, 64u, 65u, 66u, 67u, 68u, 100u, 127u, 128u, 129u, 130u, 131u, 191u, 192u, 193u, 1000u, 4096u, 65536u};
    uint64_t item = 0;
    for (uint32_t total : fixed)
        for (int mode = 0; mode < 5; ++mode)
            for (uint32_t end_one_in : {1u, 3u, 40u}) run_item(rng, slots, total, mode, end_one_in, item++, t);
    for (; item < items; ++item) {
        const uint32_t kind = rng.below(16u);
        // mostly pools of a few batches; some under one batch; a few long ones whose ring wraps hundreds of times
        const uint32_t total = kind < 4u ? 1u + rng.below(63u) : kind < 6u ? 64u * (1u + rng.below(8u)) : kind < 15u ? 1u + rng.below(1024u) : 1u + rng.below(40000u);
        run_item(rng, slots, total, (int)rng.below(5u), 1u + rng.below(30u), item, t);
    }
    printf("ok items %llu steps %llu batches %llu empty %llu full %llu hand_outs %llu wraps %llu most_wraps %llu one_batch %llu short %llu ragged %llu full_ring %llu\n",
           (unsigned long long)t.items, (unsigned long long)t.steps, (unsigned long long)t.batches, (unsigned long long)t.empty_batches,
           (unsigned long long)t.full_batches, (unsigned long long)t.hand_outs, (unsigned long long)t.wraps, (unsigned long long)t.most_wraps,
           (unsigned long long)t.one_batch_items, (unsigned long long)t.short_items, (unsigned long long)t.ragged_items, (unsigned long long)t.full_ring);
    return 0;
}
