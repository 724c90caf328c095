// rt_pool_coop.h — what the 64 lanes of a wave of the pooled trace kernel (rt_trace_pool_kernel.hip) do together: lane
// ranks and masked register updates, the closest-hit loop of the rects-only variants, and the wave-cooperative samplers
// (unit sphere, lens disk, Perlin turbulence) over the request slots of rt_pool_lds.h.
#pragma once
#include "rt_pool_groups.h"
#include "rt_pool_lds.h"
#include "rt_primary_bounds.h"
#include "rt_rect_pairs.h"

namespace RT_KNS {

static_assert(sizeof(Prim) == rt_pairs::kRecordBytes && offsetof(Prim, p) + 4 * sizeof(double) == rt_pairs::kOffsetOfK,
              "rt_rect_pairs.h addresses k in the table's bytes");

__device__ __forceinline__ int lane_rank(uint64_t mask) { // set bits of `mask` below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Posts a sphere sampler request as six 32-bit LDS stores.  Wider stores want the values in consecutive VGPRs: pixel,
// sample and candidate were then copied into such a quad in every iteration (v_mov_b32 around every round), and the
// stores cost the LDS pipe, which the path loop barely uses, instead of the vector one.  (Relaxed atomic stores: plain
// ones are merged back into wider stores.)
__device__ __forceinline__ void post_request(SphereSlot *slot, const ScatterPrefix &P, uint32_t base) {
    __hip_atomic_store(&slot->b, P.b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __hip_atomic_store(&slot->y, P.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __hip_atomic_store(&slot->x, P.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __hip_atomic_store(&slot->w, P.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __hip_atomic_store(&slot->z, P.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __hip_atomic_store(&slot->base, base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
// v = p in the lanes of `mask`, in v's own registers.  Written in C++, a masked write of the sphere sampler's `result` is a
// branch around it, and the compiler copied `result` on both sides of the branch and back at the join; this does the
// masking itself, so to the compiler it is an unconditional update of `v` in place.
__device__ __forceinline__ void move_masked(const d3 &p, uint64_t mask, d3 &v) {
    uint64_t saved;
    asm volatile("s_and_saveexec_b64 %[saved], %[mask]\n\t"
                 "v_mov_b64 %[x], %[px]\n\t"
                 "v_mov_b64 %[y], %[py]\n\t"
                 "v_mov_b64 %[z], %[pz]\n\t"
                 "s_mov_b64 exec, %[saved]"
                 : [x] "+v"(v.x), [y] "+v"(v.y), [z] "+v"(v.z), [saved] "=&s"(saved)
                 : [mask] "s"(mask), [px] "v"(p.x), [py] "v"(p.y), [pz] "v"(p.z)
                 : "scc");
}
// v += 1 in the lanes of `mask` (wave-uniform), as one add with the mask as its carry-in; written in C++ it is a select of
// 0 / 1 (v_cndmask_b32) and an add.
__device__ __forceinline__ void increment_masked(uint32_t &v, uint64_t mask) {
    asm("v_addc_co_u32 %[v], vcc, 0, %[v], %[mask]" : [v] "+v"(v) : [mask] "s"(mask) : "vcc");
}
// The pooled kernel's second argument (rt_primary_bounds.h: PrimaryRects), re-read where it is used like the first
// (kernargs_here): it follows TraceArgs in the kernel argument segment.
static_assert(sizeof(TraceArgs) % alignof(rtdev::PrimaryRects) == 0, "no padding between the kernel's two arguments");
__device__ __forceinline__ const RT_CONSTANT rtdev::PrimaryRects *primary_rects_here() {
    return (const RT_CONSTANT rtdev::PrimaryRects *)((const RT_CONSTANT unsigned char *)kernargs_here() + sizeof(TraceArgs));
}
// The number of open requests of a sampler round, 1 .. 64, as a 32-bit scalar.  The empty asm is what keeps it one: left
// to itself the compiler widens the count to 64 bits, for which the scalar unit has no ordered compare, and every
// comparison with it becomes a vector compare of two scalars (v_cmp_gt_u64 and an s_and_b64 with exec behind it).
__device__ __forceinline__ uint32_t request_count(uint64_t pending) {
    uint32_t n = (uint32_t)__builtin_popcountll(pending);
    asm("" : "+s"(n));
    return n;
}
// (The lowest set bit of every group of 2^lg bits of a lane mask, lowest_in_groups, is in rt_pool_groups.h with the rest
// of the group arithmetic: the formula it had here, over masks read from a table.)

// The closest-hit loop of the rects-only variants over the grouped table (XY, XZ, YZ rects, in that order: record order,
// strict `t < best_t`), one straight-line test per group with the plane a compile-time constant.  PAIRS: two records per
// scalar-load wait (what the path loop runs); without, one test site per plane (the camera batches: every site is a copy
// of the rect test in the kernel's text).
// `rect_mask` (the batches only): record i is stepped over, in front of its scalar load, when bit i is clear — no ray of
// the call can hit it (rt_trace_pool_kernel.hip: start_item).  Bits exist for the table's first RT_PRIMARY_RECTS records;
// a longer table comes with every bit set, so the bit of record i & 31 answers for record i.
static_assert(rtdev::RT_PRIMARY_RECTS <= 32, "a rect mask is one 32-bit word");
template <bool PAIRS>
__device__ __forceinline__ void closest_hit_rects(const Prim *table, const d3 &o, const d3 &d, const d3 &inv_d, double &best_t, int &best,
                                                  uint32_t rect_mask = ~0u, const Prim *lds_table = nullptr) {
    auto test_plane = [&](auto axis, const Prim &P, int i) {
#ifndef RT_EXACT_DIV
        rect_closest_update<decltype(axis)::value>(P.p[0], P.p[1], P.p[2], P.p[3], P.p[4], o, d, inv_d, 0.001, best_t, best, i);
        return;
#endif
        double t;
        if (rect_t<true>(decltype(axis)::value, P.p[0], P.p[1], P.p[2], P.p[3], P.p[4], o, d, inv_d, 0.001, best_t, t)) {
            best_t = t;
            best = i;
        }
    };
    const Prim *rec = table; // ONE pointer runs through the groups (they follow each other in the table)
    int i = 0;
    auto group = [&](auto axis, int end) {
        if (PAIRS) {
            for (; i + 1 < end; i += 2, rec += 2) {
                const Prim pa = load_prim_uniform(rec, 0), pb = load_prim_uniform(rec, 1);
#ifndef RT_EXACT_DIV
                // A FACING PAIR (rt_rect_pairs.h; marked in the first record's p[5] by rt_scene_create): every lane selects
                // the record its direction points at and reads that record's k, and its partner's, from the table's copy in
                // LDS (a select between two scalars is two moves and a select per word on this target).  When the partner's
                // plane lies behind t_min in every lane, the first test runs on the selected record and the second is
                // stepped over; in every other case both run as they always did.
                constexpr int AXIS = decltype(axis)::value;
                // (the two marks as 32-bit scalars — see request_count — read as the single words they are, and in hand with
                // the first record's bounds before the branch: left to itself the compiler loads the bounds behind the
                // selection, one more wait in a row.  Both k stay out of this: the settled path reads neither as a scalar)
                const RT_CONSTANT uint32_t *words = (const RT_CONSTANT uint32_t *)rec;
                uint32_t larger = words[(rt_pairs::kOffsetOfK + 12u) / 4u], step = words[(rt_pairs::kRecordBytes + rt_pairs::kOffsetOfK + 12u) / 4u];
                asm volatile("; pair requested" : "+s"(larger), "+s"(step) : "s"(pa.p[0]), "s"(pa.p[1]), "s"(pa.p[2]), "s"(pa.p[3]));
                double k_first;
                int i_first;
                uint32_t second = 1u; // whether the second record is tested too; a 32-bit scalar (see request_count)
                // (written as nested if / else with the plain case twice: one join behind them costs the scalar unit a flag
                // and a branch on it)
                auto plain = [&] {
                    k_first = pa.p[4];
                    i_first = i;
                    asm volatile("; both records" : "+v"(k_first), "+v"(i_first)); // (keeps the branch a branch: see near_zero)
                };
                if (larger != 0u) {
                    using lds_bytes = const __attribute__((address_space(3))) unsigned char *;
                    const uint32_t k_of_larger = (uint32_t)(uintptr_t)(lds_bytes)reinterpret_cast<const unsigned char *>(lds_table) + larger;
                    const uint32_t sel = rt_pairs::selected(k_of_larger, step, rt_pairs::sign_mask(comp(d, AXIS)));
                    const double k_other = *(const __attribute__((address_space(3))) double *)(uintptr_t)rt_pairs::partner(k_of_larger, step, sel);
                    // (the lane's own record is read with its partner's k, one wait for both: the asm holds the reads
                    // here, in front of the branch they would otherwise sink behind)
                    k_first = *(const __attribute__((address_space(3))) double *)(uintptr_t)sel;
                    i_first = *(const __attribute__((address_space(3))) int *)(uintptr_t)(sel + 8u);
                    asm volatile("; facing pair" : "+v"(k_first), "+v"(i_first));
                    if (ballot(!rt_pairs::settled(rt_pairs::t_of_plane(k_other, comp(o, AXIS), comp(inv_d, AXIS)))) == 0) {
                        second = 0u;
                    } else {
                        plain();
                    }
                } else {
                    plain();
                }
                rect_closest_update<AXIS, true>(pa.p[0], pa.p[1], pa.p[2], pa.p[3], k_first, o, d, inv_d, 0.001, best_t, best, i_first);
                asm("" : "+s"(second));
                if (second != 0u) test_plane(axis, pb, i + 1);
#else
                test_plane(axis, pa, i);
                test_plane(axis, pb, i + 1);
#endif
            }
            if (i < end) {
                test_plane(axis, load_prim_uniform(rec, 0), i);
                ++i;
                ++rec;
            }
        } else {
            // a plane none of whose records is left: stepped over whole, in front of the ray's reciprocal on that axis
            // (which the compiler forms where the group's first test needs it)
            const int n = end - i;
            if (n > 0 && n < 32 && ((rect_mask >> (i & 31)) & ((1u << n) - 1u)) == 0u) {
                i = end;
                // (the byte offset as a 32-bit product, in the scalar unit)
                rec = reinterpret_cast<const Prim *>(reinterpret_cast<const unsigned char *>(rec) + (uint32_t)n * (uint32_t)sizeof(Prim));
            }
            for (; i < end; ++i, ++rec)
                if ((rect_mask >> (i & 31)) & 1u) test_plane(axis, load_prim_uniform(rec, 0), i);
        }
    };
    // (the group bounds are re-read from the kernel arguments here: see the path loop of the other variants)
    const RT_CONSTANT TraceArgs *KB = kernargs_here();
    const int end_xy = KB->rect_end[0], end_xz = KB->rect_end[1], end_yz = KB->rect_end[2];
    group(std::integral_constant<int, 2>(), end_xy); // XY
    group(std::integral_constant<int, 1>(), end_xz); // XZ
    group(std::integral_constant<int, 0>(), end_yz); // YZ
}

// vec3.rs:424-430 for every lane of `pending` (a wave-uniform lane mask, like the one it returns: the lanes
// that got their sample), evaluated by the whole wave.
// Must be called by all 64 lanes (wave-uniform control flow).  Runs at most
// MAX_ROUNDS rounds: a lane whose request is still open afterwards is not in the
// returned mask and keeps `base` (its first untested candidate), so the search resumes
// at the same stream position in the next call.
// The round count is a template constant: two rounds (the plain variants) are unrolled into straight-line code.  The
// first round writes `result` in EVERY lane (no lane holds a sample yet), so only the later rounds write it under the
// mask of the lanes still searching — a masked write is a copy of the old value at the join (C3 -0.8 %); both kinds of
// round end in ONE such write (move_masked), after their branches have joined.
// Every candidate is drawn from the scatter prefix of its request (philox_from_prefix): each lane forms its own once per
// call, and a grouped round posts it, so a candidate costs 10 multiplies instead of 14.  A grouped round's answer comes
// back through the request's slot, not through lane shuffles.
template <int MAX_ROUNDS>
__device__ __forceinline__ uint64_t coop_random_in_unit_sphere(uint64_t pending, uint32_t pixel, uint32_t sample, uint32_t seg,
                                                           uint32_t &base, uint32_t k0, uint32_t k1, int lane,
                                                           SphereSlot *slot, d3 &result) {
    uint64_t have = 0;
    const ScatterPrefix own = scatter_prefix(pixel, sample, seg, k0, k1);
    // One round; false when the rounds are over.
    auto one_round = [&](int round) {
        const bool FIRST = round == 0;
        const uint32_t n = request_count(pending);
        // a round costs the whole wave ~70 instructions; past the first it only runs while enough requests are
        // open to be worth that (the others resume next iteration): C2 +2.2 %, C3 +0.3 % (thresholds 2..16 and one to
        // six rounds measured again with one-block candidates: 8 and two rounds stay)
        if (!FIRST && n < 8u) return false;
        // group size q = 2^lg, the largest power of two with n * q <= 64
        const int lg = rt_groups::group_lg(n);
        // what `result` takes: in every lane in the first round, in the lanes of `take` in the later ones.  `result` only
        // means something to a lane of the returned mask, so a lane that still needs a sample may take whatever its round
        // left it, a rejected candidate included.
        d3 cand;
        uint64_t take;
        if (lg == 0) { // more than 32 requests: one candidate each, so every lane tests its OWN (no LDS)
            const d3 p = sphere_candidate(philox_from_prefix(own, base, k0, k1));
            cand = p;
            take = pending;
            const uint64_t inside = ballot(len2(p) < 1.0); // (the comparison's own lane mask)
            have |= pending & inside;
            pending &= ~inside;
            if (__builtin_amdgcn_inverse_ballot_w64(pending)) base += 1u;
        } else {
            const rt_groups::GroupMasks groups = rt_groups::group_masks((uint32_t)lg); // (read here: the load waits behind the candidates' Philox)
            const bool need = __builtin_amdgcn_inverse_ballot_w64(pending);
            const int rank = lane_rank(pending);
            if (need) post_request(slot + rank, own, base);
            const int j = lane >> lg;              // request served by this lane
            const int c = lane & ((1 << lg) - 1);  // candidate offset inside the group
            const bool serving = (uint32_t)j < n;
            SphereSlot *const served = slot + (serving ? j : 0);
            const ScatterPrefix r = {served->b, served->y, served->x, served->w, served->z};
            const uint32_t i = served->base + (uint32_t)c; // candidate index = its block (rt_rng.h)
            const d3 p = sphere_candidate(philox_from_prefix(r, i, k0, k1));
            // (ballots of the two comparisons, ANDed as scalars: a ballot of `serving && ...` is a lane mask turned into an
            // integer and back, v_cndmask_b32 + v_cmp_ne_u32)
            const uint64_t accepted = ballot(serving) & ballot(len2(p) < 1.0);
            // The first accepted candidate of every group, in stream order, answers its request in the slot it was read
            // from (after that read: one wave's LDS accesses complete in order, and the empty asm keeps the compiler from
            // moving the double stores above the word loads).
            asm volatile("" ::: "memory");
            if (__builtin_amdgcn_inverse_ballot_w64(rt_groups::lowest_in_groups(accepted, groups))) {
                double *const answer = reinterpret_cast<double *>(served);
                answer[0] = p.x;
                answer[1] = p.y;
                answer[2] = p.z;
            }
            asm volatile("" ::: "memory"); // (and the answers' loads below them)
            // did my own request get one?  (a ballot of the comparison, ANDed with `pending` = ballot(need) as scalars)
            const int first = need ? (rank << lg) : 0;
            const uint64_t got = pending & ballot(((accepted >> first) & groups.width) != 0);
            // every lane reads a slot: what it finds means nothing to a lane that got none
            const double *const answer = reinterpret_cast<const double *>(slot + (need ? rank : 0));
            cand = mk(answer[0], answer[1], answer[2]);
            take = got;
            have |= got;
            pending &= ~got; // the lanes still searching
            if (__builtin_amdgcn_inverse_ballot_w64(pending)) base += 1u << lg;
        }
        if (FIRST) {
            result = cand;
        } else {
            move_masked(cand, take, result);
        }
        return true;
    };
    // The plain variants' two rounds are unrolled BY ORDER: round 0's unmasked write of `result` is a compile-time case of
    // `round` only then, and with the group size read off a bit count the optimiser no longer unrolls them by itself.  The
    // four rounds of the others stay with it (it peels round 0 and keeps ONE copy of the later rounds).
    if constexpr (MAX_ROUNDS == 2) {
#pragma unroll
        for (int round = 0; round < MAX_ROUNDS && pending != 0; ++round)
            if (!one_round(round)) break;
    } else {
        for (int round = 0; round < MAX_ROUNDS && pending != 0; ++round)
            if (!one_round(round)) break;
    }
    return have;
}

// util.rs:25-39 random_in_unit_disk for every lane with `need`, same scheme: one
// Philox block per candidate (block i -> x, y), first accepted candidate in stream
// order.  Runs until every request is settled (a fresh path needs its ray now).
__device__ __forceinline__ void coop_random_in_unit_disk(bool need, uint32_t pixel, uint32_t sample, uint32_t k0,
                                                         uint32_t k1, int lane, Req4 *req, double &out_x,
                                                         double &out_y) {
    uint32_t base = 0;
    uint64_t pending = ballot(need);
    while (pending != 0) {
        const uint32_t n = request_count(pending);
        const int lg = rt_groups::group_lg(n);
        if (lg == 0) { // one candidate per request: every lane tests its own (the usual first round of a batch)
            if (need) {
                const u4 b = philox4x32(pixel, sample, RT_RNG_LENS, base, k0, k1);
                const double x = sym53(b.a, b.b), y = sym53(b.c, b.d);
                if (x * x + y * y < 1.0) {
                    out_x = x;
                    out_y = y;
                    need = false;
                } else {
                    base += 1u;
                }
            }
            pending = ballot(need);
            continue;
        }
        const int rank = lane_rank(pending);
        if (need) req[rank] = Req4{pixel, sample, 0u, base};
        const int j = lane >> lg;
        const int c = lane & ((1 << lg) - 1);
        const bool serving = (uint32_t)j < n;
        const Req4 r = req[serving ? j : 0];
        const u4 b = philox4x32(r.x, r.y, RT_RNG_LENS, r.w + (uint32_t)c, k0, k1);
        const double x = sym53(b.a, b.b), y = sym53(b.c, b.d);
        const uint64_t accepted = ballot(serving && x * x + y * y < 1.0);
        const int first = need ? (rank << lg) : 0;
        const uint64_t mine = need ? ((accepted >> first) & rt_groups::group_masks((uint32_t)lg).width) : 0ull;
        const bool got = mine != 0;
        const int src = got ? first + __ffsll((unsigned long long)mine) - 1 : lane;
        const double rx = shfl_d(x, src), ry = shfl_d(y, src);
        if (got) {
            out_x = rx;
            out_y = ry;
            need = false;
        } else if (need) {
            base += 1u << lg;
        }
        pending = ballot(need);
    }
}

// SHADING SORTED BY COST: the one expensive texture.  A marble lookup (noise.rs:26-33, :98-109) is seven
// octaves of eight gradient dots, ~900 VALU instructions, and in a wave of 64 paths it is typically wanted by
// a handful of lanes at a time (noise_and_textures: <= 4 lanes in 60 % of the iterations that have one), so
// evaluated where the hit is shaded it runs at ~6 % lane use.  Octaves are independent until they are
// summed, so the wave evaluates them side by side instead: lanes note their lookup during shading
// (texture_value_deferred), then — all 64 lanes, wave-uniform control flow — eight lookups per round take
// eight lanes each, lane o of a group computes octave o (0.5^o * noise(2^o p), both scalings exact), and
// the requester adds the terms in octave order like the reference's loop.  One round costs about what ONE
// octave costs.  Every lookup goes through this code, so a value never depends on which lanes sat next to it.
// Returns turb(p, depth) (noise.rs:98-109) to the lanes with `need`; must be called by the whole wave.
__device__ __forceinline__ double coop_noise_turbulence(bool need, d3 p, int depth, int perlin, const TraceArgs &A,
                                                        const Perlin *lds_perlin, int lane, NoiseSlots &S) {
    double turb = 0.0;
    const uint64_t pending = ballot(need);
    const int n = __popcll(pending);
    const int rank = lane_rank(pending);
    const int j = lane >> 3, o8 = lane & 7; // this lane works on request j of the round, octave o8 (+ 8 per pass)
    for (int r0 = 0; r0 < n; r0 += 8) {
        const bool mine = need && rank >= r0 && rank < r0 + 8;
        const int slot = rank - r0;
        if (mine) {
            S.p[slot][0] = p.x;
            S.p[slot][1] = p.y;
            S.p[slot][2] = p.z;
            S.depth[slot] = depth;
            S.perlin[slot] = perlin;
        }
        const bool serving = r0 + j < n;
        const int dj = serving ? S.depth[j] : 0;
        double accum = 0.0; // noise.rs:99
        for (int ob = 0; ballot(serving && ob < dj) != 0; ob += 8) { // one pass unless a texture has more than 8 octaves
            const int o = ob + o8;
            double term = 0.0;
            if (serving && o < dj) {
                // noise.rs:103-106: temp_p doubles and weight halves per octave — powers of two, exact
                const d3 q = mk(__builtin_ldexp(S.p[j][0], o), __builtin_ldexp(S.p[j][1], o), __builtin_ldexp(S.p[j][2], o));
                const int pi = S.perlin[j];
                const double nz = (lds_perlin != nullptr && pi == 0) ? perlin_noise<true>(*lds_perlin, q)
                                                                     : perlin_noise<false>(A.perlins[pi], q);
                term = __builtin_ldexp(nz, -o);
            }
            S.term[j][o8] = term;
            if (mine) { // accum += weight * noise(temp_p), in octave order (absent octaves are +0.0)
#pragma unroll
                for (int k = 0; k < 8; ++k) accum += S.term[slot][k];
            }
        }
        if (mine) turb = fabs(accum); // noise.rs:108
    }
    return turb;
}

} // namespace RT_KNS
