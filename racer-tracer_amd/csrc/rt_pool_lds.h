// rt_pool_lds.h — the per-wave LDS layouts of the pooled trace kernel (rt_trace_pool_kernel.hip): the request slots of
// the cooperative samplers and the two forms of a wave's scratch, WaveLds and PretraceLds.
#pragma once
#include "rt_trace_common.h"

namespace RT_KNS {

// Request slots of the wave-cooperative Perlin turbulence (coop_noise_turbulence): eight lookups per
// round, eight lanes each.
struct NoiseSlots {
    double p[8][3];    // hit point of the lookup
    int depth[8];      // its texture's octave count (noise.rs:28)
    int perlin[8];     // ... and gradient table
    double term[8][8]; // 0.5^o * noise(2^o * p) of the round's octaves, summed in order by the requester
};
// A request of the lens-disk sampler: {pixel, sample, 0, next candidate}
struct alignas(16) Req4 { // one 128-bit LDS access
    uint32_t x, y, z, w;
};
// A request of the sphere sampler: the scatter prefix of (pixel, sample, segment) and the next candidate.  After the
// round's ballot the same 24 bytes carry the answer back: the first accepted candidate of the group that served the slot
// writes its three coordinates over the request, and the requester reads them from there.
struct alignas(8) SphereSlot {
    uint32_t b, y, x, w, z, base;
};
static_assert(sizeof(SphereSlot) == 3 * sizeof(double), "a slot holds the request or the sample");

// The sampler's request slots and the turbulence slots are never live at the same time (the Noise rounds of
// an iteration end before its sampler rounds begin, and both finish with what they posted), so they share
// their LDS: the textured variants — the BVH ones above all, whose node array already fills LDS to
// three blocks per CU — cost no more LDS than the plain ones.
// (A round of the samplers that has more than 32 requests open gives every lane its own candidate and touches no slot, so 32
// slots are all they use; variants without textures have no Noise lookups to make room for.)
template <bool TEXTURED> union SamplerScratch {
    Req4 req[32];
    SphereSlot sphere[32];
    NoiseSlots noise;
};
template <> union SamplerScratch<false> {
    Req4 req[32];
    SphereSlot sphere[32];
};

// What the END of an item needs of it (finish_item), parked while the item's last paths are in flight and the wave already
// hands out the next item's.
struct alignas(16) ItemInfo {
    int chunk, tx, ty, tile_py0, region, reg_tiles, rows_aligned, _pad;
};

// Per-wave scratch in LDS.  HAS_TIME: the scene has MovingSpheres (PRIMS_ANY variants).
// NBUF: batches of camera samples kept (2, or 1 for the BVH variants, whose node array wants the LDS).
// The lens-disk samples of a batch (16 B per entry) are NOT in here: only a camera with an aperture draws them, and
// without their 8 KB per block the plain variants fit six blocks per CU instead of five (cornell 85.2 -> 82.1 ms).
// They live behind everything else in DYNAMIC LDS, which the launch sizes by the camera (TraceArgs.lens_lds).
// OVERLAP: the variant keeps two items in flight (see SUMS AND OVERLAPPED ITEMS in the kernel): two sets of sums, and — to pay
// for them — the per-pixel `base` vector is replaced by the jitter it is made of.
template <bool TEXTURED, int NBUF, bool OVERLAP> struct WaveLds {
    // per pixel of the CURRENT item's tile (the one entries are handed out of): upper_left_corner + u * horizontal with the
    // pixel's ONE horizontal jitter u = (px + ju) / (W - 1) (cpu.rs:35-36, camera.rs:331) — or, OVERLAP, just u: the
    // hand-out then forms the vector (three fma and a read of `ulc` per iteration for 1 KB)
    double base[OVERLAP ? 1 : 64][3];
    double u[OVERLAP ? 64 : 1];
    // per-pixel radiance sums: doubles — or, OVERLAP, 64-bit fixed-point integers (TraceArgs.sum_scale) of the (up to) two
    // items in flight: slot s, pixel p at [s * 64 + p]
    double sum[OVERLAP ? 128 : 64][3];
    SamplerScratch<TEXTURED> scratch; // cooperative sampler requests / Noise lookups
    uint8_t pix_of[64]; // pool slot -> lane-order pixel index, for tiles cut by the image edge (current item)
    // Camera samples of the pool entries, drawn 64 entries at a time by the WHOLE wave
    // (prepare_batch below): entry w sits in slot w & 63 of buffer (w >> 6) & (NBUF - 1).
    double v[NBUF][64];        // (py + jv) / (H - 1)                      cpu.rs:39-40
    ItemInfo info[2];
    // camera.upper_left_corner, for the hand-out: v_fma_f64 reads ONE scalar operand, so of upper_left_corner + u * horizontal
    // one vector has to come from vector registers — copied there with six v_mov_b32 per iteration, or read from here
    double ulc[3];
};

// Survivors of the PRETRACE variant's camera batches that may wait for a lane (see PRIMARY SEGMENTS IN THE BATCHES in the
// kernel): a batch adds up to 64 and runs when at most RING_SLOTS - 64 are waiting.  67 is what 2 024 bytes per wave hold
// of 30-byte entries; nothing but a batch needs free slots.
enum : uint32_t { RING_SLOTS = 67u };
// A ring entry's `best` word: the primitive in the low bits (the table is staged in LDS, 192 bytes a record: under 1 000
// records), and above it the sign bits of the camera ray's direction, which is all the normal of the hit needs of it
enum : uint32_t { RING_BEST_BITS = 13u, RING_BEST_MASK = (1u << RING_BEST_BITS) - 1u };
// Per-wave scratch of the PRETRACE variant (rects only, no textures, no specular materials): the members of WaveLds that
// variant reads, under the same names, and the ring of pool entries whose primary segment a batch has traced and that
// live on.  An entry is the POINT of its primary hit, its pool index, and the `best` word above: 30 bytes, as a structure
// of arrays.  The lane that takes it loads the point into its ray origin and computes nothing: the camera ray, its
// parameter and the lens sample were consumed by the batch.  WaveLds' `base` and `v` have no counterpart.  The block has
// at most 20 096 bytes of static LDS, and seven blocks fit a CU beside C3's primitive table (the seven-block edge is
// 23 040 bytes) — in the RT_PROFILE_REGIONS build too, which 64 bytes more would cost a block per CU.
struct PretraceLds {
    // camera.origin and background.top, for the same reason as `ulc` below: a rect test and an LDS add take their
    // operands from vector registers, and an LDS read puts them there without a vector instruction
    double cam_origin[3], bg_top[3];
    double u[64];      // per pixel of the tile: (px + ju) / (W - 1)
    double sum[64][3]; // per-pixel radiance sums (doubles)
    SamplerScratch<false> scratch;
    uint8_t pix_of[64];
    double ring_p[3][RING_SLOTS];   // the entry's primary hit: its point (ray_at of the batch's ray) ...
    uint32_t ring_w[RING_SLOTS];    // (its index in the item's pool)
    uint16_t ring_best[RING_SLOTS]; // ... its primitive, and the ray direction's signs: bit RING_BEST_BITS + k set = d[k] < 0
    uint32_t n_started;            // paths this wave has started (RtRenderStats.samples): every entry of every batch
    // the current item's rect mask (start_item): bit i clear = no pixel of the item can see record i of the table, and the
    // item's batches step over it.  Here, not in a scalar register: the path loop has none to spare.  (32 bits for the
    // RT_PRIMARY_RECTS = 16 records that have a rectangle: the word fills the padding in front of `info`, so the block's
    // static LDS stays at 20 096 bytes.)
    uint32_t rect_mask;
    ItemInfo info[1]; // (one item at a time)
    double ulc[3];
};

} // namespace RT_KNS
