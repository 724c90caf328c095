// rt_pool_profile.h — the region markers of the pooled trace kernel (rt_trace_pool_kernel.hip): RT_REGION_DECL,
// RT_REGION(k), RT_LANES(n, tail) and RT_REGION_FLUSH, which the kernel's text carries in every build and which expand
// to nothing in the product.  (Macros: they name the kernel's own `lane`, `A` and lane_rank of rt_pool_coop.h.)
#pragma once

// -DRT_PROFILE_REGIONS: developer build that accumulates the shader-clock cycles each wave
// spends per region of the path loop into A.segments[RT_STAT_REGIONS..]; rt_scene_last_stats prints them
// (tools/region_profile.sh).  Not part of the product build.
#ifdef RT_PROFILE_REGIONS
// rt_t_[0..15] region cycles, [16] the previous marker, [17..34] the two lane histograms, [35..36] noise counts
#define RT_REGION_DECL                                                          \
    __shared__ unsigned long long rt_t_all_[4][56];                             \
    unsigned long long *rt_t_ = rt_t_all_[threadIdx.x >> 6];                    \
    if ((threadIdx.x & 63) < 56) rt_t_[threadIdx.x & 63] = 0;                   \
    if ((threadIdx.x & 63) == 16) rt_t_[16] = __builtin_readcyclecounter();   \
    const unsigned long long rt_wave_start_ = wall_clock64();
// usable inside divergent code: the first ACTIVE lane books the time since the previous marker
#define RT_REGION(k)                                                            \
    do {                                                                        \
        const unsigned long long act_ = ballot(1);                            \
        if (lane_rank(act_) == 0) {                                             \
            const unsigned long long now_ = __builtin_readcyclecounter();       \
            rt_t_[k] += now_ - rt_t_[16];                                       \
            rt_t_[40 + (k)] += (now_ - rt_t_[16]) * (unsigned long long)__popcll(act_); \
            rt_t_[16] = now_;                                                   \
        }                                                                       \
    } while (0)
/* lanes tracing this iteration (wave-uniform n), booked while the pool has entries / in the item's tail */ \
#define RT_LANES(n, tail)                                                       \
    do {                                                                        \
        const int n_ = (n); /* the ballot needs every lane */                   \
        if (lane == 0) rt_t_[17 + ((tail) ? 9 : 0) + (n_ + 7) / 8] += 1;        \
    } while (0)
#define RT_REGION_FLUSH                                                         \
    if (lane < 16) atomicAdd(A.segments + RT_STAT_REGIONS + lane, rt_t_[lane]); \
    if (lane < 18) atomicAdd(A.segments + RT_STAT_LANES_BODY + lane, rt_t_[17 + lane]); \
    if (lane < 4) atomicAdd(A.segments + RT_STAT_NOISE + lane, rt_t_[35 + lane]); \
    if (lane < 16) atomicAdd(A.segments + RT_STAT_REGION_LANES + lane, rt_t_[40 + lane]); \
    if (lane == 0) { /* wall clock (100 MHz) of the first/last wave start and end */ \
        const unsigned long long end_ = wall_clock64();                         \
        atomicMin(A.segments + RT_STAT_WALL + 0, rt_wave_start_);               \
        atomicMax(A.segments + RT_STAT_WALL + 1, rt_wave_start_);               \
        atomicMin(A.segments + RT_STAT_WALL + 2, end_);                         \
        atomicMax(A.segments + RT_STAT_WALL + 3, end_);                         \
    }
#else
#define RT_REGION_DECL
#ifdef RT_ISA_MARKERS // `make isa`: the region boundaries as comments in the assembly listing (tools/isa_regions.py)
#define RT_REGION(k) asm volatile("; ==== end of region " #k);
#else
#define RT_REGION(k)
#endif
#define RT_LANES(n, tail)
#define RT_REGION_FLUSH
#endif
