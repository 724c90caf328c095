// rt_frame_kernels.hip — the kernels that trace nothing and only turn sums into frames, with their launchers:
//   k_resolve_f64         the v1 kernel's (rt_trace_kernel.hip) and the NEE frame's resolve pass over per-pixel sums;
//   k_resolve_chunks_f64  the pooled kernel's (rt_trace_pool_kernel.hip) resolve pass over its slices;
//   k_fold_chunks_f64     one pass of a progressive frame over the same slices;
//   k_fold_adaptive_f64   one pass of an adaptive frame: that fold, and the tiles' decisions (rt_tile_decide.h).
// Built in both arithmetic flavours like the trace kernels (rt_trace_common.h: ARITHMETIC): RT_ARITH_FAST contracts the
// folds' multiply-adds, RT_ARITH_REFERENCE does not.
#include "rt_trace_common.h"
#include "rt_tile_decide.h"

namespace RT_KNS {

// vec3.rs:119-125 scale_sqrt over the owned rows: out = sqrt(accum / samples)
__global__ __launch_bounds__(256) void k_resolve_f64(const double *__restrict__ accum, double *__restrict__ out,
                                                     int width, int height, int strip_rows, int strip_count,
                                                     int strip_index, double scale) {
    size_t n = (size_t)width * (size_t)height * 3;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (strip_count > 1) {
            int row = (int)(i / ((size_t)width * 3));
            if ((row / strip_rows) % strip_count != strip_index) continue;
        }
        out[i] = sqrt(scale * accum[i]);
    }
}

// vec3.rs:119-125 scale_sqrt over the owned rows: out = sqrt(sum over chunks / samples),
// chunks added in index order.  With step_x/step_y > 1 (preview renderer) every pixel takes
// the value of its block's top-left pixel and pixels outside the covered area are (0,0,0)
// (cpu_scaled.rs:50-52, :80-89).  `out` is the plain [height][width][3] frame (out_cols == 1) or the tile-column layout
// of the tile stream — column c of out_col_step pixels (the last takes the remainder, cpu.rs:97-109) stored as
// [height][column width][3] behind the columns before it — so that a tile of rt_render is one contiguous run.
__global__ __launch_bounds__(256) void k_resolve_chunks_f64(const double *__restrict__ partial, double *__restrict__ out,
                                                            int width, int height, int n_chunks, int slice_rows, int strip_rows,
                                                            int strip_count, int strip_index, int step_x, int step_y,
                                                            int cover_w, int cover_h, int out_col_step, int out_cols,
                                                            double scale) {
    // a slice holds the launch's OWNED rows only (TraceArgs.slice_rows): with strips the pass walks those rows and maps
    // each to its image row; the preview's slice rows are grid rows, read by every pixel of a block
    const size_t slice = (size_t)width * (size_t)slice_rows * 3;
    const size_t n = (size_t)width * (size_t)(strip_count > 1 ? slice_rows : height) * 3;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        size_t src = i, dst = i;
        if (strip_count > 1 || step_x > 1 || step_y > 1 || out_cols > 1) {
            const size_t pixel = i / 3;
            const int ch = (int)(i - pixel * 3);
            const int r = (int)(pixel / (size_t)width), col = (int)(pixel - (size_t)r * (size_t)width);
            int row = r;
            if (strip_count > 1) { // r is a row of the owned-row grid
                row = ((r / strip_rows) * strip_count + strip_index) * strip_rows + r % strip_rows;
                if (row >= height) continue;
            }
            dst = ((size_t)row * (size_t)width + (size_t)col) * 3 + ch;
            if (out_cols > 1) {
                int c = col / out_col_step;
                if (c > out_cols - 1) c = out_cols - 1;
                const int col_x = c * out_col_step;
                const int col_w = c == out_cols - 1 ? width - col_x : out_col_step;
                dst = ((size_t)height * (size_t)col_x + (size_t)row * (size_t)col_w + (size_t)(col - col_x)) * 3 + ch;
            }
            if (col >= cover_w || row >= cover_h) {
                out[dst] = 0.0;
                continue;
            }
            src = ((size_t)(r / step_y) * (size_t)width + (size_t)(col - col % step_x)) * 3 + ch;
        }
        double acc = 0.0;
        for (int c = 0; c < n_chunks; ++c) acc += partial[(size_t)c * slice + src];
        out[dst] = sqrt(scale * acc);
    }
}

// One pass of a progressive frame (rt_progressive.hip): whole-frame slices (n = width * height * 3 elements each), the
// slices [c0, c1) added to the running sums in index order and out = sqrt(scale * running), scale = 1 / samples so far.
// `running` starts the frame at +0.0, so the passes together are k_resolve_chunks_f64's left fold over the same slices and
// the last pass's frame is bit-identical to the one-shot frame.
__global__ __launch_bounds__(256) void k_fold_chunks_f64(const double *__restrict__ partial, double *__restrict__ running,
                                                         double *__restrict__ out, size_t n, int c0, int c1, double scale) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        double acc = running[i];
        for (int c = c0; c < c1; ++c) acc += partial[(size_t)c * n + i];
        running[i] = acc;
        out[i] = sqrt(scale * acc);
    }
}

// One pass of rt_render_adaptive (rt_progressive.hip; rtdev::AdaptiveFold): rt_tile_decide.h's step with the fold in front.
// A running tile folds exactly as k_fold_chunks_f64 does — same left fold from +0.0, same sqrt(scale * acc) — so its
// pixels are the progressive frame's bits; beside the sums it keeps Q, the chunks' squares over their sample counts, for
// the error over the chunks as batch means.
__global__ __launch_bounds__(1024) void k_fold_adaptive_f64(const AdaptiveFold F) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = (int)blockIdx.x * 16 + wave; // wave-uniform
    uint32_t keep = 0; // (lane 0) this wave's tile runs on
    if (t < F.d.n_tiles) {
        const size_t n = (size_t)F.d.width * (size_t)F.d.height * 3;
        keep = decide_tile(F.d, t, lane, [&](size_t i, double (&acc)[3], double (&q)[3]) {
            for (int c = F.c0; c < F.d.chunks_done; ++c) {
                const double *src = F.partial + (size_t)c * n + i;
                const double v0 = src[0], v1 = src[1], v2 = src[2], inv = F.inv_chunk[c];
                acc[0] += v0;
                acc[1] += v1;
                acc[2] += v2;
                q[0] += v0 * v0 * inv;
                q[1] += v1 * v1 * inv;
                q[2] += v2 * v2 * inv;
            }
            for (int ch = 0; ch < 3; ++ch) {
                F.d.running[i + ch] = acc[ch];
                F.d.squares[i + ch] = q[ch];
            }
        });
    }
    append_running_tiles(F.d, t, lane, wave, keep);
}

} // namespace RT_KNS

extern "C" hipError_t RT_LAUNCHER(rtdev_launch_resolve)(const double *accum, double *out, int width, int height,
                                           int strip_rows, int strip_count, int strip_index, int samples,
                                           hipStream_t stream) {
    size_t n = (size_t)width * (size_t)height * 3;
    unsigned blocks = (unsigned)((n + 255) / 256);
    if (blocks > 2048u) blocks = 2048u;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(RT_KNS::k_resolve_f64, dim3(blocks), dim3(256), 0, stream, accum, out, width, height,
                       strip_rows, strip_count, strip_index, 1.0 / (double)samples);
    return hipGetLastError();
}

extern "C" hipError_t RT_LAUNCHER(rtdev_launch_resolve_chunks)(const double *partial, double *out, int width, int height, int n_chunks,
                                                               int slice_rows, int strip_rows, int strip_count, int strip_index, int step_x, int step_y,
                                                               int cover_w, int cover_h, int out_col_step, int out_cols, int samples,
                                                               hipStream_t stream) {
    if (out_cols <= 1 || out_col_step <= 0) {
        out_cols = 1;
        out_col_step = width;
    }
    size_t n = (size_t)width * (size_t)(strip_count > 1 ? slice_rows : height) * 3;
    unsigned blocks = (unsigned)((n + 255) / 256);
    if (blocks > 4096u) blocks = 4096u;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(RT_KNS::k_resolve_chunks_f64, dim3(blocks), dim3(256), 0, stream, partial, out, width, height,
                       n_chunks, slice_rows, strip_rows, strip_count, strip_index, step_x, step_y, cover_w, cover_h, out_col_step, out_cols,
                       1.0 / (double)samples);
    return hipGetLastError();
}

extern "C" hipError_t RT_LAUNCHER(rtdev_launch_fold_chunks)(const double *partial, double *running, double *out, size_t n, int c0,
                                                            int c1, int samples_done, hipStream_t stream) {
    unsigned blocks = (unsigned)((n + 255) / 256);
    if (blocks > 4096u) blocks = 4096u;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(RT_KNS::k_fold_chunks_f64, dim3(blocks), dim3(256), 0, stream, partial, running, out, n, c0, c1,
                       1.0 / (double)samples_done);
    return hipGetLastError();
}

extern "C" hipError_t RT_LAUNCHER(rtdev_launch_fold_adaptive)(const rtdev::AdaptiveFold *f, hipStream_t stream) {
    if (f->d.n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(RT_KNS::k_fold_adaptive_f64, dim3((unsigned)(f->d.n_tiles + 15) / 16), dim3(1024), 0, stream, *f);
    return hipGetLastError();
}
