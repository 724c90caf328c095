// rt_filter_taps.h — the tap loops and weights that the five guide-aware filter units share: rt_denoise.hip (the a-trous
// level), rt_temporal.hip (the variance-guided level, the variance of a history), rt_variance_filter.hip (the variance
// of a still frame), and rt_upsample.hip and rt_preview_temporal.hip (the blend of a preview's four anchors, at phase
// (0, 0) and at a frame's own).  DESIGN.md 4.6 and 4.11 to 4.14 define them; tests hold the paths to each other bit for
// bit, which they are because each is one function here.  Everything is f64, lane = pixel, 16x16 pixels per block, and
// every loop adds in one fixed order (dy, then dx; the anchors j, then i).
//
// The kernels that call these keep their names, arguments and launch shapes; against the hand-copied bodies they compile
// to the same floating-point instructions in the same registers, with other integer address and branch glue (LABNOTES).
#pragma once
#include "rt_trace_common.h"

namespace RT_KNS {

// Rec. 709 luminance; the weights one by one for the loop of k_batch_variance, which rounds each product on its own
__device__ __forceinline__ double luminance_weight(int c) { return c == 0 ? 0.2126 : c == 1 ? 0.7152 : 0.0722; }
__device__ __forceinline__ double luminance(d3 c) {
    return luminance_weight(0) * c.x + luminance_weight(1) * c.y + luminance_weight(2) * c.z;
}

// demodulation: v^2 (/ max(albedo, 1e-3)); the albedo is read only where it divides
__device__ __forceinline__ double demodulated(double v, const double &albedo, int demodulate) {
    const double L = v * v;
    return demodulate ? L / fmax(albedo, 1e-3) : L;
}

// w times the normal stop, then the plane stop, of tap q against the centre's normal np and position xp; a stop whose
// inverse sigma is 0 is off.  inv_fx = inv_sx / footprint_p.
__device__ __forceinline__ double guide_stops(double w, double inv_sn2, double inv_sx, double inv_fx, d3 np, d3 xp,
                                              const RtGuides &G, size_t q) {
    if (inv_sn2 > 0.0) {
        const d3 dn = np - ld3(G.normal + 3 * q);
        w *= exp(-len2(dn) * inv_sn2);
    }
    if (inv_sx > 0.0) {
        const double dist = dot(np, ld3(G.position + 3 * q) - xp) * inv_fx;
        w *= exp(-(dist * dist));
    }
    return w;
}

// One pixel of one a-trous level.  Each tap reads the neighbour's id, and where the ids agree its colour, normal and
// position (10 doubles); the weights are exp() of the stops' squared distances, multiplied in the order
// h(dx) h(dy) w_n w_x w_c of DESIGN.md 4.6.  VAR adds the luminance factor
// exp(-|l_p - l_q| / (sigma_l sqrt(vbar_p) + 1e-10)) after them and filters `var` alongside with the squared weights;
// without it sigma_l, var and var_out are not used.
template <bool VAR>
__device__ __forceinline__ void atrous_pixel(int width, int height, int step, double inv_sn2, double inv_sx, double inv_sc2,
                                             double sigma_l, const double *__restrict__ I, const double *__restrict__ var,
                                             const RtGuides &G, double *__restrict__ out, double *__restrict__ var_out) {
    const int px = blockIdx.x * 16 + (threadIdx.x & 15);
    const int py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= width || py >= height) return;
    const size_t p = (size_t)py * (size_t)width + (size_t)px;
    const d3 ip = ld3(I + 3 * p);
    const int id = G.obj_id[p];
    if (id < 0) { // a guide miss passes through
        out[3 * p + 0] = ip.x;
        out[3 * p + 1] = ip.y;
        out[3 * p + 2] = ip.z;
        if (VAR) var_out[p] = var[p];
        return;
    }
    double inv_sl = 0.0, lp = 0.0;
    if (VAR) {
        // vbar: the 3x3 Gaussian of the variance around the centre, at step 1, over the taps inside the image
        double vs = 0.0, vw = 0.0;
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = py + dy;
            if (qy < 0 || qy >= height) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = px + dx;
                if (qx < 0 || qx >= width) continue;
                const double k = (dx == 0 ? 0.5 : 0.25) * (dy == 0 ? 0.5 : 0.25); // 1/4, 1/8, 1/16
                vs += k * var[(size_t)qy * (size_t)width + (size_t)qx];
                vw += k;
            }
        }
        inv_sl = 1.0 / (sigma_l * sqrt(vs / vw) + 1e-10);
        lp = luminance(ip);
    }
    const double kh[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    const d3 np = ld3(G.normal + 3 * p), xp = ld3(G.position + 3 * p);
    const d3 sp = mk(sqrt(ip.x), sqrt(ip.y), sqrt(ip.z));
    const double inv_fx = inv_sx / G.footprint[p]; // 1 / (sigma_x * s * footprint_p)
    d3 sum = mk(0.0, 0.0, 0.0);
    double wsum = 0.0, vsum = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = py + dy * step;
        if (qy < 0 || qy >= height) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = px + dx * step;
            if (qx < 0 || qx >= width) continue;
            const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
            if (G.obj_id[q] != id) continue;
            const d3 iq = ld3(I + 3 * q);
            double w = guide_stops(kh[dx + 2] * kh[dy + 2], inv_sn2, inv_sx, inv_fx, np, xp, G, q);
            if (inv_sc2 > 0.0) {
                const d3 dc = sp - mk(sqrt(iq.x), sqrt(iq.y), sqrt(iq.z));
                w *= exp(-len2(dc) * inv_sc2);
            }
            if (VAR) w *= exp(-fabs(lp - luminance(iq)) * inv_sl);
            sum = sum + w * iq;
            wsum += w;
            if (VAR) vsum += (w * w) * var[q];
        }
    }
    const double inv = 1.0 / wsum; // the centre tap alone weighs 9/64
    out[3 * p + 0] = sum.x * inv;
    out[3 * p + 1] = sum.y * inv;
    out[3 * p + 2] = sum.z * inv;
    if (VAR) var_out[p] = vsum * (inv * inv);
}

// The variance of the luminance of C over the 7x7 window of pixel p = (px, py) with id >= 0, under the two guide stops.
// The squares are rounded on their own (__dmul_rn): a flat window gives exactly 0.
__device__ __forceinline__ double spatial_variance(int px, int py, int width, int height, double inv_sn2, double inv_sx,
                                                   const double *__restrict__ C, const RtGuides &G, size_t p, int id) {
    const d3 np = ld3(G.normal + 3 * p), xp = ld3(G.position + 3 * p);
    const double inv_fx = inv_sx / G.footprint[p];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int dy = -3; dy <= 3; ++dy) {
        const int qy = py + dy;
        if (qy < 0 || qy >= height) continue;
        for (int dx = -3; dx <= 3; ++dx) {
            const int qx = px + dx;
            if (qx < 0 || qx >= width) continue;
            const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
            if (G.obj_id[q] != id) continue;
            const double w = guide_stops(1.0, inv_sn2, inv_sx, inv_fx, np, xp, G, q);
            const double lq = luminance(ld3(C + 3 * q));
            s0 += w;
            s1 += w * lq;
            s2 += w * __dmul_rn(lq, lq);
        }
    }
    const double mean = s1 / s0; // the centre tap weighs 1, so a pixel alone in its window has none
    return fmax(0.0, s2 / s0 - __dmul_rn(mean, mean));
}

// (i0, i1, t) of one axis of the preview's grid shifted by the phase j: the anchors of column i sit at x = i step + j
__device__ __forceinline__ void shifted_axis(int x, int j, int step, int count, int &i0, int &i1, double &t) {
    const int xs = x - j;
    i0 = xs < 0 ? 0 : min(xs / step, count - 1);
    i1 = min(i0 + 1, count - 1);
    t = (xs < 0 || i1 == i0) ? 0.0 : (double)(xs - i0 * step) / (double)step;
}

// the four anchors' weighted sum for one pixel; (i0, j0) is its first anchor
struct AnchorBlend {
    d3 acc;
    double wsum;
    int i0, j0;
};

// DESIGN.md 4.13's blend of the anchors (j0,i0) (j0,i1) (j1,i0) (j1,i1) around pixel p = (px, py) of the preview frame
// `rgb`, on the grid of P (step_x, step_y, gx, gy) shifted by the phase (jx, jy) of 4.14: b = by bx, a tap with b == 0 or
// another obj_id is skipped, w = b w_n w_x, the value demodulated.  An anchor's guides are read at the pixel it traced,
// (i step_x + jx, j step_y + jy), its colour at its block's top-left pixel; at phase (0, 0) the two are one pixel.
template <class Args>
__device__ __forceinline__ AnchorBlend anchor_blend(const Args &P, int jx, int jy, const double *__restrict__ rgb,
                                                    const RtGuides &G, int px, int py, size_t p, int id, d3 np, d3 xp) {
    AnchorBlend r;
    int i1, j1;
    double tx, ty;
    shifted_axis(px, jx, P.step_x, P.gx, r.i0, i1, tx);
    shifted_axis(py, jy, P.step_y, P.gy, r.j0, j1, ty);
    const int qi[2] = {r.i0, i1}, qj[2] = {r.j0, j1};
    const double bx[2] = {1.0 - tx, tx}, by[2] = {1.0 - ty, ty};
    const double inv_fx = P.inv_sx / G.footprint[p]; // a miss has footprint inf: 0
    r.acc = mk(0.0, 0.0, 0.0);
    r.wsum = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double b = by[k >> 1] * bx[k & 1];
        if (b == 0.0) continue;
        const int ay = qj[k >> 1] * P.step_y, ax = qi[k & 1] * P.step_x; // the block's top-left pixel: the colour
        const size_t qc = (size_t)ay * (size_t)P.width + (size_t)ax;
        const size_t q = (size_t)(ay + jy) * (size_t)P.width + (size_t)(ax + jx); // the pixel it traced: the guides
        if (G.obj_id[q] != id) continue; // (-1 == -1: sky interpolates between sky anchors)
        const double w = guide_stops(b, P.inv_sn2, P.inv_sx, inv_fx, np, xp, G, q);
        const d3 v = mk(demodulated(rgb[3 * qc + 0], G.albedo[3 * q + 0], P.demodulate),
                        demodulated(rgb[3 * qc + 1], G.albedo[3 * q + 1], P.demodulate),
                        demodulated(rgb[3 * qc + 2], G.albedo[3 * q + 2], P.demodulate));
        r.acc = r.acc + w * v;
        r.wsum += w;
    }
    return r;
}

} // namespace RT_KNS
