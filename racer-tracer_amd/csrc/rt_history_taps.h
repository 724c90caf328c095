// rt_history_taps.h — the history of one pixel, for the two kernels that accumulate into an RtHistory:
// k_temporal_accumulate (rt_temporal.hip) and k_preview_accumulate (rt_preview_temporal.hip, 4.14).  The
// re-projection through the previous camera with its four bilinear taps, the blend of a sample with them and the stores of a
// history pixel are each one function here, so with steps of one the second kernel's history is the first's bit for bit
// (identity (b) of 4.14).  The argument block is a template parameter: the two blocks name the fields alike.
//
// The kernels keep their names, arguments and launch shapes; against the bodies written out in each they compile to the
// same floating-point instructions in the same registers, with other integer, address and branch glue (LABNOTES 18).
#pragma once
#include "rt_trace_common.h"

namespace RT_KNS {

__device__ __forceinline__ d3 cross3(d3 a, d3 b) {
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// the taps' weighted sums and 1 / their weight: a value is sum * inv, formed where it is used
struct HistorySums {
    d3 c;          // radiance
    double m1, m2; // luminance moments
    double len;    // history length
    double inv;
    double len_rn, w_rn; // LIVE only: the length's sum and the weight again, every product and sum rounded on its own
};

// One tap's share of a CARRIED length.  The sums of history_value may be contracted into fused multiply-adds as the compiler
// sees fit (sum(w L) and sum(w) then round differently, and a pixel whose taps all have length L would carry L only to
// rounding); these are not: w = round(a b), len_rn += round(w L), w_rn += w.  Where the taps share one length L that is a
// power of two every product is exact, len_rn == L w_rn, and the quotient is L itself whatever the weights' last bits are.
__device__ __forceinline__ void exact_tap(double a, double b, double lq, double &len_rn, double &w_rn) {
#pragma clang fp contract(off)
    const double w = a * b;
    len_rn = len_rn + w * lq;
    w_rn = w_rn + w;
}

// The history value of pixel p (id >= 0, normal np, position xp): the hit point through the PREVIOUS camera's pinhole
// (Cramer's rule) and the four bilinear taps (j, then i) that agree with it in id, normal and plane.  LIVE (4.14) adds one
// condition on a tap, its length must be > 0, so that a fill is never read as history, and exact_tap's sums; without it
// neither is compiled.  Whether a tap exists is decided on doubles: no index is formed, and nothing of the previous history
// is loaded, before the re-projected position is known to be finite and within one pixel of the previous image, and every
// tap is bounds-checked on its own.
// false: the hit point is behind or outside the previous image, or the taps that agree weigh less than 1e-3.
template <bool LIVE, class Args>
__device__ __forceinline__ bool history_value(const Args &P, const RtGuides &G, const RtHistory &prev, size_t p, int id, d3 np,
                                              d3 xp, HistorySums &h) {
    // ulc + u hor - v ver - o = s (x - o): columns hor, -ver, -(x - o) against o - ulc
    const d3 o = ld3(P.o);
    const d3 a = ld3(P.hor), b = -ld3(P.ver), cc = -(xp - o), r = o - ld3(P.ulc);
    const d3 bxc = cross3(b, cc);
    const double det = dot(a, bxc);
    const double u = dot(r, bxc) / det;
    const double v = dot(a, cross3(r, cc)) / det;
    const double s = dot(a, cross3(b, r)) / det;
    const double fx = u * (double)(P.width - 1) - 0.5;
    const double fy = v * (double)(P.height - 1) - 0.5;
    // (a NaN fails every comparison below)
    const bool inside = det != 0.0 && s > 0.0 && fx >= -1.0 && fx <= (double)P.width && fy >= -1.0 && fy <= (double)P.height;
    if (!inside) return false;
    const double flx = floor(fx), fly = floor(fy);
    const int x0 = (int)flx, y0 = (int)fly; // in [-1, W] and [-1, H]
    const double tx = fx - flx, ty = fy - fly;
    const double fp = G.footprint[p];
    d3 ch = mk(0.0, 0.0, 0.0);
    double mh1 = 0.0, mh2 = 0.0, lh = 0.0, wsum = 0.0;
    if (LIVE) h.len_rn = h.w_rn = 0.0;
    for (int j = 0; j < 2; ++j) {
        const int qy = y0 + j;
        if (qy < 0 || qy >= P.height) continue;
        for (int i = 0; i < 2; ++i) {
            const int qx = x0 + i;
            if (qx < 0 || qx >= P.width) continue;
            const size_t q = (size_t)qy * (size_t)P.width + (size_t)qx;
            if (prev.obj_id[q] != id) continue;
            const d3 dn = np - ld3(prev.normal + 3 * q);
            if (!(len2(dn) <= P.normal_tol2)) continue;
            const double dist = dot(np, ld3(prev.position + 3 * q) - xp);
            if (!(fabs(dist) <= P.plane_tol * fp)) continue;
            const double lq = prev.length[q];
            if (LIVE && !(lq > 0.0)) continue; // a fill
            const double w = (i ? tx : 1.0 - tx) * (j ? ty : 1.0 - ty);
            ch = ch + w * ld3(prev.radiance + 3 * q);
            mh1 += w * prev.moments[2 * q + 0];
            mh2 += w * prev.moments[2 * q + 1];
            lh += w * lq;
            wsum += w;
            if (LIVE) exact_tap(i ? tx : 1.0 - tx, j ? ty : 1.0 - ty, lq, h.len_rn, h.w_rn);
        }
    }
    if (!(wsum >= 1e-3)) return false;
    h.c = ch;
    h.m1 = mh1;
    h.m2 = mh2;
    h.len = lh;
    h.inv = 1.0 / wsum;
    return true;
}

// one pixel of a history, but for the guides it copies
struct HistoryPixel {
    d3 rad;
    double m1, m2, len;
};

// a sample (colour cp, luminance lp) that has no history: length 1
__device__ __forceinline__ HistoryPixel fresh_pixel(d3 cp, double lp) { return {cp, lp, lp * lp, 1.0}; }

// 4.11's blend of a sample with its history: N = L_h + 1, a = max(1 / N, alpha), the moments likewise
template <class Args> __device__ __forceinline__ HistoryPixel blended_pixel(const Args &P, const HistorySums &h, d3 cp, double lp) {
    const double inv = h.inv;
    const double N = h.len * inv + 1.0;
    const double al = fmax(1.0 / N, P.alpha), am = fmax(1.0 / N, P.alpha_moments);
    HistoryPixel r;
    r.rad = (1.0 - al) * (h.c * inv) + al * cp;
    r.m1 = (1.0 - am) * (h.m1 * inv) + am * lp;
    r.m2 = (1.0 - am) * (h.m2 * inv) + am * (lp * lp);
    r.len = fmin(N, P.max_history);
    return r;
}

// the thirteen stores of pixel p: its value and the current guides' normal, position and obj_id
__device__ __forceinline__ void store_history(const RtHistory &out, size_t p, const HistoryPixel &v, d3 np, d3 xp, int id) {
    out.radiance[3 * p + 0] = v.rad.x;
    out.radiance[3 * p + 1] = v.rad.y;
    out.radiance[3 * p + 2] = v.rad.z;
    out.moments[2 * p + 0] = v.m1;
    out.moments[2 * p + 1] = v.m2;
    out.length[p] = v.len;
    out.normal[3 * p + 0] = np.x;
    out.normal[3 * p + 1] = np.y;
    out.normal[3 * p + 2] = np.z;
    out.position[3 * p + 0] = xp.x;
    out.position[3 * p + 1] = xp.y;
    out.position[3 * p + 2] = xp.z;
    out.obj_id[p] = id;
}

} // namespace RT_KNS
