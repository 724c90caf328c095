// rt_primary_bounds.h — the pixel rectangles outside which no camera ray of a render can hit the scene, or one of its rects.
// The pooled trace kernel skips the camera batches of an 8x8 item none of whose pixels lies inside the scene's rectangle
// (rt_trace_pool_kernel.hip: start_item): on a camera that looks at the scene from outside that is every tile beside the
// scene's projection.  In the items that are left, a batch steps over the records of the rect table whose own rectangle
// holds no pixel of the item (primary_rects below; start_item forms the item's mask, closest_hit_rects<false> reads it): a
// tile usually sees one wall.
// Plain C++: no HIP header is needed, so the host compiler tests it alone (tests/test_primary_bounds_cpu.py,
// tests/test_primary_rect_bounds_cpu.py).
#pragma once
#include <cmath>
#include <stdint.h>

namespace rtdev {

// Inclusive: pixel (px, py) is inside when px0 <= px <= px1 and py0 <= py <= py1.  May be empty (px0 > px1 or py0 > py1:
// the box projects beside the frame).
struct PixelRect {
    int32_t px0, px1, py0, py1;
};

// The rectangle of the images of `n` points: false — "cannot tell" — when a point is on or behind the camera plane, the
// system is singular or ill-conditioned, or anything is not finite.  (The camera's vectors are the caller's to check.)
//
// The ray through (u, v) is ulc + u * horizontal - v * vertical - origin (camera.rs:331); pixel px draws
// u = (px + ju) / (W - 1) with ju in [0, 1) and row py draws v = (py + jv) / (H - 1) likewise (cpu.rs:35-40).  A point X
// is projected by solving (ulc - origin) + u * horizontal - v * vertical = lambda * (X - origin) for (u, v, lambda); with
// every point strictly in front of the camera (lambda > 0) the map is a perspective one, the image of the points' hull is
// the hull of their images and px sees the hull only if px + 1 > Umin and px <= Umax, U = u * (W - 1).
// The rectangle is rounded outward and padded by a whole pixel: at the distances of a scene a pixel is a fraction of a
// scene unit, a dozen orders of magnitude above any rounding here or in the device's primitive tests.
inline bool project_points(const double origin[3], const double ulc[3], const double horizontal[3], const double vertical[3],
                           int width, int height, const double (*points)[3], int n, PixelRect &out) {
    const double kPad = 1.0; // pixels
    // columns of the system: a = horizontal, b = -vertical, c = -(X - origin); right-hand side r = origin - ulc
    const double a[3] = {horizontal[0], horizontal[1], horizontal[2]};
    const double b[3] = {-vertical[0], -vertical[1], -vertical[2]};
    const double r[3] = {origin[0] - ulc[0], origin[1] - ulc[1], origin[2] - ulc[2]};
    auto det3 = [](const double p[3], const double q[3], const double s[3]) {
        return p[0] * (q[1] * s[2] - q[2] * s[1]) - p[1] * (q[0] * s[2] - q[2] * s[0]) + p[2] * (q[0] * s[1] - q[1] * s[0]);
    };
    auto norm3 = [](const double p[3]) { return std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]); };
    double u_min = INFINITY, u_max = -INFINITY, v_min = INFINITY, v_max = -INFINITY;
    for (int i = 0; i < n; ++i) {
        double c[3];
        for (int k = 0; k < 3; ++k) c[k] = -(points[i][k] - origin[k]);
        const double det = det3(a, b, c);
        // (ill-conditioned: the three columns nearly in one plane — the point nearly in the plane through the camera that
        // the image plane is parallel to, or a degenerate camera)
        if (!std::isfinite(det) || !(std::fabs(det) > 1e-9 * norm3(a) * norm3(b) * norm3(c))) return false;
        const double u = det3(r, b, c) / det, v = det3(a, r, c) / det, lambda = det3(a, b, r) / det;
        if (!std::isfinite(u) || !std::isfinite(v) || !std::isfinite(lambda) || !(lambda > 0.0)) return false;
        u_min = std::fmin(u_min, u);
        u_max = std::fmax(u_max, u);
        v_min = std::fmin(v_min, v);
        v_max = std::fmax(v_max, v);
    }
    // outward rounding, the pad, and a clamp to the frame's neighbourhood in double (the integers cannot overflow)
    auto low = [&](double t, int m) { return (int32_t)std::fmin(std::fmax(std::floor(t * (double)(m - 1)) - 1.0 - kPad, 0.0), (double)m); };
    auto high = [&](double t, int m) { return (int32_t)std::fmax(std::fmin(std::ceil(t * (double)(m - 1)) + kPad, (double)(m - 1)), -1.0); };
    out = PixelRect{low(u_min, width), high(u_max, width), low(v_min, height), high(v_max, height)};
    return true;
}

// A pixel OUTSIDE the rectangle has no primary ray that can hit anything inside the box [mn, mx]: the rectangle of the
// box's eight corners (project_points).
//
// Conservative by construction: in every doubtful case the answer is the whole frame ("cull off") — a corner on or
// behind the camera plane (which covers a camera inside the box), a singular or ill-conditioned system, anything
// non-finite, an empty box, a frame narrower than two pixels, and an aperture (the origins of its rays differ per sample).
inline PixelRect primary_bounds(const double origin[3], const double ulc[3], const double horizontal[3], const double vertical[3],
                                double lens_radius, int width, int height, const double mn[3], const double mx[3]) {
    const PixelRect whole = {0, width - 1, 0, height - 1};
    if (width < 2 || height < 2) return whole;
    if (!(lens_radius == 0.0)) return whole;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(origin[k]) || !std::isfinite(ulc[k]) || !std::isfinite(horizontal[k]) || !std::isfinite(vertical[k]))
            return whole;
        if (!std::isfinite(mn[k]) || !std::isfinite(mx[k]) || mn[k] > mx[k]) return whole;
    }
    double corners[8][3];
    for (int corner = 0; corner < 8; ++corner)
        for (int k = 0; k < 3; ++k) corners[corner][k] = (corner >> k) & 1 ? mx[k] : mn[k];
    PixelRect rect;
    return project_points(origin, ulc, horizontal, vertical, width, height, corners, 8, rect) ? rect : whole;
}

// An untransformed axis-aligned rect as the closest-hit loop tests it (xy_rect.rs:28-48): `axis` is the coordinate its
// plane fixes at k (2: XY, 1: XZ, 0: YZ); a in [a0, a1] and b in [b0, b1] are the other two, in x, y, z order.
struct RectGeo {
    int32_t axis;
    double a0, a1, b0, b1, k;
};

// The first records of the grouped device table (XY, then XZ, then YZ rects: TraceArgs.rect_end) a render gives
// rectangles of their own.  A kernel argument: 16 bytes a record.
enum { RT_PRIMARY_RECTS = 16 };

// Kernel argument of the pooled trace kernel, behind TraceArgs.  r[i] is the rectangle of record i of the device table, in
// table order; the camera batches of an item step over record i < n when no pixel of the item lies inside r[i].  n == 0
// — every rectangle is then the whole frame — says that nothing may be stepped over: the scene's own rectangle is the
// whole frame (ONE decision per render: an aperture, a corner of the scene behind the camera, an ill-conditioned system), the table
// has more rect records than RT_PRIMARY_RECTS, or the table is not one of plain rects only.
struct alignas(8) PrimaryRects {
    int32_t n, _pad;
    PixelRect r[RT_PRIMARY_RECTS];
};

inline bool is_whole_frame(const PixelRect &r, int width, int height) {
    return r.px0 == 0 && r.px1 == width - 1 && r.py0 == 0 && r.py1 == height - 1;
}

// A pixel OUTSIDE the rectangle has no primary ray that can hit the rect: the rectangle of its four corners, with the
// rounding, the pad and the doubts of primary_bounds.  `scene` is primary_bounds of the render: when that is the whole
// frame so is this (the camera's own doubts — an aperture, non-finite vectors, a narrow frame — are all in there).  Any
// doubt about the rect itself (non-finite or reversed bounds, a corner not in front of the camera) gives the whole frame
// for this rect.
inline PixelRect primary_rect_bounds(const double origin[3], const double ulc[3], const double horizontal[3], const double vertical[3],
                                     int width, int height, const PixelRect &scene, const RectGeo &g) {
    const PixelRect whole = {0, width - 1, 0, height - 1};
    if (width < 2 || height < 2 || is_whole_frame(scene, width, height)) return whole;
    if (g.axis < 0 || g.axis > 2) return whole;
    if (!std::isfinite(g.a0) || !std::isfinite(g.a1) || !std::isfinite(g.b0) || !std::isfinite(g.b1) || !std::isfinite(g.k)) return whole;
    if (g.a0 > g.a1 || g.b0 > g.b1) return whole;
    const int ia = g.axis == 0 ? 1 : 0, ib = g.axis == 2 ? 1 : 2; // (rt_trace_common.h: rect_t)
    double corners[4][3];
    for (int corner = 0; corner < 4; ++corner) {
        corners[corner][g.axis] = g.k;
        corners[corner][ia] = corner & 1 ? g.a1 : g.a0;
        corners[corner][ib] = corner & 2 ? g.b1 : g.b0;
    }
    PixelRect rect;
    return project_points(origin, ulc, horizontal, vertical, width, height, corners, 4, rect) ? rect : whole;
}

// The kernel argument of a render: `scene` as above, `rects` the scene's plain rect records in device table order (or
// none: a table that holds anything else).  Nothing is kept between calls.
inline PrimaryRects primary_rects(const double origin[3], const double ulc[3], const double horizontal[3], const double vertical[3],
                                  int width, int height, const PixelRect &scene, const RectGeo *rects, int n_rects) {
    PrimaryRects out;
    out._pad = 0;
    const bool off = n_rects <= 0 || n_rects > RT_PRIMARY_RECTS || width < 2 || height < 2 || is_whole_frame(scene, width, height);
    out.n = off ? 0 : n_rects;
    for (int i = 0; i < RT_PRIMARY_RECTS; ++i)
        out.r[i] = !off && i < n_rects ? primary_rect_bounds(origin, ulc, horizontal, vertical, width, height, scene, rects[i])
                                       : PixelRect{0, width - 1, 0, height - 1};
    return out;
}

} // namespace rtdev
