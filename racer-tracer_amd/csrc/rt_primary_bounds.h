// rt_primary_bounds.h — the pixel rectangle outside which no camera ray of a render can hit the scene.
// The pooled trace kernel skips the camera batches of an 8x8 item none of whose pixels lies inside it (rt_trace_pool_kernel.hip:
// start_item): on a camera that looks at the scene from outside that is every tile beside the scene's projection.
// Plain C++: no HIP header is needed, so the host compiler tests it alone (tests/test_primary_bounds_cpu.py).
#pragma once
#include <cmath>
#include <stdint.h>

namespace rtdev {

// Inclusive: pixel (px, py) is inside when px0 <= px <= px1 and py0 <= py <= py1.  May be empty (px0 > px1 or py0 > py1:
// the box projects beside the frame).
struct PixelRect {
    int32_t px0, px1, py0, py1;
};

// A pixel OUTSIDE the rectangle has no primary ray that can hit anything inside the box [mn, mx].
//
// The ray through (u, v) is ulc + u * horizontal - v * vertical - origin (camera.rs:331); pixel px draws
// u = (px + ju) / (W - 1) with ju in [0, 1) and row py draws v = (py + jv) / (H - 1) likewise (cpu.rs:35-40).  Each of
// the box's corners X is projected by solving (ulc - origin) + u * horizontal - v * vertical = lambda * (X - origin)
// for (u, v, lambda); with every corner strictly in front of the camera (lambda > 0) the map is a perspective one, the
// box's image is the hull of the corners' and px sees the box only if px + 1 > Umin and px <= Umax, U = u * (W - 1).
// The rectangle is rounded outward and padded by a whole pixel: at the distances of a scene a pixel is a fraction of a
// scene unit, a dozen orders of magnitude above any rounding here or in the device's primitive tests.
//
// Conservative by construction: in every doubtful case the answer is the whole frame ("cull off") — a corner on or
// behind the camera plane (which covers a camera inside the box), a singular or ill-conditioned system, anything
// non-finite, an empty box, a frame narrower than two pixels, and an aperture (the origins of its rays differ per sample).
inline PixelRect primary_bounds(const double origin[3], const double ulc[3], const double horizontal[3], const double vertical[3],
                                double lens_radius, int width, int height, const double mn[3], const double mx[3]) {
    const PixelRect whole = {0, width - 1, 0, height - 1};
    const double kPad = 1.0; // pixels
    if (width < 2 || height < 2) return whole;
    if (!(lens_radius == 0.0)) return whole;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(origin[k]) || !std::isfinite(ulc[k]) || !std::isfinite(horizontal[k]) || !std::isfinite(vertical[k]))
            return whole;
        if (!std::isfinite(mn[k]) || !std::isfinite(mx[k]) || mn[k] > mx[k]) return whole;
    }
    // columns of the system: a = horizontal, b = -vertical, c = -(X - origin); right-hand side r = origin - ulc
    const double a[3] = {horizontal[0], horizontal[1], horizontal[2]};
    const double b[3] = {-vertical[0], -vertical[1], -vertical[2]};
    const double r[3] = {origin[0] - ulc[0], origin[1] - ulc[1], origin[2] - ulc[2]};
    auto det3 = [](const double p[3], const double q[3], const double s[3]) {
        return p[0] * (q[1] * s[2] - q[2] * s[1]) - p[1] * (q[0] * s[2] - q[2] * s[0]) + p[2] * (q[0] * s[1] - q[1] * s[0]);
    };
    auto norm3 = [](const double p[3]) { return std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]); };
    double u_min = INFINITY, u_max = -INFINITY, v_min = INFINITY, v_max = -INFINITY;
    for (int corner = 0; corner < 8; ++corner) {
        double c[3];
        for (int k = 0; k < 3; ++k) c[k] = -(((corner >> k) & 1 ? mx[k] : mn[k]) - origin[k]);
        const double det = det3(a, b, c);
        // (ill-conditioned: the three columns nearly in one plane — the corner nearly in the plane through the camera that
        // the image plane is parallel to, or a degenerate camera)
        if (!std::isfinite(det) || !(std::fabs(det) > 1e-9 * norm3(a) * norm3(b) * norm3(c))) return whole;
        const double u = det3(r, b, c) / det, v = det3(a, r, c) / det, lambda = det3(a, b, r) / det;
        if (!std::isfinite(u) || !std::isfinite(v) || !std::isfinite(lambda) || !(lambda > 0.0)) return whole;
        u_min = std::fmin(u_min, u);
        u_max = std::fmax(u_max, u);
        v_min = std::fmin(v_min, v);
        v_max = std::fmax(v_max, v);
    }
    // outward rounding, the pad, and a clamp to the frame's neighbourhood in double (the integers cannot overflow)
    auto low = [&](double t, int n) { return (int32_t)std::fmin(std::fmax(std::floor(t * (double)(n - 1)) - 1.0 - kPad, 0.0), (double)n); };
    auto high = [&](double t, int n) { return (int32_t)std::fmax(std::fmin(std::ceil(t * (double)(n - 1)) + kPad, (double)(n - 1)), -1.0); };
    return PixelRect{low(u_min, width), high(u_max, width), low(v_min, height), high(v_max, height)};
}

} // namespace rtdev
