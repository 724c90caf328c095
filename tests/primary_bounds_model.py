"""A numpy model around racer-tracer_amd/csrc/rt_primary_bounds.h, shared by tests/test_primary_bounds_cpu.py and
tests/test_gpu_primary_cull.py: the camera of camera.rs:196-234, the rays of cpu.rs:35-40 / camera.rs:331, a slab test, and
the rectangle itself from projections by dot products (the header solves a 3x3 system per corner instead)."""
import math

import numpy as np

CORNELL_BOX = ((0.0, 0.0, 0.0), (555.0, 555.0, 555.0))
C3_CAMERA = dict(look_from=(278.0, 278.0, -800.0), look_at=(278.0, 278.0, 0.0), vfov=40.0, aperture=0.0, focus_distance=10000.0)


def camera(look_from, look_at, vfov, aperture, focus_distance, width, height, scene_up=(0.0, 1.0, 0.0)):
    """-> dict(origin, ulc, horizontal, vertical, forward, lens_radius), float64 vectors (camera.rs:196-234)."""
    look_from, look_at, scene_up = (np.asarray(v, dtype=np.float64) for v in (look_from, look_at, scene_up))
    h = math.tan(math.radians(vfov) / 2.0)
    viewport_height = 2.0 * h
    viewport_width = (float(width) / float(height)) * viewport_height
    forward = look_from - look_at
    forward = forward / np.linalg.norm(forward)
    right = np.cross(scene_up, forward)
    right = right / np.linalg.norm(right)
    up = np.cross(forward, right)
    horizontal = focus_distance * viewport_width * right
    vertical = focus_distance * viewport_height * up
    ulc = look_from + vertical / 2.0 - horizontal / 2.0 - focus_distance * forward
    return dict(origin=look_from, ulc=ulc, horizontal=horizontal, vertical=vertical, forward=forward, lens_radius=aperture * 0.5)


def case_line(cam, width, height, mn, mx, lens_radius=None):
    """One case of tests/primary_bounds_driver.cpp (hexadecimal floats: the doubles themselves)."""
    def fmt(x):
        x = float(x)
        return "nan" if math.isnan(x) else ("inf" if x > 0 else "-inf") if math.isinf(x) else x.hex()
    lr = cam["lens_radius"] if lens_radius is None else lens_radius
    vals = list(cam["origin"]) + list(cam["ulc"]) + list(cam["horizontal"]) + list(cam["vertical"]) + [lr, width, height] + list(mn) + list(mx)
    return " ".join(fmt(v) for v in vals)


def rays_hit_box(cam, u, v, mn, mx):
    """Slab test of the rays through every (u[i], v[j]) against the box, t > 0 -> number of rays that hit."""
    return sum(int(_rays_hit_box(cam, u[i:i + 128], v, mn, mx).sum()) for i in range(0, len(u), 128))


def _rays_hit_box(cam, u, v, mn, mx):
    d = (cam["ulc"][None, None, :] + u[:, None, None] * cam["horizontal"][None, None, :]
         - v[None, :, None] * cam["vertical"][None, None, :] - cam["origin"][None, None, :])
    o = cam["origin"]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        t1 = (np.asarray(mn) - o) * inv
        t2 = (np.asarray(mx) - o) * inv
    t_near = np.fmax.reduce(np.fmin(t1, t2), axis=-1)   # (fmin / fmax drop a NaN of 0 * inf: towards a hit)
    t_far = np.fmin.reduce(np.fmax(t1, t2), axis=-1)
    return t_far >= np.fmax(t_near, 0.0)


JITTERS = (0.0, 0.5, 1.0 - 2.0 ** -53)


def pixel_samples(indices, n):
    """u (or v) of the pixels `indices` of an n-pixel axis at every jitter of JITTERS, flattened."""
    idx = np.asarray(indices, dtype=np.float64)
    return np.concatenate([(idx + j) / float(n - 1) for j in JITTERS]) if len(idx) else np.zeros(0)


def outside_rays_that_hit(cam, width, height, rect, mn, mx):
    """Number of sampled rays of pixel columns and rows OUTSIDE `rect` (px0, px1, py0, py1) that hit the box grown by
    1e-9 of its extent: every outside column against every row of the frame, every outside row against every column."""
    px0, px1, py0, py1 = rect
    mn, mx = np.asarray(mn, dtype=np.float64), np.asarray(mx, dtype=np.float64)
    grow = 1e-9 * (mx - mn)
    lo, hi = mn - grow, mx + grow
    cols = [x for x in range(width) if x < px0 or x > px1]
    rows = [y for y in range(height) if y < py0 or y > py1]
    bad = 0
    if cols:
        bad += rays_hit_box(cam, pixel_samples(cols, width), pixel_samples(range(height), height), lo, hi)
    if rows:
        bad += rays_hit_box(cam, pixel_samples(range(width), width), pixel_samples(rows, height), lo, hi)
    return bad


def model_rect(cam, width, height, mn, mx, pad=1):
    """The rectangle by dot products: a corner X in front of the camera (depth = -(X - origin) . forward > 0) projects to
    the image plane at the focus distance.  None when some corner is not in front (or the camera has an aperture)."""
    if cam["lens_radius"] != 0.0:
        return None
    right = cam["horizontal"] / np.linalg.norm(cam["horizontal"])
    up = cam["vertical"] / np.linalg.norm(cam["vertical"])
    focus = float(np.dot(cam["origin"] - cam["ulc"], cam["forward"]))   # ulc lies focus_distance in front of the origin
    us, vs = [], []
    for k in range(8):
        x = np.array([(mx if (k >> a) & 1 else mn)[a] for a in range(3)], dtype=np.float64) - cam["origin"]
        depth = -float(np.dot(x, cam["forward"]))
        if not depth > 0.0:
            return None
        p = cam["origin"] + x * (focus / depth) - cam["ulc"]   # the corner's image, relative to the upper left corner
        us.append(float(np.dot(p, right)) / float(np.linalg.norm(cam["horizontal"])))
        vs.append(-float(np.dot(p, up)) / float(np.linalg.norm(cam["vertical"])))
    return (max(0, math.floor(min(us) * (width - 1)) - 1 - pad), min(width - 1, math.ceil(max(us) * (width - 1)) + pad),
            max(0, math.floor(min(vs) * (height - 1)) - 1 - pad), min(height - 1, math.ceil(max(vs) * (height - 1)) + pad))


def tiles_outside(rect, width, height):
    """(8x8 tiles without a pixel inside rect, tiles of the frame)."""
    px0, px1, py0, py1 = rect
    tx, ty = (width + 7) // 8, (height + 7) // 8
    n = 0
    for j in range(ty):
        for i in range(tx):
            x0, x1, y0, y1 = i * 8, min(i * 8 + 7, width - 1), j * 8, min(j * 8 + 7, height - 1)
            if x1 < px0 or x0 > px1 or y1 < py0 or y0 > py1:
                n += 1
    return n, tx * ty
