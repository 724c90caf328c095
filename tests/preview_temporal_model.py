"""numpy restatement of csrc/rt_preview_temporal.hip: the definition k_preview_accumulate is held to.

Built on temporal_model (histories, the re-projection, demodulation, the resolve) and upsample_model (the grid).  The
arithmetic follows the kernel's order: history taps j, then i; the fill's anchors (j0, i0) (j0, i1) (j1, i0) (j1, i1).
Like temporal_model.accumulate, accumulate() returns every pixel's MARGIN: the smallest relative distance of any of its
decisions (the range tests of the re-projection, each tap's normal and plane test, the Wsum test, the length >= 4 test
of the resolve's variance) from its threshold.  The decisions that 4.14 adds have no margin to speak of: sampled(p) and
the fill's b == 0 are integer facts, and a tap's length > 0 compares a stored value (a fill's length is exactly 0.0).
"""
import numpy as np

import temporal_model as T
import upsample_model as U

DEMODULATE = T.DEMODULATE
preview_grid = U.preview_grid


def phase(step_x, step_y, frame_index):
    """(jx, jy) of a frame: i = (k g) mod n with k = frame_index mod n and g the smallest integer >= max(1, (5 n + 4) // 8)
    coprime to n; jx = i mod step_x, jy = i // step_x."""
    n = step_x * step_y
    g = max(1, (5 * n + 4) // 8)
    while np.gcd(g, n) != 1:
        g += 1
    i = ((frame_index % n) * g) % n
    return i % step_x, i // step_x


def phase_camera_corner(cam, width, height, jx, jy):
    """The upper_left_corner of the phase camera of an abi.RtCamera, per component as DESIGN.md 4.14 writes it."""
    _, ulc, hor, ver = T.camera_vectors(cam)
    if (jx, jy) == (0, 0):
        return ulc
    return ulc + ((jx / (width - 1)) * hor - (jy / (height - 1)) * ver)


def sampled_mask(h, w, step_x, step_y, jx, jy):
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cw, ch = (w // step_x) * step_x, (h // step_y) * step_y
    return (xs < cw) & (ys < ch) & (xs % step_x == jx) & (ys % step_y == jy)


def replicate_phase(full, step_x, step_y, jx, jy):
    """The preview frame of phase (jx, jy) of a full-resolution frame: every block holds its pixel (jx, jy), the uncovered
    edges are 0 (what rt_render_frame writes with the phase camera)."""
    h, w = full.shape[:2]
    cw, ch = (w // step_x) * step_x, (h // step_y) * step_y
    out = np.zeros_like(full)
    ys, xs = np.arange(ch), np.arange(cw)
    out[:ch, :cw] = full[(ys - ys % step_y + jy)[:, None], (xs - xs % step_x + jx)[None, :]]
    return out


def history_value(guides, prev, prev_cam, normal_tolerance=0.25, plane_tolerance=2.0):
    """4.11's re-projection and taps with the one more condition length'_q > 0 -> (has [H, W] bool, ch [H, W, 3],
    mh [H, W, 2], lh [H, W], wsum [H, W], margin [H, W], taps [H, W]): the taps' weighted sums and their weight where
    `has`.  temporal_model.accumulate's statements, in its order."""
    ids, n, x, fp = guides["obj_id"], guides["normal"], guides["position"], guides["footprint"]
    h, w = ids.shape
    margin = np.ones((h, w))
    taps = np.zeros((h, w), dtype=int)
    ch, mh, lh, wsum = np.zeros((h, w, 3)), np.zeros((h, w, 2)), np.zeros((h, w)), np.zeros((h, w))
    if prev is None:
        return np.zeros((h, w), dtype=bool), ch, mh, lh, wsum, margin, taps
    hit = ids >= 0
    fx, fy, s, det = T.reproject(x, prev_cam, w, h)
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(fx) & np.isfinite(fy)
        inside = hit & (det != 0.0) & (s > 0.0) & finite & (fx >= -1.0) & (fx <= w) & (fy >= -1.0) & (fy <= h)
    o, _, hor, ver = prev_cam
    scale = np.linalg.norm(hor) * np.linalg.norm(ver) * np.linalg.norm(x - o, axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mg = np.minimum.reduce([np.abs(det) / np.maximum(scale, 1e-300), np.abs(s),
                                np.abs(fx + 1.0), np.abs(fx - w), np.abs(fy + 1.0), np.abs(fy - h)])
    mg = np.where(np.isfinite(mg), mg, 1.0)
    margin[hit] = np.minimum(margin, mg)[hit]
    fxs, fys = np.where(inside, fx, 0.0), np.where(inside, fy, 0.0)
    x0, y0 = np.floor(fxs), np.floor(fys)
    tx, ty = fxs - x0, fys - y0
    x0, y0 = x0.astype(int), y0.astype(int)
    ntol2 = normal_tolerance * normal_tolerance
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            ok = inside & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            ok &= prev["obj_id"][qy, qx] == ids
            dn = n - prev["normal"][qy, qx]
            dn2 = np.sum(dn * dn, axis=-1)
            dist = np.abs(np.sum(n * (prev["position"][qy, qx] - x), axis=-1))
            with np.errstate(invalid="ignore"):
                lim = plane_tolerance * fp
                valid = ok & (dn2 <= ntol2) & (dist <= lim)
                tm = np.minimum(T._rel(dn2, ntol2), T._rel(dist, np.where(np.isfinite(lim), lim, 1.0)))
            margin[ok] = np.minimum(margin, tm)[ok]
            with np.errstate(invalid="ignore"):
                valid &= prev["length"][qy, qx] > 0.0   # a fill is never read as history
            wt = np.where(valid, (tx if i else 1.0 - tx) * (ty if j else 1.0 - ty), 0.0)
            ch = ch + wt[..., None] * np.where(valid[..., None], prev["radiance"][qy, qx], 0.0)
            mh = mh + wt[..., None] * np.where(valid[..., None], prev["moments"][qy, qx], 0.0)
            lh = lh + wt * np.where(valid, prev["length"][qy, qx], 0.0)
            wsum = wsum + wt
            taps += valid
    margin[inside] = np.minimum(margin, T._rel(wsum, 1e-3))[inside]
    has = inside & (wsum >= 1e-3)
    return has, ch, mh, lh, wsum, margin, taps


def _axis(x, j, step, count):
    """(i0, i1, t) of DESIGN.md 4.14 for one coordinate array: the anchors of column i sit at i step + j."""
    xs = x - j
    i0 = np.where(xs < 0, 0, np.minimum(np.maximum(xs, 0) // step, count - 1))
    i1 = np.minimum(i0 + 1, count - 1)
    t = np.where((xs < 0) | (i1 == i0), 0.0, (xs - i0 * step) / float(step))
    return i0, i1, t


def fill(rgb, guides, step_x, step_y, jx, jy, flags=DEMODULATE, sigma_normal=0.1, sigma_plane=1.0):
    """4.13's blend on the grid shifted by the phase, before its re-modulation and square root -> radiance [H, W, 3] of
    every pixel (accumulate() keeps it where a pixel is neither sampled nor has a history)."""
    rgb = np.asarray(rgb, dtype=np.float64)
    h, w = rgb.shape[:2]
    gx, gy = w // step_x, h // step_y
    ids, n, x, fp, albedo = (guides[k] for k in ("obj_id", "normal", "position", "footprint", "albedo"))
    demod = bool(flags & DEMODULATE)
    inv_sn2 = 1.0 / (sigma_normal * sigma_normal) if sigma_normal > 0 else 0.0
    inv_sx = 1.0 / (sigma_plane * max(step_x, step_y)) if sigma_plane > 0 else 0.0
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    i0, i1, tx = _axis(xs, jx, step_x, gx)
    j0, j1, ty = _axis(ys, jy, step_y, gy)
    with np.errstate(divide="ignore"):
        inv_fx = inv_sx / fp   # a miss has footprint inf: 0
    acc, wsum = np.zeros((h, w, 3)), np.zeros((h, w))
    for jj, by in ((j0, 1.0 - ty), (j1, ty)):
        for ii, bx in ((i0, 1.0 - tx), (i1, tx)):
            b = by * bx
            ay, ax = jj * step_y, ii * step_x   # the block's top-left pixel: the colour
            qy, qx = ay + jy, ax + jx           # the pixel the anchor traced: the guides
            use = (b != 0.0) & (ids[qy, qx] == ids)
            wt = b
            with np.errstate(invalid="ignore", over="ignore"):
                if inv_sn2 > 0:
                    dn = n - n[qy, qx]
                    wt = wt * np.exp(-(dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1] + dn[..., 2] * dn[..., 2]) * inv_sn2)
                if inv_sx > 0:
                    dx = x[qy, qx] - x
                    dist = (n[..., 0] * dx[..., 0] + n[..., 1] * dx[..., 1] + n[..., 2] * dx[..., 2]) * inv_fx
                    wt = wt * np.exp(-(dist * dist))
            wt = np.where(use, wt, 0.0)
            v = rgb[ay, ax] * rgb[ay, ax]
            if demod:
                v = v / np.maximum(albedo[qy, qx], 1e-3)
            acc = acc + wt[..., None] * np.where(use[..., None], v, 0.0)
            wsum = wsum + wt
    # no anchor qualifies: the frame at p, or outside the cover (where the frame holds 0) at the nearest covered pixel
    own = rgb[np.minimum(ys, gy * step_y - 1), np.minimum(xs, gx * step_x - 1)]
    own = own * own
    if demod:
        own = own / np.maximum(albedo, 1e-3)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((wsum > 0.0)[..., None], acc / wsum[..., None], own)


def accumulate(rgb, guides, prev, prev_cam, step_x, step_y, jx, jy, flags=DEMODULATE, alpha=0.2, alpha_moments=0.2,
               max_history=32.0, normal_tolerance=0.25, plane_tolerance=2.0, sigma_normal=0.1, sigma_plane=1.0, **_unused):
    """One accumulation of the preview frame rgb [H, W, 3] of phase (jx, jy) -> (history, info); info: sampled, fresh
    (sampled without history), carried, fill [H, W] bool, margin [H, W], taps [H, W]."""
    C = T.demodulate(rgb, guides, flags)
    h, w = C.shape[:2]
    l = T.luminance(C)
    ids = guides["obj_id"]
    sampled = sampled_mask(h, w, step_x, step_y, jx, jy)
    has, ch, mh, lh, wsum, margin, taps = history_value(guides, prev, prev_cam, normal_tolerance, plane_tolerance)
    out = {"radiance": C.copy(), "moments": np.stack([l, l * l], axis=-1), "length": np.ones((h, w)),
           "normal": guides["normal"].copy(), "position": guides["position"].copy(), "obj_id": ids.copy()}
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / wsum
        N = lh * inv + 1.0
        a = np.maximum(1.0 / N, alpha)
        am = np.maximum(1.0 / N, alpha_moments)
        rad = (1.0 - a)[..., None] * (ch * inv[..., None]) + a[..., None] * C
        mom = (1.0 - am)[..., None] * (mh * inv[..., None]) + am[..., None] * out["moments"]
        length = np.minimum(N, max_history)
        carried_rad, carried_mom, carried_len = ch * inv[..., None], mh * inv[..., None], lh / wsum
    blend, carried, filled = sampled & has, ~sampled & has, ~sampled & ~has
    out["radiance"][blend], out["moments"][blend], out["length"][blend] = rad[blend], mom[blend], length[blend]
    out["radiance"][carried], out["moments"][carried] = carried_rad[carried], carried_mom[carried]
    out["length"][carried] = carried_len[carried]
    if filled.any():
        F = fill(rgb, guides, step_x, step_y, jx, jy, flags, sigma_normal, sigma_plane)
        lf = T.luminance(F)
        out["radiance"][filled] = F[filled]
        out["moments"][filled] = np.stack([lf, lf * lf], axis=-1)[filled]
        out["length"][filled] = 0.0
    hit = ids >= 0
    margin[hit] = np.minimum(margin, T._rel(out["length"], 4.0))[hit]
    return out, {"sampled": sampled, "fresh": sampled & ~has, "carried": carried, "fill": filled, "margin": margin,
                 "taps": taps}


def resolve(history, guides, **kw):
    """rt_denoise_history_device on the history (temporal_model.denoise_history's keywords)."""
    return T.denoise_history(history, guides, **kw)
