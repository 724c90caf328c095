"""numpy restatement of csrc/rt_temporal.hip: the definition the temporal kernels are held to.

A history is a dict of numpy planes — radiance [H, W, 3], moments [H, W, 2], length [H, W], normal, position [H, W, 3] f64,
obj_id [H, W] int32; guides are denoise_model's.  The arithmetic follows the kernels' order (history taps j, then i; the 7x7
window and the a-trous taps dy, then dx), so the two agree to rounding.  accumulate() also returns, per pixel, the MARGIN:
the smallest relative distance of any of its decisions (the range tests of the re-projection, each tap's normal and plane
test, the Wsum test, the length >= 4 test of the variance) from its threshold.  A pixel with a tiny margin may legitimately
fall on the other side on the device, so the tests leave those out — and check that there are next to none.
"""
import math

import numpy as np

import denoise_model as M

DEMODULATE = M.DEMODULATE
LUMA = (0.2126, 0.7152, 0.0722)
PLANES = ("radiance", "moments", "length", "normal", "position", "obj_id")
DEFAULTS = dict(alpha=0.2, alpha_moments=0.2, max_history=32.0, normal_tolerance=0.25, plane_tolerance=2.0,
                sigma_luminance=4.0)


def luminance(c):
    return LUMA[0] * c[..., 0] + LUMA[1] * c[..., 1] + LUMA[2] * c[..., 2]


def demodulate(rgb, guides, flags=DEMODULATE):
    """C = g^2 / max(albedo, 1e-3), or g^2: denoise_model.denoise's first step."""
    rgb = np.asarray(rgb, dtype=np.float64)
    L = rgb * rgb
    return L / np.maximum(guides["albedo"], 1e-3) if flags & DEMODULATE else L


def camera_vectors(cam):
    """(o, ulc, hor, ver) of an abi.RtCamera."""
    return (np.array(cam.origin[:]), np.array(cam.upper_left_corner[:]), np.array(cam.horizontal[:]),
            np.array(cam.vertical[:]))


def orbit(cam, degrees):
    """A camera dict (scenes_py) turned about the vertical axis through its look_at."""
    a = math.radians(degrees)
    f, t = np.array(cam["look_from"], dtype=float), np.array(cam["look_at"], dtype=float)
    d = f - t
    r = np.array([d[0] * math.cos(a) + d[2] * math.sin(a), d[1], -d[0] * math.sin(a) + d[2] * math.cos(a)])
    return dict(cam, look_from=tuple(float(v) for v in t + r))


def reproject(position, prev_cam, width, height):
    """(fx, fy, s, det) of every pixel's hit point through the previous camera: ulc + u hor - v ver - o = s (x - o) by
    Cramer's rule on the columns hor, -ver, -(x - o) against o - ulc."""
    o, ulc, hor, ver = prev_cam
    a, b, r = hor, -ver, o - ulc
    c = -(position - o)
    bxc = np.cross(b, c)
    det = bxc @ a
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (bxc @ r) / det
        v = (np.cross(r, c) @ a) / det
        s = (np.cross(b, r) @ a) * np.ones_like(det) / det
    return u * (width - 1) - 0.5, v * (height - 1) - 0.5, s, det


def _rel(a, b):
    """|a - b| / max(|a|, |b|): the relative distance of a from its threshold b (1 where both are 0)."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=float), np.asarray(b, dtype=float))
    m = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(m > 0, np.abs(a - b) / m, 1.0)


def first_history(rgb, guides, flags=DEMODULATE):
    return accumulate(rgb, guides, None, None, flags=flags)[0]


def accumulate(rgb, guides, prev, prev_cam, flags=DEMODULATE, alpha=0.2, alpha_moments=0.2, max_history=32.0,
               normal_tolerance=0.25, plane_tolerance=2.0, **_unused):
    """One accumulation -> (history, info); info: fresh [H, W] bool (the pixel starts afresh), margin [H, W], taps [H, W]
    (valid history taps), shift (fx - x, fy - y)."""
    C = demodulate(rgb, guides, flags)
    h, w = C.shape[:2]
    l = luminance(C)
    ids, n, x, fp = guides["obj_id"], guides["normal"], guides["position"], guides["footprint"]
    out = {"radiance": C.copy(), "moments": np.stack([l, l * l], axis=-1), "length": np.ones((h, w)),
           "normal": n.copy(), "position": x.copy(), "obj_id": ids.copy()}
    fresh = np.ones((h, w), dtype=bool)
    margin = np.ones((h, w))
    info = {"fresh": fresh, "margin": margin, "taps": np.zeros((h, w), dtype=int), "shift": None}
    if prev is not None:
        hit = ids >= 0
        fx, fy, s, det = reproject(x, prev_cam, w, h)
        with np.errstate(invalid="ignore"):
            finite = np.isfinite(fx) & np.isfinite(fy)
            inside = hit & (det != 0.0) & (s > 0.0) & finite & (fx >= -1.0) & (fx <= w) & (fy >= -1.0) & (fy <= h)
        # margins of the range tests (absolute distances in pixels, relative for s)
        o, ulc, hor, ver = prev_cam
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
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        info["shift"] = (fx - xs, fy - ys)
        ch = np.zeros_like(C)
        mh = np.zeros((h, w, 2))
        lh = np.zeros((h, w))
        wsum = np.zeros((h, w))
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
                    tm = np.minimum(_rel(dn2, ntol2), _rel(dist, np.where(np.isfinite(lim), lim, 1.0)))
                margin[ok] = np.minimum(margin, tm)[ok]
                wt = np.where(valid, (tx if i else 1.0 - tx) * (ty if j else 1.0 - ty), 0.0)
                ch = ch + wt[..., None] * prev["radiance"][qy, qx]
                mh = mh + wt[..., None] * prev["moments"][qy, qx]
                lh = lh + wt * prev["length"][qy, qx]
                wsum = wsum + wt
                info["taps"] += valid
        margin[inside] = np.minimum(margin, _rel(wsum, 1e-3))[inside]
        cont = inside & (wsum >= 1e-3)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / wsum
            N = lh * inv + 1.0
            a = np.maximum(1.0 / N, alpha)
            am = np.maximum(1.0 / N, alpha_moments)
            rad = (1.0 - a)[..., None] * (ch * inv[..., None]) + a[..., None] * C
            mom = (1.0 - am)[..., None] * (mh * inv[..., None]) + am[..., None] * out["moments"]
            length = np.minimum(N, max_history)
        out["radiance"][cont] = rad[cont]
        out["moments"][cont] = mom[cont]
        out["length"][cont] = length[cont]
        fresh[cont] = False
    hit = ids >= 0
    margin[hit] = np.minimum(margin, _rel(out["length"], 4.0))[hit]
    return out, info


def variance(history, guides, sigma_normal=0.1, sigma_plane=1.0):
    """The variance of the accumulated luminance [H, W]: 0 on a miss, (m2 - m1^2) / length where length >= 4, else the
    7x7 neighbourhood's under the object, normal and plane weights at step 1."""
    rad, mom, length = history["radiance"], history["moments"], history["length"]
    h, w = length.shape
    ids, n, x, fp = guides["obj_id"], guides["normal"], guides["position"], guides["footprint"]
    lum = luminance(rad)
    inv_sn2 = 1.0 / (sigma_normal * sigma_normal) if sigma_normal > 0 else 0.0
    inv_sx = 1.0 / sigma_plane if sigma_plane > 0 else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_fx = inv_sx / fp
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    s0, s1, s2 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            qy, qx = ys + dy, xs + dx
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            use = inside & (ids[qy, qx] == ids)
            wt = np.ones((h, w))
            with np.errstate(invalid="ignore", over="ignore"):
                if inv_sn2 > 0:
                    wt = wt * np.exp(-np.sum((n - n[qy, qx]) ** 2, axis=-1) * inv_sn2)
                if inv_sx > 0:
                    dist = np.sum(n * (x[qy, qx] - x), axis=-1) * inv_fx
                    wt = wt * np.exp(-(dist * dist))
            wt = np.where(use, wt, 0.0)
            lq = lum[qy, qx]
            s0 = s0 + wt
            s1 = s1 + wt * lq
            s2 = s2 + wt * (lq * lq)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = s1 / s0
        spatial = np.maximum(0.0, s2 / s0 - mean * mean)
        temporal = np.maximum(0.0, mom[..., 1] - mom[..., 0] * mom[..., 0]) / length
    var = np.where(length >= 4.0, temporal, spatial)
    var[ids < 0] = 0.0
    return var


def gauss3(var):
    """The 3x3 Gaussian (1/4, 1/8, 1/16) at step 1 over the taps inside the image, renormalised."""
    h, w = var.shape
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    vs, vw = np.zeros((h, w)), np.zeros((h, w))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qy, qx = ys + dy, xs + dx
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            k = (0.5 if dx == 0 else 0.25) * (0.5 if dy == 0 else 0.25)
            vs = vs + np.where(inside, k * var[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)], 0.0)
            vw = vw + np.where(inside, k, 0.0)
    return vs / vw


def atrous_var(I, var, guides, i, sigma_color=0.0, sigma_normal=0.0, sigma_plane=0.0, sigma_luminance=0.0):
    """One variance-guided level (step 2^i) over radiance I [H, W, 3] and its variance [H, W] -> (I', var')."""
    h, w = I.shape[:2]
    step = 1 << i
    ids, n, x, fp = guides["obj_id"], guides["normal"], guides["position"], guides["footprint"]
    inv_sn2 = 1.0 / (sigma_normal * sigma_normal) if sigma_normal > 0 else 0.0
    inv_sx = 1.0 / (sigma_plane * step) if sigma_plane > 0 else 0.0
    sc = math.ldexp(sigma_color, -i) if sigma_color > 0 else 0.0
    inv_sc2 = 1.0 / (sc * sc) if sc > 0 else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_fx = inv_sx / fp
        sp = np.sqrt(I)
    lum = luminance(I)
    inv_sl = 1.0 / (sigma_luminance * np.sqrt(gauss3(var)) + 1e-10) if sigma_luminance > 0 else None
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    acc = np.zeros_like(I)
    wsum, vsum = np.zeros((h, w)), np.zeros((h, w))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            qy, qx = ys + dy * step, xs + dx * step
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            use = inside & (ids[qy, qx] == ids)
            wt = np.full((h, w), M.H5[dx + 2] * M.H5[dy + 2])
            with np.errstate(invalid="ignore", over="ignore"):
                if inv_sn2 > 0:
                    wt = wt * np.exp(-np.sum((n - n[qy, qx]) ** 2, axis=-1) * inv_sn2)
                if inv_sx > 0:
                    dist = np.sum(n * (x[qy, qx] - x), axis=-1) * inv_fx
                    wt = wt * np.exp(-(dist * dist))
                if inv_sc2 > 0:
                    wt = wt * np.exp(-np.sum((sp - sp[qy, qx]) ** 2, axis=-1) * inv_sc2)
                if inv_sl is not None:
                    wt = wt * np.exp(-np.abs(lum - lum[qy, qx]) * inv_sl)
            wt = np.where(use, wt, 0.0)
            acc = acc + wt[..., None] * I[qy, qx]
            wsum = wsum + wt
            vsum = vsum + (wt * wt) * var[qy, qx]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / wsum
        out = acc * inv[..., None]
        var_out = vsum * (inv * inv)
    miss = ids < 0
    out[miss] = I[miss]
    var_out[miss] = var[miss]
    return out, var_out


def denoise_history(history, guides, iterations=5, flags=DEMODULATE, sigma_color=0.0, sigma_normal=0.1, sigma_plane=1.0,
                    sigma_luminance=4.0):
    """rt_denoise_history_device: variance, the levels, sqrt(max(I * albedo, 0)) -> the gamma-encoded frame [H, W, 3]."""
    I = history["radiance"]
    if sigma_luminance > 0 and iterations > 0:
        var = variance(history, guides, sigma_normal, sigma_plane)
        for i in range(iterations):
            I, var = atrous_var(I, var, guides, i, sigma_color, sigma_normal, sigma_plane, sigma_luminance)
    else:
        for i in range(iterations):
            I = M.atrous(I, guides, i, sigma_color, sigma_normal, sigma_plane)
    L = I * guides["albedo"] if flags & DEMODULATE else I
    return np.sqrt(np.maximum(L, 0.0))


def temporal_kwargs(tp):
    """An abi.RtTemporalParams as accumulate()'s keyword arguments."""
    return dict(alpha=tp.alpha, alpha_moments=tp.alpha_moments, max_history=tp.max_history,
                normal_tolerance=tp.normal_tolerance, plane_tolerance=tp.plane_tolerance)
