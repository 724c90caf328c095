"""numpy restatement of the preview upsampler of csrc/rt_upsample.hip: the definition the device kernel is
held to.  Plain loops over pixels and taps, in the kernel's order; the guides, mismatch and gamma_rmse are denoise_model's.

rgb: the replicated preview frame [H, W, 3] (what rt_render_frame writes with scale > 1; only its anchor pixels are
read).  guides: full-resolution planes as Scene.render_guides returns them.
"""
import math

import numpy as np

from denoise_model import DEMODULATE, gamma_rmse, mismatch, oracle_guides, synthetic_frame, synthetic_guides  # noqa: F401


def preview_grid(width, height, tiles_w, tiles_h, scale):
    """(step_x, step_y, cover_w, cover_h): step = the largest divisor <= scale of size / max(tiles, 1) (cpu_scaled.rs:18-41)."""
    if scale <= 1:
        return 1, 1, width, height

    def highest_divisible(value, div):
        while value % div != 0:
            div -= 1
        return div
    sx = highest_divisible(width // max(tiles_w, 1), scale)
    sy = highest_divisible(height // max(tiles_h, 1), scale)
    return sx, sy, (width // sx) * sx, (height // sy) * sy


def replicate(full, step_x, step_y, cover_w, cover_h):
    """The preview frame of a full-resolution frame: every block holds its top-left pixel, the uncovered edges are 0."""
    h, w = full.shape[:2]
    out = np.zeros_like(full)
    ys, xs = np.arange(cover_h), np.arange(cover_w)
    out[:cover_h, :cover_w] = full[(ys - ys % step_y)[:, None], (xs - xs % step_x)[None, :]]
    return out


def _axis(x, step, count):
    """(i0, i1, t) of DESIGN.md 4.13 for one coordinate."""
    i0 = min(x // step, count - 1)
    i1 = min(i0 + 1, count - 1)
    t = float(x - i0 * step) / float(step) if i1 != i0 else 0.0
    return i0, i1, t


def upsample(rgb, guides, step_x, step_y, flags=DEMODULATE, sigma_normal=0.1, sigma_plane=1.0):
    """The replicated preview frame rgb [H, W, 3] upsampled with full-resolution guides -> [H, W, 3]."""
    rgb = np.asarray(rgb, dtype=np.float64)
    h, w = rgb.shape[:2]
    gx, gy = w // step_x, h // step_y
    ids, n, x, fp, albedo = (guides[k] for k in ("obj_id", "normal", "position", "footprint", "albedo"))
    demodulate = bool(flags & DEMODULATE)
    inv_sn2 = 1.0 / (sigma_normal * sigma_normal) if sigma_normal > 0 else 0.0
    inv_sx = 1.0 / (sigma_plane * max(step_x, step_y)) if sigma_plane > 0 else 0.0
    out = np.zeros_like(rgb)
    for py in range(h):
        j0, j1, ty = _axis(py, step_y, gy)
        for px in range(w):
            i0, i1, tx = _axis(px, step_x, gx)
            inv_fx = float(inv_sx / fp[py, px])   # a miss has footprint inf: 0
            acc = np.zeros(3)
            wsum = 0.0
            for j, by in ((j0, 1.0 - ty), (j1, ty)):
                for i, bx in ((i0, 1.0 - tx), (i1, tx)):
                    b = by * bx
                    qy, qx = j * step_y, i * step_x
                    if b == 0.0 or ids[qy, qx] != ids[py, px]:
                        continue
                    wt = b
                    if inv_sn2 > 0:
                        dn = n[py, px] - n[qy, qx]
                        wt *= math.exp(-float(dn[0] * dn[0] + dn[1] * dn[1] + dn[2] * dn[2]) * inv_sn2)
                    if inv_sx > 0:
                        dx = x[qy, qx] - x[py, px]
                        npx = n[py, px]
                        dist = float(npx[0] * dx[0] + npx[1] * dx[1] + npx[2] * dx[2]) * inv_fx
                        wt *= math.exp(-(dist * dist))
                    v = rgb[qy, qx] * rgb[qy, qx]
                    if demodulate:
                        v = v / np.maximum(albedo[qy, qx], 1e-3)
                    acc = acc + wt * v
                    wsum += wt
            if wsum > 0.0:
                L = acc / wsum
                if demodulate:
                    L = L * albedo[py, px]
                out[py, px] = np.sqrt(np.maximum(L, 0.0))
            else:
                out[py, px] = rgb[j0 * step_y, i0 * step_x]
    return out
