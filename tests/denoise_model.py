"""numpy restatement of the denoiser of csrc/rt_denoise.hip: the definition the device kernels are held to.

guides: dict of numpy planes as Scene.render_guides returns them — normal, position, albedo [H, W, 3] f64, footprint [H, W]
f64, obj_id [H, W] int32.  The arithmetic follows the kernel's order (taps dy, then dx; weights h(dx) h(dy) w_n w_x w_c), so
the two agree to rounding.  oracle_guides() forms the same planes with the CPU oracle.
"""
import ctypes as C
import math

import numpy as np

H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
DEMODULATE = 1


def atrous(I, guides, i, sigma_color=0.0, sigma_normal=0.0, sigma_plane=0.0):
    """One a-trous level (step 2^i) over demodulated linear radiance I [H, W, 3]."""
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
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    acc = np.zeros_like(I)
    wsum = np.zeros((h, w))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            qy, qx = ys + dy * step, xs + dx * step
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            use = inside & (ids[qy, qx] == ids)
            wt = np.full((h, w), H5[dx + 2] * H5[dy + 2])
            with np.errstate(invalid="ignore", over="ignore"):
                if inv_sn2 > 0:
                    wt = wt * np.exp(-np.sum((n - n[qy, qx]) ** 2, axis=-1) * inv_sn2)
                if inv_sx > 0:
                    dist = np.sum(n * (x[qy, qx] - x), axis=-1) * inv_fx
                    wt = wt * np.exp(-(dist * dist))
                if inv_sc2 > 0:
                    wt = wt * np.exp(-np.sum((sp - sp[qy, qx]) ** 2, axis=-1) * inv_sc2)
            wt = np.where(use, wt, 0.0)
            acc = acc + wt[..., None] * I[qy, qx]
            wsum = wsum + wt
    with np.errstate(divide="ignore", invalid="ignore"):
        out = acc * (1.0 / wsum)[..., None]
    miss = ids < 0
    out[miss] = I[miss]
    return out


def denoise(rgb, guides, iterations=5, flags=DEMODULATE, sigma_color=0.0, sigma_normal=0.1, sigma_plane=1.0):
    """The gamma-encoded frame rgb [H, W, 3] filtered -> [H, W, 3] (iterations 0: an exact copy)."""
    rgb = np.asarray(rgb, dtype=np.float64)
    if iterations == 0:
        return rgb.copy()
    albedo = guides["albedo"]
    L = rgb * rgb
    I = L / np.maximum(albedo, 1e-3) if flags & DEMODULATE else L
    for i in range(iterations):
        I = atrous(I, guides, i, sigma_color, sigma_normal, sigma_plane)
    L = I * albedo if flags & DEMODULATE else I
    return np.sqrt(np.maximum(L, 0.0))


def params_kwargs(dp):
    """An abi.RtDenoiseParams as denoise()'s keyword arguments."""
    return dict(iterations=dp.iterations, flags=dp.flags, sigma_color=dp.sigma_color, sigma_normal=dp.sigma_normal,
                sigma_plane=dp.sigma_plane)


def oracle_guides(orc, bundle, cam, width, height):
    """The guide planes of include/rt_abi.h with the CPU oracle: pinhole rays through the pixel centres at the middle of
    the shutter interval, orc_scene_hit_time over [0.001, inf), orc_texture_value for the albedo.  Scenes with wrapped
    primitives use the oracle's linear scan (its BVH keeps RotateY's mis-sized box, tests/variant_scenes.py)."""
    abi = orc.abi
    desc = bundle.desc
    lib = orc.lib()
    use_bvh = 0 if any(bundle.primitives[i].flags for i in range(desc.n_primitives)) else 1
    scene = lib.orc_scene_build(C.byref(desc), use_bvh, 1)
    g = {"normal": np.zeros((height, width, 3)), "position": np.zeros((height, width, 3)),
         "albedo": np.ones((height, width, 3)), "footprint": np.full((height, width), np.inf),
         "obj_id": np.full((height, width), -1, dtype=np.int32)}
    o = np.array(cam.origin[:])
    ulc, hor, ver = np.array(cam.upper_left_corner[:]), np.array(cam.horizontal[:]), np.array(cam.vertical[:])
    time = (cam.time_a + cam.time_b) * 0.5
    vlen = math.sqrt(float(np.dot(ver, ver)))
    hit = orc.OrcHit()
    tex = (C.c_double * 3)()
    try:
        for py in range(height):
            v = (py + 0.5) / (height - 1)
            for px in range(width):
                u = (px + 0.5) / (width - 1)
                d = ulc + u * hor - v * ver - o
                if not lib.orc_scene_hit_time(scene, orc.d3(o), orc.d3(d), time, 0.001, math.inf, C.byref(hit)):
                    continue
                g["normal"][py, px] = hit.normal[:]
                g["position"][py, px] = hit.point[:]
                g["footprint"][py, px] = hit.t * vlen / (height - 1)
                g["obj_id"][py, px] = hit.obj_id
                m = desc.materials[hit.material]
                if m.kind in (abi.RT_MAT_LAMBERTIAN, abi.RT_MAT_METAL):
                    lib.orc_texture_value(C.byref(desc), m.texture, hit.u, hit.v, orc.d3(hit.point), tex)
                    g["albedo"][py, px] = np.clip(np.array(tex[:]), 0.0, 1.0)
    finally:
        lib.orc_scene_free(scene)
    return g


def gamma_rmse(a, b):
    """RMSE of two gamma-encoded frames (the tone map aside)."""
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))
