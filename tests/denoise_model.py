"""numpy restatement of the denoiser of csrc/rt_denoise.hip: the definition the device kernels are held to.

guides: dict of numpy planes as Scene.render_guides returns them — normal, position, albedo [H, W, 3] f64, footprint [H, W]
f64, obj_id [H, W] int32.  The arithmetic follows the kernel's order (taps dy, then dx; weights h(dx) h(dy) w_n w_x w_c), so
the two agree to rounding.  oracle_guides() forms the same planes with the CPU oracle.  The model itself is held to
tests/denoise_reference.py, a 40-digit restatement of DESIGN.md 4.6 that shares nothing with it.
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


def synthetic_guides(h=24, w=32, seed=3):
    """Caller-made guide planes [h, w] that reach the filter's corners, and the generator that made them.

    Two objects split by a diagonal with noisy normals and positions on two planes; a miss band on the left (w >= 10)
    and misses on a lattice inside the frame; single-pixel islands (id 7) on another lattice, none 4-adjacent to another;
    a footprint that jumps by up to 20x from one pixel to the next; albedo channels at 0 and in (0, 1e-3), below the
    demodulation clamp.  Misses carry the values rt_abi.h gives them: id -1, normal and position 0, albedo 1,
    footprint inf."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ids = np.where(xs + ys < (h + w) // 2, 1, 2).astype(np.int32)
    ids[(ys % 4 == 1) & (xs % 5 == 1)] = 7
    ids[:, :w // 10] = -1
    ids[(ys % 3 == 0) & (xs % 4 == 1)] = -1
    n = np.zeros((h, w, 3))
    n[..., 2] = 1.0
    n[ids == 2] = (0.0, 0.6, 0.8)
    n[ids == 7] = (0.6, 0.0, 0.8)
    n = n + rng.normal(0.0, 0.05, n.shape)
    x = np.stack([xs * 0.1, ys * 0.1, rng.normal(0.0, 0.01, (h, w))], axis=-1)
    x[ids == 2, 2] += 0.2 * ys[ids == 2]
    albedo = rng.uniform(0.05, 1.0, (h, w, 3))
    pick = rng.random((h, w, 3))
    albedo[pick < 0.06] = 0.0
    low = (pick >= 0.06) & (pick < 0.12)
    albedo[low] = rng.uniform(1e-6, 9e-4, low.sum())
    g = {"normal": n, "position": x, "albedo": albedo, "footprint": 0.05 * np.exp(rng.uniform(-1.5, 1.5, (h, w))),
         "obj_id": ids}
    miss = ids < 0
    g["normal"][miss] = 0.0
    g["position"][miss] = 0.0
    g["albedo"][miss] = 1.0
    g["footprint"][miss] = np.inf
    return g, rng


def synthetic_frame(g, rng):
    """A gamma-encoded frame for synthetic_guides: g in [0.2, 1.5) with about 8 % of the pixels scaled by 10..630 (up to
    g ~ 1e3), about 5 % black and about 5 % of the channels 0."""
    h, w = g["obj_id"].shape
    rgb = rng.uniform(0.2, 1.5, (h, w, 3))
    pick = rng.random((h, w))
    rgb[pick < 0.08] *= 10.0 ** rng.uniform(1.0, 2.8, ((pick < 0.08).sum(), 1))
    rgb[(pick >= 0.08) & (pick < 0.13)] = 0.0
    rgb[rng.random((h, w, 3)) < 0.05] = 0.0
    return rgb


# Where a true output's square (the linear radiance) lies below the f64 normal range (|g| < 2^-511), no f64 pipeline can
# produce it: an edge stop of exp(-x), x > 745, underflows to 0.  A high-precision reference still carries e^-800 of a
# neighbour into a black pixel, so there, and only there, any value below the bound is accepted.
TINY = 2.0 ** -511


def mismatch(got, want, rel):
    """Number of channels where |got - want| > rel |want| (zeros exact, values below TINY aside)."""
    got, want = np.asarray(got), np.asarray(want)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - want) <= rel * np.abs(want)
    ok |= (np.abs(want) < TINY) & (np.abs(got) < TINY)
    return int((~ok).sum())


def gamma_rmse(a, b):
    """RMSE of two gamma-encoded frames (the tone map aside)."""
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))
