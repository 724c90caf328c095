"""Caller-made inputs for k_preview_accumulate, shared by tests/test_preview_temporal_cpu.py (which checks
the margin cap on them) and tests/test_gpu_preview_temporal.py (which runs them on the device): same generators, same seeds.

A textured plane under two pinhole cameras a fraction of a pixel apart.  Object ids and misses are functions of the world
position, so both cameras agree on them; the previous history is the previous camera's guides with normals, ids and
positions spoiled at random pixels and lengths drawn from lengths_of(shape).
"""
import numpy as np

import preview_temporal_model as PT
import scenes_py as S
import temporal_model as T

# (width, height, tiles_w, tiles_h, scale) -> the grid's steps, and the phases the device test runs
CASES = [((8, 6, 1, 1, 2), (2, 2), [(0, 0), (1, 0), (0, 1), (1, 1)]),
         ((13, 7, 1, 1, 4), (1, 1), [(0, 0)]),
         ((103, 47, 10, 5, 4), (2, 3), [(1, 2)]),        # an uncovered column (102 of 103) and uncovered rows (45 of 47)
         ((33, 17, 1, 1, 16), (11, 1), [(10, 0)])]
# The lengths of a case's previous history.  Zero is a fill, which is never read.  Where the grid has blocks (pixels can be
# carried), every other pixel has ONE length, a power of two: a carried length is sum(w L) / sum(w) over the valid taps, the
# kernel forms both sums without fused multiply-adds, every w L is then exact, and the quotient is L itself on the device
# and in numpy alike, whatever the last bits of the re-projected weights are — so the test can hold it bit for bit.  With
# steps of 1 nothing is carried and the lengths are mixed.  No 4 and no 3: a carried 4.0, or a blend's N = 3 + 1, would sit
# on the resolve's length >= 4 threshold.
MIXED_LENGTHS = [0.0, 0.0, 1.0, 2.0, 8.0, 32.0]
CARRIED_LENGTH = {(8, 6): 2.0, (103, 47): 8.0, (33, 17): 32.0}


def lengths_of(shape):
    """The values a case's previous lengths are drawn from (uniformly)."""
    one = CARRIED_LENGTH.get(tuple(shape[:2]))
    return MIXED_LENGTHS if one is None else [0.0, 0.0, one, one, one, one]


DEPTH = 5.0
SHIFT = (2.3, -1.4)   # the previous camera, in pixel pitches on the plane: the left columns and bottom rows re-project outside


def _camera(at, w, h):
    return S.camera_for(dict(look_from=(at[0], at[1], 0.0), look_at=(at[0], at[1], -1.0), vfov=40.0, aperture=0.0,
                             focus_distance=1.0), w, h)


def plane_guides(cam, w, h, pitch, rng, misses=True):
    """The guides of the plane z = -DEPTH: three objects and misses in world-space cells, a normal per object, albedo
    channels at 0 and below the demodulation clamp.  Misses carry rt_abi.h's values."""
    o, ulc, hor, ver = T.camera_vectors(cam)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u, v = (xs + 0.5) / (w - 1), (ys + 0.5) / (h - 1)
    d = ulc + u[..., None] * hor - v[..., None] * ver - o
    t = (-DEPTH - o[2]) / d[..., 2]
    x = o + t[..., None] * d
    cx, cy = np.floor(x[..., 0] / (2.7 * pitch)).astype(int), np.floor(x[..., 1] / (2.7 * pitch)).astype(int)
    ids = (1 + (cx + 2 * cy) % 3).astype(np.int32)
    mx, my = np.floor(x[..., 0] / (1.9 * pitch)).astype(int), np.floor(x[..., 1] / (1.9 * pitch)).astype(int)
    miss = ((mx + 3 * my) % 7 == 0) & misses
    normals = np.array([(0.0, 0.0, 1.0), (0.1, 0.0, 1.0), (0.0, 0.15, 1.0)])
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    n = normals[ids - 1]
    albedo = rng.uniform(0.05, 1.0, (h, w, 3))
    pick = rng.random((h, w, 3))
    albedo[pick < 0.05] = 0.0
    low = (pick >= 0.05) & (pick < 0.1)
    albedo[low] = rng.uniform(1e-6, 9e-4, low.sum())
    g = {"normal": n.copy(), "position": x, "albedo": albedo, "footprint": t * np.linalg.norm(ver) / (h - 1), "obj_id": ids}
    g["obj_id"][miss], g["normal"][miss], g["position"][miss] = -1, 0.0, 0.0
    g["albedo"][miss], g["footprint"][miss] = 1.0, np.inf
    return g


def make(shape, misses=True):
    """-> dict: params' shape, steps, cam_prev, cam, guides (the current camera's), full (a full-resolution gamma frame whose
    pixels the anchors of any phase carry), prev (the previous history)."""
    w, h, tw, th, scale = shape
    rng = np.random.default_rng(1000 * w + h)
    cam = _camera((0.0, 0.0), w, h)
    _, _, hor, _ = T.camera_vectors(cam)
    pitch = DEPTH * np.linalg.norm(hor) / (w - 1)   # (focus distance 1: the viewport sits at z = -1)
    cam_prev = _camera((SHIFT[0] * pitch, SHIFT[1] * pitch), w, h)
    g, g_prev = plane_guides(cam, w, h, pitch, rng, misses), plane_guides(cam_prev, w, h, pitch, rng, misses)
    full = rng.uniform(0.2, 1.5, (h, w, 3))
    full[rng.random((h, w)) < 0.05] = 0.0
    prev = T.first_history(rng.uniform(0.2, 1.5, (h, w, 3)), g_prev)
    lum = T.luminance(prev["radiance"])
    m1 = lum * rng.uniform(0.8, 1.2, (h, w))
    prev["moments"] = np.stack([m1, m1 * m1 * (1.0 + rng.uniform(0.0, 0.5, (h, w)))], axis=-1)
    prev["length"] = rng.choice(lengths_of(shape), (h, w))
    spoil = rng.random((h, w))
    prev["normal"][spoil < 0.08] = (1.0, 0.0, 0.0)                        # a normal mismatch
    prev["obj_id"][(spoil >= 0.08) & (spoil < 0.16)] = 9                   # an id mismatch
    prev["position"][(spoil >= 0.16) & (spoil < 0.22), 2] += 10.0 * pitch  # off the plane
    return dict(shape=shape, steps=PT.preview_grid(w, h, tw, th, scale)[:2], cam_prev=cam_prev, cam=cam, guides=g, full=full,
                prev=prev)


def frame_of(case, jx, jy):
    """The preview frame of phase (jx, jy): what a render with the phase camera writes for case['full']."""
    sx, sy = case["steps"]
    return PT.replicate_phase(case["full"], sx, sy, jx, jy)
