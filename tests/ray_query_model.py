"""The ray query's expected planes (include/rt_rays.h), from the oracle's LINEAR scan: orc_scene_build(desc,
0, ...) and orc_scene_hit_time over each ray's own window and time.  (The oracle's tree reproduces RotateY's box slip: on
the ray sets below it differs from the linear scan on 2-3 of 4096 rays of the wrapped scenes.)

A helper, not a test file.  tests/test_rays_cpu.py holds it to ray_probes.q_scene and checks the ray sets' conditions;
tests/test_gpu_rays.py compares the device with it.

Every scene is numbered first: obj_id = i + 1 on primitive i, so that the oracle's record names the description index.
"""
import ctypes as C
import math

import numpy as np

import scenes_py as S
import variant_scenes as V

abi = S.abi
T_MIN = 0.001
MISS, INVALID = -1, -2
PLANES = ("t", "point", "normal", "uv", "prim", "obj_id", "front_face")
SEED = 2026


def number(bundle):
    """obj_id = i + 1 on every primitive; -> bundle."""
    for i in range(bundle.desc.n_primitives):
        bundle.primitives[i].obj_id = i + 1
    return bundle


# name -> (bundle, camera dict, spread of the random set's targets, closest_hit option, tree in LDS or None: no tree)
def scene(name):
    if name == "three_balls":
        bundle, cam, _ = S.three_balls()
        return number(bundle), cam, 3.0, abi.RT_HIT_AUTO, None
    if name == "cornell_box_boxes":
        bundle, cam, _ = S.cornell_box_boxes()
        return number(bundle), cam, 250.0, abi.RT_HIT_AUTO, None
    if name == "large_bvh":
        bundle, cam = V.large_bvh_scene()
        return number(bundle), cam, 30.0, abi.RT_HIT_BVH, 0
    form = tuple(int(x) for x in name.split("-")[1:])
    bundle, cam = V.build(form)
    return number(bundle), cam, 3.0, (abi.RT_HIT_BVH if form[3] else abi.RT_HIT_AUTO), (1 if form[3] else None)


SCENES = ["form-%d-%d-%d-%d" % f for f in V.SPECS] + ["large_bvh", "three_balls", "cornell_box_boxes"]


def random_rays(cam, n, spread):
    """THE random ray set: origins around look_from, unnormalised directions to targets around look_at, times in [0, 1),
    the default window."""
    rng = np.random.default_rng(SEED)
    origin = np.array(cam["look_from"]) + rng.uniform(-1, 1, (n, 3))
    target = np.array(cam["look_at"]) + rng.uniform(-1, 1, (n, 3)) * spread
    direction = target - origin
    time = rng.uniform(0, 1, n)
    return np.ascontiguousarray(origin), np.ascontiguousarray(direction), time


def valid_ray(o, d, t_min, t_max, time):
    fin = all(math.isfinite(x) for x in (*o, *d, time, t_min))
    return fin and t_min >= 0.0 and t_max >= t_min and any(x != 0.0 for x in d)      # (NaN >= x is False)


def empty(n):
    return {"t": np.full(n, np.inf), "point": np.zeros((n, 3)), "normal": np.zeros((n, 3)), "uv": np.zeros((n, 2)),
            "prim": np.full(n, MISS, dtype=np.int32), "obj_id": np.full(n, -1, dtype=np.int32),
            "front_face": np.zeros(n, dtype=np.int32)}


def expected(orc, bundle, origin, direction, t_min=None, t_max=None, time=None):
    """-> the planes of RT_RAYS_CLOSEST for these rays on the (numbered) scene."""
    lib = orc.lib()
    n = len(origin)
    out = empty(n)
    handle = lib.orc_scene_build(C.byref(bundle.desc), 0, 1)
    hit = orc.OrcHit()
    try:
        for i in range(n):
            lo = T_MIN if t_min is None else float(t_min[i])
            hi = math.inf if t_max is None else float(t_max[i])
            tm = 0.0 if time is None else float(time[i])
            if not valid_ray(origin[i], direction[i], lo, hi, tm):
                out["prim"][i] = INVALID
                continue
            if lib.orc_scene_hit_time(handle, orc.d3(origin[i]), orc.d3(direction[i]), tm, lo, hi, C.byref(hit)):
                out["t"][i], out["point"][i], out["normal"][i] = hit.t, hit.point[:], hit.normal[:]
                out["uv"][i] = (hit.u, hit.v)
                out["prim"][i], out["obj_id"][i], out["front_face"][i] = hit.obj_id - 1, hit.obj_id, hit.front_face
    finally:
        lib.orc_scene_free(handle)
    return out


def primitive_t(orc, prim, o, d, time, lo, hi):
    """orc_hit_primitive_time of one primitive over [lo, hi] -> t or None."""
    hit = orc.OrcHit()
    if orc.lib().orc_hit_primitive_time(C.byref(prim), orc.d3(o), orc.d3(d), float(time), float(lo), float(hi), C.byref(hit)):
        return hit.t
    return None


def tie_margins(orc, bundle, origin, direction, time, want):
    """For every hit ray of `want` (expected()'s planes, default window): the distance in t from the winner to the nearest
    other primitive's hit, or inf."""
    prims = [bundle.primitives[j] for j in range(bundle.desc.n_primitives)]
    out = np.full(len(origin), np.inf)
    for i in np.nonzero(want["prim"] >= 0)[0]:
        for j, p in enumerate(prims):
            if j == want["prim"][i]:
                continue
            t = primitive_t(orc, p, origin[i], direction[i], time[i], T_MIN, math.inf)
            if t is not None:
                out[i] = min(out[i], abs(t - want["t"][i]))
    return out


def probe_rays(probe):
    """The rays oracle_guides forms for a probe (tests/ray_probes.py): d itself, plus the fan, at the probe's time.
    -> origin [n, 3], direction [n, 3], time [n], in the guide frame's pixel order."""
    s = probe.spec()
    w, h, _ = probe.guide_shape()
    o = np.array([float(x) for x in s["o"]])
    cam = probe.camera()
    ulc, hor, ver = np.array(cam.upper_left_corner[:]), np.array(cam.horizontal[:]), np.array(cam.vertical[:])
    rows = []
    for py in range(h):
        for px in range(w):
            rows.append(ulc + (px + 0.5) / (w - 1) * hor - (py + 0.5) / (h - 1) * ver - o)
    direction = np.ascontiguousarray(np.array(rows))
    origin = np.ascontiguousarray(np.tile(o, (len(rows), 1)))
    return origin, direction, np.full(len(rows), float(s["time"]))
