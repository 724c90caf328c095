"""The multi-hit query's expected planes (include/rt_multihit.h), from the oracle's per-primitive test:
for every ray, orc_hit_primitive_time (tests/ray_query_model.py: primitive_t's call) of EVERY primitive of the numbered
scene over the ray's own window and time, the hits sorted by (t, description index), the first k of them.  The record of a
slot is that call's own record.  No tree and no closest-hit loop of the oracle is involved.

A helper, not a test file.  tests/test_multihit_cpu.py checks the conditions of the ray sets (tests/multihit_scenes.py),
tests/test_gpu_multihit.py compares the device with the planes.  A call costs about 6 us: rays x primitives stays at or
below 10^6 per scene.
"""
import ctypes as C
import math

import numpy as np

import ray_query_model as Q

MISS, INVALID = Q.MISS, Q.INVALID
PLANES = Q.PLANES
TIE = 1e-9      # two hits closer than TIE max(1, t) are a tie: which primitive comes first is not compared


def hit_lists(orc, bundle, origin, direction, t_min=None, t_max=None, time=None):
    """-> one entry per ray: None for an invalid ray, else the list of (t, prim, point, normal, (u, v), obj_id, front_face)
    of every primitive with a hit inside the ray's window, sorted by (t, prim)."""
    lib = orc.lib()
    prims = [bundle.primitives[j] for j in range(bundle.desc.n_primitives)]
    hit = orc.OrcHit()
    out = []
    for i in range(len(origin)):
        lo = Q.T_MIN if t_min is None else float(t_min[i])
        hi = math.inf if t_max is None else float(t_max[i])
        tm = 0.0 if time is None else float(time[i])
        if not Q.valid_ray(origin[i], direction[i], lo, hi, tm):
            out.append(None)
            continue
        o, d = orc.d3(origin[i]), orc.d3(direction[i])
        found = []
        for j, p in enumerate(prims):
            if lib.orc_hit_primitive_time(C.byref(p), o, d, tm, lo, hi, C.byref(hit)):
                found.append((hit.t, j, tuple(hit.point[:]), tuple(hit.normal[:]), (hit.u, hit.v), hit.obj_id, hit.front_face))
        found.sort(key=lambda h: (h[0], h[1]))
        out.append(found)
    return out


def empty(k, n):
    return {"t": np.full((k, n), np.inf), "point": np.zeros((k, n, 3)), "normal": np.zeros((k, n, 3)), "uv": np.zeros((k, n, 2)),
            "prim": np.full((k, n), MISS, dtype=np.int32), "obj_id": np.full((k, n), -1, dtype=np.int32),
            "front_face": np.zeros((k, n), dtype=np.int32), "count": np.zeros(n, dtype=np.int32)}


def expected(lists, k):
    """hit_lists' answer -> the planes of rt_trace_rays_multi with this k, shape (k, n[, c]), plus count [n]."""
    n = len(lists)
    out = empty(k, n)
    for i, found in enumerate(lists):
        if found is None:
            out["count"][i] = INVALID
            out["prim"][:, i] = INVALID
            continue
        out["count"][i] = min(len(found), k)
        for j, (t, prim, point, normal, uv, obj_id, front) in enumerate(found[:k]):
            out["t"][j, i], out["point"][j, i], out["normal"][j, i], out["uv"][j, i] = t, point, normal, uv
            out["prim"][j, i], out["obj_id"][j, i], out["front_face"][j, i] = prim, obj_id, front
    return out


def counts(lists):
    """-> int [n]: how many primitives each ray hits in all (-1 for an invalid ray)."""
    return np.array([-1 if f is None else len(f) for f in lists])


def tied(lists, k):
    """-> bool [n]: a TIED ray is one where two of its first min(count, k) + 1 model hits lie within TIE max(1, t) of each
    other (the + 1: the first hit left out decides who fills slot k - 1)."""
    out = np.zeros(len(lists), dtype=bool)
    for i, found in enumerate(lists):
        if not found:
            continue
        t = [h[0] for h in found[:min(len(found), k) + 1]]
        out[i] = any(b - a <= TIE * max(1.0, abs(b)) for a, b in zip(t, t[1:]))
    return out


def smallest_gap(lists, first):
    """-> the smallest relative distance (b - a) / max(1, b) between neighbours among each ray's first `first` hits."""
    gap = math.inf
    for found in lists:
        t = [h[0] for h in (found or [])[:first]]
        for a, b in zip(t, t[1:]):
            gap = min(gap, (b - a) / max(1.0, abs(b)))
    return gap
