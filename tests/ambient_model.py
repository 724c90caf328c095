"""The ambient-occlusion query's rays and counts (include/rt_ambient.h) restated in numpy: the draws come
from the oracle's orc_rng_triple under purpose RT_RNG_AMBIENT, the operations stand in the header's stated order with one
rounding each (numpy contracts nothing: RT_ARITH_REFERENCE's arithmetic), and the verdict on a ray is occlusion_model's.

A helper, not a test file.  tests/test_ambient_cpu.py checks the model's directions against the cosine law and the seeds'
distance from the acceptance edge; tests/test_gpu_ambient.py compares the device's exported rays with rays().
"""
import ctypes as C
import math

import numpy as np

import occlusion_model as O
import ray_query_model as Q

RT_RNG_AMBIENT = 9
INVALID = O.INVALID
BIAS, RADIUS = 1e-3, math.inf      # rt_ambient_params_default
RAY_BAND, RAY_E_MAX = 32, 1022      # rt_query_ray.h
abi = Q.abi

# what tests/test_gpu_ambient.py draws and compares between flavours or with this model: (seed, index_base, n, samples);
# tests/test_ambient_cpu.py holds both clear of the acceptance edge
IDENTITY = (2028, 0, 256, 256)
WALL = (2029, 0, 4096, 64)


def floor_and_box():
    """The closed forms' scenes: a lone floor rect at y = 0, and a closed box of side 2 around the origin whose six rects
    overlap at the edges (no ray leaves through a corner)."""
    tex, mat = [abi.solid((0.5, 0.5, 0.5))], [abi.material(abi.RT_MAT_LAMBERTIAN, 0)]
    floor = abi.SceneBundle([abi.rect(abi.RT_PRIM_XZ_RECT, -50, 50, -50, 50, 0, 0, 1)], mat, tex, abi.sky())
    walls = [abi.rect(kind, -2, 2, -2, 2, k, 0, i + 1)
             for i, (kind, k) in enumerate([(abi.RT_PRIM_XY_RECT, -1), (abi.RT_PRIM_XY_RECT, 1), (abi.RT_PRIM_XZ_RECT, -1),
                                            (abi.RT_PRIM_XZ_RECT, 1), (abi.RT_PRIM_YZ_RECT, -1), (abi.RT_PRIM_YZ_RECT, 1)])]
    return Q.number(floor), Q.number(abi.SceneBundle(walls, mat, tex, abi.sky()))


def draws(orc, seed, index_base, n, samples):
    """u of every sample: -> (u [n, samples, 3], edge: the smallest | |c|^2 - 1 | over EVERY candidate looked at, accepted or
    not, blocks [n, samples]: how many candidates sample s of point p took)."""
    lib = orc.lib()
    e = (C.c_double * 3)()
    u = np.zeros((n, samples, 3))
    blocks = np.zeros((n, samples), dtype=np.int32)
    edge = math.inf
    for p in range(n):
        g = (index_base + p) & 0xFFFFFFFF
        for s in range(samples):
            i = 0
            while True:
                lib.orc_rng_triple(seed, g, s, 0, RT_RNG_AMBIENT, i, e)
                cx, cy, cz = -1.0 + 2.0 * e[0], -1.0 + 2.0 * e[1], -1.0 + 2.0 * e[2]      # random_double_range(-1, 1): exact
                l2 = (cx * cx + cy * cy) + cz * cz
                edge = min(edge, abs(l2 - 1.0))
                i += 1
                if l2 < 1.0:
                    break
            u[p, s] = (cx, cy, cz)
            blocks[p, s] = i
    return u, edge, blocks


def unit(a):
    """The header's unit(a), RT_ARITH_REFERENCE: l2 = (x x + y y) + z z, l = sqrt(l2), (x / l, y / l, z / l)."""
    x, y, z = a[..., 0], a[..., 1], a[..., 2]
    l = np.sqrt((x * x + y * y) + z * z)
    return np.stack([x / l, y / l, z / l], axis=-1)


def scaled_normal(normal):
    """Step 1's n' = normal * 2^-E (rt_query_ray.h: ray_exponent): E = 0 for a largest |component| within 2^+-32."""
    big = np.abs(normal).max(axis=-1)
    with np.errstate(all="ignore"):
        e = np.frexp(np.where(np.isfinite(big), big, 1.0))[1] - 1      # floor(log2 big); 0 gives -1
    e = np.where(big == 0.0, -1023, e)
    e = np.where((e >= -RAY_BAND) & (e <= RAY_BAND), 0, np.clip(e, -RAY_E_MAX, RAY_E_MAX))
    return np.ldexp(normal, -e[..., None])


def valid_points(points, normals, t_min, t_max, time):
    """rt_query_ray.h's ray_valid with the normal in the direction's place -> bool [n]."""
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(points).all(axis=1) & np.isfinite(normals).all(axis=1) & np.isfinite(time) & np.isfinite(t_min)
        return fin & (t_min >= 0.0) & (t_max >= t_min) & (normals != 0.0).any(axis=1)


def rays(orc, points, normals, samples, seed=0, index_base=0, bias=BIAS, radius=RADIUS, t_min=None, t_max=None, time=None, u=None):
    """The n * samples rays of the header's steps 1-6, ray j = p * samples + s -> dict: origin, direction [n S, 3], t_min,
    t_max, time [n S], valid [n] (bool), length [n S] (|dir| of step 3, before step 5's unit), edge (draws').  An invalid
    point's rays have a direction of zeros.  u: draws(...)[0] where the caller has it."""
    points, normals = np.asarray(points, dtype=np.float64), np.asarray(normals, dtype=np.float64)
    n = len(points)
    t_min = np.full(n, bias) if t_min is None else np.asarray(t_min, dtype=np.float64)
    t_max = np.full(n, radius) if t_max is None else np.asarray(t_max, dtype=np.float64)
    time = np.zeros(n) if time is None else np.asarray(time, dtype=np.float64)
    valid = valid_points(points, normals, t_min, t_max, time)
    edge = None
    if u is None:
        u, edge, _ = draws(orc, seed, index_base, n, samples)
    with np.errstate(all="ignore"):
        nhat = unit(scaled_normal(np.where(valid[:, None], normals, 1.0)))      # (an invalid point's is never used)
        direction = nhat[:, None, :] + unit(u)                                       # step 3
        near_zero = (np.abs(direction) < 1e-8).all(axis=-1)                          # step 4
        direction = np.where(near_zero[..., None], nhat[:, None, :], direction)
        x, y, z = direction[..., 0], direction[..., 1], direction[..., 2]
        length = np.sqrt((x * x + y * y) + z * z)
        dhat = unit(direction)                                                       # step 5
    dhat = np.where(valid[:, None, None], dhat, 0.0)
    rep = lambda a: np.ascontiguousarray(np.repeat(a, samples, axis=0))      # noqa: E731
    return dict(origin=rep(points), direction=np.ascontiguousarray(dhat.reshape(n * samples, 3)), t_min=rep(t_min), t_max=rep(t_max),
                time=rep(time), valid=valid, length=length.reshape(n * samples), edge=edge)


def expected(orc, bundle, points, normals, samples, **kw):
    """-> int32 [n]: the open samples of every point on the (numbered) scene — occlusion_model's verdict 0 on the model's
    rays — or INVALID."""
    r = rays(orc, points, normals, samples, **kw)
    n = len(r["valid"])
    occluded = O.expected(orc, bundle, r["origin"], r["direction"], t_min=r["t_min"], t_max=r["t_max"], time=r["time"])
    open_ = (occluded.reshape(n, samples) == 0).sum(axis=1).astype(np.int32)
    return np.where(r["valid"], open_, INVALID).astype(np.int32)
