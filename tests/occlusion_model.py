"""The occlusion query's expected answers (include/rt_occlusion.h), on top of tests/ray_query_model.py: a
ray is occluded iff the closest query's model, Q.expected over the ray's own window, names a primitive; an invalid ray is
INVALID here as there.

A helper, not a test file.  Two ray sets per scene of Q.SCENES:

  A  THE random set of Q.random_rays with the default window [0.001, inf);
  B  the same rays with t_max = f * t_model where the model hits and t_max = 1 elsewhere, f drawn by default_rng(2027)
     uniformly in [0.5, 1.5]: about half of the hit rays lose their hit to the window's far end.

tests/test_occlusion_cpu.py checks the sets' conditions, tests/test_gpu_occlusion.py compares the device with them.
"""
import numpy as np

import ray_query_model as Q

INVALID = Q.INVALID
SEED_B = 2027
N_A, N_B = 16384, 4096      # what the tests use


def expected(orc, bundle, origin, direction, t_min=None, t_max=None, time=None):
    """-> int32 [n]: 1 occluded, 0 not, INVALID, for these rays on the (numbered) scene."""
    prim = Q.expected(orc, bundle, origin, direction, t_min=t_min, t_max=t_max, time=time)["prim"]
    return np.where(prim == INVALID, INVALID, (prim >= 0).astype(np.int32)).astype(np.int32)


def set_a(orc, name, n=N_A):
    """-> dict: bundle, closest_hit, in_lds, origin, direction, time, t_max (None), closest (Q.expected's planes over the
    default window), want (int32 [n])."""
    bundle, cam, spread, closest_hit, in_lds = Q.scene(name)
    o, d, time = Q.random_rays(cam, n, spread)
    closest = Q.expected(orc, bundle, o, d, time=time)
    want = (closest["prim"] >= 0).astype(np.int32)      # (the set has no invalid ray)
    return freeze(dict(bundle=bundle, closest_hit=closest_hit, in_lds=in_lds, origin=o, direction=d, time=time, t_max=None,
                       closest=closest, want=want))


def factors(n):
    """Set B's f, one per ray."""
    return np.random.default_rng(SEED_B).uniform(0.5, 1.5, n)


def set_b(orc, name, n=N_B, a=None):
    """-> set_a's dict with t_max [n], f [n] and want over [0.001, t_max]; `a`: set_a(orc, name, n) if the caller has it."""
    a = a if a is not None else set_a(orc, name, n)
    f = factors(n)
    t_model = a["closest"]["t"]
    t_max = np.where(a["closest"]["prim"] >= 0, f * np.where(np.isfinite(t_model), t_model, 1.0), 1.0)
    want = expected(orc, a["bundle"], a["origin"], a["direction"], t_max=t_max, time=a["time"])
    return freeze(dict(a, t_max=t_max, f=f, want=want))


def freeze(s):
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            freeze(v)
    return s
