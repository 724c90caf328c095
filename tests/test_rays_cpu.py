"""The ray query's model and ray sets, on the CPU with the oracle alone (tests/ray_query_model.py): the model agrees with the
exact rational model of tests/ray_probes.py on every probe's rays, and THE random ray set meets, on every scene of
tests/test_gpu_rays.py and at that test's n, the conditions its comparisons rest on — enough hits and misses, every
primitive kind hit, and next to no ray whose two nearest primitives tie."""
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

import ray_probes as P
import ray_query_model as Q

N = 16384      # tests/test_gpu_rays.py: every scene form
abi = Q.abi


@pytest.fixture(scope="module")
def sets(orc):
    """name -> (bundle, origin, direction, time, expected planes), computed once, never written to."""
    cache = {}

    def get(name):
        if name not in cache:
            bundle, cam, spread, _, _ = Q.scene(name)
            o, d, time = Q.random_rays(cam, N, spread)
            want = Q.expected(orc, bundle, o, d, time=time)
            for a in (o, d, time, *want.values()):
                a.setflags(write=False)
            cache[name] = (bundle, o, d, time, want)
        return cache[name]
    return get


def test_the_scene_list_is_the_one_meant():
    assert len(Q.SCENES) == 16 + 3 and len(set(Q.SCENES)) == len(Q.SCENES)


@pytest.mark.parametrize("name", Q.SCENES)
def test_random_set_hits_enough_and_every_kind(sets, name):
    bundle, o, d, time, want = sets(name)
    hit = want["prim"] >= 0
    share = hit.mean()
    print("%s: hit share %.3f" % (name, share))
    assert 0.3 <= share <= 0.95
    assert (want["prim"][~hit] == Q.MISS).all() and np.isinf(want["t"][~hit]).all()
    kinds = lambda idx: {(bundle.primitives[int(i)].kind, bundle.primitives[int(i)].flags) for i in idx}      # noqa: E731
    present = kinds(range(bundle.desc.n_primitives))
    assert kinds(np.unique(want["prim"][hit])) == present
    assert np.array_equal(want["obj_id"][hit], want["prim"][hit] + 1)


@pytest.mark.parametrize("name", [n for n in Q.SCENES if n != "large_bvh"])
def test_random_set_has_next_to_no_ties(orc, sets, name):
    """Scenes of at most 64 primitives: at most 1 ray in 10^4 whose winner has another primitive within 1e-9 max(1, t)."""
    bundle, o, d, time, want = sets(name)
    assert bundle.desc.n_primitives <= 64
    margins = Q.tie_margins(orc, bundle, o, d, time, want)
    close = margins < 1e-9 * np.maximum(1.0, np.where(np.isfinite(want["t"]), want["t"], 1.0))
    print("%s: %d rays with a tie margin below 1e-9, smallest margin %.3g" % (name, close.sum(), margins.min()))
    assert close.sum() <= N // 10 ** 4


@pytest.mark.parametrize("name", list(P.PROBES))
def test_model_agrees_with_the_rational_model_on_every_probe(orc, name):
    probe = P.PROBES[name]
    bundle = probe.bundle()
    o, d, time = Q.probe_rays(probe)
    prims = [bundle.primitives[i] for i in range(bundle.desc.n_primitives)]
    want = Q.expected(orc, bundle, o, d, time=time)
    seen = {}
    for i in range(len(o)):
        key = (tuple(o[i]), tuple(d[i]))
        if key not in seen:
            seen[key] = P.q_scene(prims, o[i], d[i], time[i])
        best, t = seen[key]
        if best is None:
            assert want["prim"][i] == Q.MISS
            continue
        # a tie the probe declares (two primitives at one t): the linear scan's rule, the later one, is the model's too
        assert want["prim"][i] == best, (name, i)
        assert math.isclose(want["t"][i], float(t), rel_tol=1e-12), (name, i)
        assert Fr(Q.T_MIN) <= t
