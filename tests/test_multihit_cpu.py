"""The multi-hit query's ray sets, on the CPU with the oracle alone (tests/multihit_model.py, tests/multihit_scenes.py): the
conditions the comparisons of tests/test_gpu_multihit.py rest on, at that test's own n.  And the binding: it is there,
bound per library, and refuses what it must before a scene is looked at."""
import importlib

import numpy as np
import pytest

import multihit_model as M
import multihit_scenes as MS
import ray_query_model as Q

KS = (1, 2, 3, 4, 5, 8)      # the k of the device tests
TIE_CAP = {"cornell_box_boxes": 0.05}      # the boxes stand on the floor; 0.001 elsewhere


@pytest.fixture(scope="module")
def sets(orc):
    cache = {}

    def get(name, which):
        if (name, which) not in cache:
            cache[name, which] = MS.ray_set(orc, name, which)
        return cache[name, which]
    return get


def test_the_binding_exists_and_names_the_headers_limits():
    mh = importlib.import_module("racer-tracer_amd.multihit")
    rays = importlib.import_module("racer-tracer_amd.rays")
    assert mh.RT_MULTIHIT_MAX == 8 and mh.RT_MULTIHIT_HOST_CHUNK * 8 == rays.RT_RAYS_HOST_CHUNK
    assert mh.RtRays is rays.RtRays and mh.RtRayHits is rays.RtRayHits
    assert mh.multihit_params().k == 4 and mh.multihit_params()._reserved == 0
    assert mh.multihit_params(7).k == 7


@pytest.mark.parametrize("name", MS.STACKS)
def test_the_stack_set_is_deep_and_has_short_lists(sets, name):
    """At least 0.5 of the rays pass more than 8 primitives (k = 8 truncates), at least 0.05 fewer than 4 (unfilled slots at
    k = 4), and the rays from inside the nest meet spheres whose near root lies behind them."""
    s = sets(name, "stack")
    c = M.counts(s["lists"])
    print("%s: hits per ray %s; smallest relative gap among the first nine %.3g" %
          (name, np.bincount(c).tolist(), M.smallest_gap(s["lists"], 9)))
    assert len(c) == MS.N and (c >= 0).all()
    assert (c > 8).mean() >= 0.5
    assert (c < 4).mean() >= 0.05
    assert (c == 0).any()
    inside = np.arange(MS.N) % 4 == 3
    o, d = s["origin"], s["direction"]
    far_roots = 0
    for i in np.nonzero(inside)[0]:
        for t, prim, *_ in s["lists"][i]:
            if prim < 6:      # a sphere of the nest around an origin inside it: only its far root is in front
                assert np.linalg.norm(o[i] - np.array(MS.CENTRE)) < prim + 1
                far_roots += 1
    assert far_roots >= 6 * inside.sum() * 0.9


@pytest.mark.parametrize("name", Q.SCENES)
def test_the_pair_set_truncates_small_k(sets, name):
    """At least 0.05 of the rays pass more than 2 primitives, so k = 2 truncates; on the tree forms and large_bvh at least
    one ray passes more than 4.  Every ray passes the two primitives it was aimed through."""
    s = sets(name, "pair")
    c = M.counts(s["lists"])
    print("%s: hits per ray %s" % (name, np.bincount(c).tolist()))
    assert len(c) == MS.n_for(name)
    assert (c > 2).mean() >= 0.05
    assert (c >= 2).mean() >= 0.95
    if s["in_lds"] is not None:
        assert (c > 4).sum() >= 1


@pytest.mark.parametrize("name", MS.ALL_SCENES)
def test_tied_rays_are_rare(sets, name):
    """The cap on tied rays (multihit_model.tied) for every set and k of the device tests: 0.05 on cornell_box_boxes, 0.001
    elsewhere.  A condition of the sets, not a measurement: a set that breaks it is to be changed, not the cap."""
    cap = TIE_CAP.get(name, 0.001)
    for which in MS.sets_of(name):
        s = sets(name, which)
        shares = {k: M.tied(s["lists"], k).mean() for k in KS}
        print("%s set %s: tied share per k %s" % (name, which, shares))
        assert max(shares.values()) <= cap, which


@pytest.mark.parametrize("name", MS.ALL_SCENES)
def test_slot_0_is_the_closest_querys_model(orc, sets, name):
    """On every ray without a tie at k = 1 the model's slot 0 is ray_query_model.expected's answer: plane by plane, bit for
    bit (both come from the oracle's per-primitive test)."""
    for which in MS.sets_of(name):
        s = sets(name, which)
        want = Q.expected(orc, s["bundle"], s["origin"], s["direction"], time=s["time"])
        got = M.expected(s["lists"], 1)
        free = ~M.tied(s["lists"], 1)
        assert free.mean() >= 0.95
        assert np.array_equal(got["count"][free], (want["prim"][free] >= 0).astype(np.int32))
        for plane in Q.PLANES:
            assert np.array_equal(got[plane][0][free], want[plane][free], equal_nan=plane == "uv"), (which, plane)


def test_the_model_marks_invalid_rays_and_truncates():
    lists = [None, [], [(1.0, 3, (0, 0, 1), (0, 0, 1), (0.5, 0.5), 4, 1), (2.0, 1, (0, 0, 2), (0, 0, -1), (0.1, 0.2), 2, 0)]]
    got = M.expected(lists, 1)
    assert got["count"].tolist() == [Q.INVALID, 0, 1]
    assert got["prim"][0].tolist() == [Q.INVALID, Q.MISS, 3] and got["t"][0].tolist() == [np.inf, np.inf, 1.0]
    got = M.expected(lists, 3)
    assert got["count"].tolist() == [Q.INVALID, 0, 2] and got["prim"][:, 2].tolist() == [3, 1, Q.MISS]
    assert got["prim"][:, 0].tolist() == [Q.INVALID] * 3 and np.isinf(got["t"][2]).all()
    assert M.tied(lists, 1).tolist() == [False, False, False]
    assert M.tied([[(1.0, 0), (1.0 + 5e-10, 1), (3.0, 2)]], 1).tolist() == [True]
    assert M.tied([[(1.0, 0), (2.0, 1), (2.0, 2)]], 1).tolist() == [False]      # the tie lies behind slot k
    assert M.tied([[(1.0, 0), (2.0, 1), (2.0, 2)]], 2).tolist() == [True]
