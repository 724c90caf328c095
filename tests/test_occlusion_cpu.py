"""The occlusion query's ray sets, on the CPU with the oracle alone (tests/occlusion_model.py): set B meets, on every scene of
tests/test_gpu_occlusion.py and at that test's n, the conditions its comparisons rest on.  Set A's conditions — enough hits
and misses, every primitive kind hit, next to no ties — are tests/test_rays_cpu.py's own and are not repeated here."""
import numpy as np
import pytest

import occlusion_model as M
import ray_query_model as Q


@pytest.fixture(scope="module")
def set_b(orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = M.set_b(orc, name)
        return cache[name]
    return get


def test_the_factors_keep_clear_of_one():
    """Every |f - 1| >= 1e-6: a window's far end lies at least that far, relatively, from the model's hit, the margin at which
    tests/test_gpu_rays.py's window test already holds the 0.9999 cap."""
    f = M.factors(M.N_B)
    assert f.shape == (M.N_B,) and (f >= 0.5).all() and (f <= 1.5).all()
    print("smallest |f - 1| = %.3g" % np.abs(f - 1.0).min())
    assert (np.abs(f - 1.0) >= 1e-6).all()
    assert np.array_equal(f, M.factors(M.N_B))


@pytest.mark.parametrize("name", Q.SCENES)
def test_set_b_splits_the_hit_rays(set_b, name):
    """Of the rays whose default window hits, between 0.3 and 0.7 stay occluded under set B's far end; a ray that misses
    with the default window misses with every window."""
    b = set_b(name)
    hit = b["closest"]["prim"] >= 0
    assert b["want"].shape == (M.N_B,) and np.isin(b["want"], (0, 1)).all()
    share = b["want"][hit].mean()
    print("%s: %d of %d rays hit, %.3f of them occluded in set B" % (name, hit.sum(), M.N_B, share))
    assert 0.3 <= share <= 0.7
    assert (b["want"][~hit] == 0).all()
    assert (b["t_max"][~hit] == 1.0).all() and (b["t_max"][hit] == b["f"][hit] * b["closest"]["t"][hit]).all()
    # the far end beyond the model's hit keeps it; the far end in front of the NEAREST hit leaves nothing to hit
    assert (b["want"][hit] == (b["f"][hit] > 1.0)).all()
