"""tests/nee_model.py, the restatement of rt_render_frame_nee's estimator, on the CPU: with no light listed it is the
oracle's plain estimator, at max_depth 1 it is the plain frame even with lights, and its mean is the plain mean (the
oracle's) on cornell_box and on a scene that mixes every case of the contract."""
import numpy as np
import pytest

import nee_model as NM
import scenes_py as S


def _params(abi, w, h, spp, depth, seed):
    p = abi.render_params(w, h, spp, max_depth=depth)
    p.seed = seed
    return p


@pytest.mark.parametrize("scene", ["cornell_box", "three_balls"])
def test_no_light_listed_is_the_oracle(orc, abi, scene):
    bundle, cam, _ = getattr(S, scene)()
    c = S.camera_for(cam, 24, 16)
    p = _params(abi, 24, 16, 3, 20, 5)
    model = NM.Model(orc, bundle.desc)
    got, segs = model.render(c, p, max_lights=0)
    want, want_segs = orc.render(bundle.desc, c, p)
    assert np.abs(got - want).max() < 1e-12
    assert segs == want_segs


def test_max_depth_one_is_the_plain_frame(orc, abi):
    bundle, cam = NM.mixed_scene(abi)
    c = S.camera_for(cam, 16, 12)
    p = _params(abi, 16, 12, 4, 1, 3)
    got, _ = NM.Model(orc, bundle.desc).render(c, p)
    want, _ = orc.render(bundle.desc, c, p)
    assert np.abs(got - want).max() < 1e-12


def test_the_light_list(abi):
    bundle, _ = NM.mixed_scene(abi)
    assert NM.light_list(bundle.desc) == [2, 3, 8]   # the moving emitter (4) is never listed
    assert NM.light_list(bundle.desc, 2) == [2, 3]
    box, _, _ = S.cornell_box()
    assert NM.light_list(box.desc) == [5]


CASES = [("cornell_box", h, d) for h in (NM.POWER, NM.BALANCE) for d in (2, 3, 8)] + \
        [("mixed", h, d) for h in (NM.POWER, NM.BALANCE) for d in (2, 3, 8)]


@pytest.mark.parametrize("scene,heuristic,depth", CASES)
def test_the_mean_is_the_plain_mean(orc, abi, scene, heuristic, depth):
    """Block means of linear radiance over 12 independent seeds each: |z| <= 5 everywhere, mean z^2 <= 2."""
    if scene == "mixed":
        bundle, cam = NM.mixed_scene(abi)
    else:
        bundle, cam, _ = S.cornell_box()
        cam = dict(cam)
    w, h, spp, seeds = 8, 8, 4, 12
    c = S.camera_for(cam, w, h)
    model = NM.Model(orc, bundle.desc)
    nee = [model.render(c, _params(abi, w, h, spp, depth, 100 + k), heuristic=heuristic)[0] for k in range(seeds)]
    plain = [orc.render(bundle.desc, c, _params(abi, w, h, 4 * spp, depth, 900 + k))[0] for k in range(seeds)]
    z = NM.block_z(nee, plain, block=4)
    assert np.all(np.abs(z) <= 5.0), z
    assert float(np.mean(z * z)) <= 2.0, z
