"""tests/nee_model.py, the restatement of rt_render_frame_nee's estimator, on the CPU: with no light listed it is the
oracle's plain estimator, at max_depth 1 it is the plain frame even with lights, and its mean is the plain mean (the
oracle's) on cornell_box and on a scene that mixes every case of the contract; and all of that on the scene of every
kernel form (tests/variant_scenes.py) with several lights of every kind, where the GPU comparison of every form needs it."""
import numpy as np
import pytest

import nee_model as NM
import nee_variant_frames as F
import scenes_py as S
import variant_scenes as V


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


# ---- the variant scenes (tests/variant_scenes.py), which the GPU comparison of every k_nee_f64 form stands on ------------

FORMS = sorted(V.SPECS)
_form_id = lambda f: "%s%s%s%s" % ("RSA"[f[0]], "t" * f[1], "s" * f[2], "-bvh" * f[3])  # noqa: E731


@pytest.mark.parametrize("light2", [False, True], ids=["plain", "light2"])
@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_no_light_listed_is_the_oracle_on_every_form(orc, abi, form, light2):
    """Boxes, wrappers, the lens, the moving sphere, Perlin, images and the Noise light: the model's geometry, textures
    and camera are the oracle's on every scene the GPU comparison uses."""
    bundle, cam = V.build(form, light2=light2)
    c = S.camera_for(cam, 24, 14)
    p = _params(abi, 24, 14, 4, 20, 5)
    got, segs = NM.Model(orc, bundle.desc).render(c, p, max_lights=0)
    want, want_segs = orc.render(bundle.desc, c, p, use_bvh=0)
    assert np.abs(got - want).max() < 1e-12
    assert segs == want_segs


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_the_light_list_of_every_form(abi, form):
    plain, _ = V.build(form)
    assert len(NM.light_list(plain.desc)) == 1
    bundle, _ = V.build(form, light2=True)
    lights = NM.light_list(bundle.desc)
    assert len(lights) == F.N_LIGHTS[form[0]]
    assert lights[0] == NM.light_list(plain.desc)[0]   # the appended lights come after every primitive of the plain scene
    assert bundle.desc.n_primitives == plain.desc.n_primitives + len(lights) - 1
    kinds = sorted(bundle.desc.primitives[i].kind for i in lights)
    want = {V.RECTS: [NM.XY, NM.XZ, NM.YZ], V.SPHERES: [NM.SPHERE, NM.SPHERE], V.ANY: [NM.SPHERE, NM.XY, NM.XZ, NM.YZ]}
    assert kinds == want[form[0]]
    assert NM.light_list(bundle.desc, 1) == lights[:1]


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_the_gpu_comparison_sees_the_lights_of_every_form(orc, abi, form):
    """At the GPU comparison's own arguments: the light samples move at least 30 % of the frame's values by more than
    1e-3 (its bound on the largest difference), so a kernel that skipped them fails it; so do the second and later lights,
    and the two heuristics differ."""
    power, segs = F.model_frame(orc, abi, form, *F.RENDERS[0])
    balance, _ = F.model_frame(orc, abi, form, *F.RENDERS[1])
    capped, _ = F.model_frame(orc, abi, form, *F.RENDERS[2])
    off, off_segs = F.model_frame(orc, abi, form, NM.POWER, 0, V.DEPTH)
    full_depth2, _ = F.model_frame(orc, abi, form, NM.POWER, NM.MAX_LIGHTS, 2)
    assert segs == off_segs   # the same paths
    share = float((np.abs(power - off) > 1e-3).mean())
    assert share >= 0.30, share
    assert np.abs(capped - full_depth2).max() > 1e-3
    assert np.abs(power - balance).max() > 1e-3
    assert power.std() > 0.05 and capped.std() > 0.05


_PLAIN_MEANS = {}   # form -> the plain frames of the mean check, the same under both heuristics


@pytest.mark.parametrize("heuristic", [NM.POWER, NM.BALANCE], ids=["power", "balance"])
@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_the_mean_is_the_plain_mean_on_every_form(orc, abi, form, heuristic):
    """test_the_mean_is_the_plain_mean on the light2 scene of every form: several lights of every kind next to boxes,
    wrappers, the lens, Perlin and the Noise light.  16x16, 4 against 16 samples, 12 seeds each: 48 block means (at 8x8,
    12 of them, the mean of z^2 alone scatters up to the cap)."""
    bundle, cam = V.build(form, light2=True)
    w, h, spp, seeds, depth = 16, 16, 4, 12, 8
    c = S.camera_for(cam, w, h)
    model = NM.Model(orc, bundle.desc)
    nee = [model.render(c, _params(abi, w, h, spp, depth, 100 + k), heuristic=heuristic)[0] for k in range(seeds)]
    if form not in _PLAIN_MEANS:
        _PLAIN_MEANS[form] = [orc.render(bundle.desc, c, _params(abi, w, h, 4 * spp, depth, 900 + k), use_bvh=0)[0]
                              for k in range(seeds)]
    z = NM.block_z(nee, _PLAIN_MEANS[form], block=4)
    assert np.all(np.abs(z) <= 5.0), np.abs(z).max()
    assert float(np.mean(z * z)) <= 2.0, float(np.mean(z * z))
