"""tests/nee_model.py's frames of the variant scenes (tests/variant_scenes.py) with `light2`, at the arguments the GPU
comparison uses (tests/test_gpu_nee.py: test_every_variant_of_the_nee_kernel_matches_the_model).  The CPU tests
(tests/test_nee_cpu.py) check on the same frames that the comparison can see what it is there for.  One model render per
key serves every test of a session."""
import nee_model as NM
import scenes_py as S
import variant_scenes as V

W, H, SPP, SEED = 32, 20, 6, 7
# (heuristic, max_lights, max_depth) of the three renders of a GPU case; the last one: the cap, and seg + 1 < max_depth
# leaves only the first vertex a light sample
RENDERS = ((NM.POWER, NM.MAX_LIGHTS, V.DEPTH), (NM.BALANCE, NM.MAX_LIGHTS, V.DEPTH), (NM.POWER, 1, 2))
N_LIGHTS = {V.RECTS: 3, V.SPHERES: 2, V.ANY: 4}   # listed in a light2 scene

_FRAMES = {}   # (form, heuristic, max_lights, depth) -> (frame, segments)


def case(abi, form):
    """-> (bundle, camera) of the form's light2 scene."""
    bundle, cam = V.build(form, light2=True)
    return bundle, S.camera_for(cam, W, H)


def params(abi, depth):
    p = abi.render_params(W, H, SPP, max_depth=depth)
    p.seed = SEED
    return p


def model_frame(orc, abi, form, heuristic, max_lights, depth):
    key = (form, heuristic, max_lights, depth)
    if key not in _FRAMES:
        bundle, camera = case(abi, form)
        model = NM.Model(orc, bundle.desc)
        try:
            _FRAMES[key] = model.render(camera, params(abi, depth), max_lights=max_lights, heuristic=heuristic)
        finally:
            model.close()
        _FRAMES[key][0].setflags(write=False)
    return _FRAMES[key]
