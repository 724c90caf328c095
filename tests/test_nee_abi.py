"""rt_render_frame_nee and its companions without a device: exported and bound, the parameter block laid out as gcc lays
it out, the defaults, and every refusal the header lists returned before a device is touched."""
import ctypes as C
import os
import subprocess
import tempfile

NEW = ("rt_light_sampling_params_default", "rt_scene_lights", "rt_render_frame_nee", "rt_render_frame_nee_device")
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def test_the_entry_points_are_exported_and_bound(rt):
    lib = C.CDLL(rt.LIB_PATH)
    for name in NEW:
        assert name in rt.abi.PROTOTYPES and hasattr(lib, name), name


def test_the_parameter_block_matches_gcc(abi):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(void){printf("%zu %zu %zu %zu %d %d\\n",'
           ' sizeof(RtLightSamplingParams), offsetof(RtLightSamplingParams, heuristic), offsetof(RtLightSamplingParams, max_lights),'
           ' offsetof(RtLightSamplingParams, _reserved), RT_MIS_POWER, RT_MIS_BALANCE); return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "l.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", INC, "-o", os.path.join(d, "l"), os.path.join(d, "l.c")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "l")]).split()]
    cls = abi.RtLightSamplingParams
    assert got == [C.sizeof(cls), cls.heuristic.offset, cls.max_lights.offset, cls._reserved.offset,
                   abi.RT_MIS_POWER, abi.RT_MIS_BALANCE]


def test_the_defaults_are_power_and_64(rt):
    ls = rt.light_sampling_params()
    assert (ls.heuristic, ls.max_lights, list(ls._reserved)) == (rt.abi.RT_MIS_POWER, 64, [0] * 6)
    rt.lib().rt_light_sampling_params_default(None)  # ignored
    assert rt.light_sampling_params(max_lights=3, heuristic=rt.abi.RT_MIS_BALANCE).max_lights == 3


def test_every_refusal_comes_before_the_device(rt, abi):
    cam = abi.RtCamera()
    out = (C.c_double * (16 * 16 * 3))()

    def call(params=None, ls=None, device=False, **ls_fields):
        p = params or abi.render_params(16, 16, 4)
        l = ls if ls is not None else rt.light_sampling_params(**ls_fields)
        if device:
            return rt.lib().rt_render_frame_nee_device(None, C.byref(cam), C.byref(p), C.byref(l), None, None)
        return rt.lib().rt_render_frame_nee(None, C.byref(cam), C.byref(p), C.byref(l), out)

    for device in (False, True):
        cases = [(dict(heuristic=2), b"heuristic"), (dict(heuristic=-1), b"heuristic"), (dict(max_lights=-1), b"max_lights"),
                 (dict(max_lights=65), b"max_lights"),
                 (dict(params=abi.render_params(16, 16, 4, strip_rows=8, strip_count=2)), b"strip"),
                 (dict(params=abi.render_params(16, 16, 4, scale=2)), b"scale"), (dict(), b"scene is NULL")]
        bad = rt.light_sampling_params()
        bad._reserved[5] = 1
        cases.append((dict(ls=bad), b"_reserved"))
        for kw, msg in cases:
            assert call(device=device, **kw) == abi.RT_ERR_INVALID_ARGUMENT, (device, kw)
            assert msg in rt.lib().rt_last_error_message(), (device, kw, rt.lib().rt_last_error_message())
        assert rt.lib().rt_render_frame_nee(None, None, None, None, out) == abi.RT_ERR_INVALID_ARGUMENT
        assert b"NULL" in rt.lib().rt_last_error_message()
    n = C.c_int32(7)
    assert rt.lib().rt_scene_lights(None, None, 0, C.byref(n)) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"NULL" in rt.lib().rt_last_error_message()
