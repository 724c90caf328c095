"""include/rt_occlusion.h on a machine without a GPU: the header is plain C, the library exports what the header declares,
occlusion.PROTOTYPES names exactly that, every refusal comes before a device is touched and leaves its own message, and the
kernel and its launcher exist in both arithmetic flavours.  No compute call is made here."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

from test_abi_layout import INC, ROOT, declared_functions, declared_parameter_counts

HEADER = "rt_occlusion.h"
FUNCTIONS = ["rt_trace_occlusion", "rt_trace_occlusion_device"]


@pytest.fixture(scope="module")
def occ():
    return importlib.import_module("racer-tracer_amd.occlusion")


def test_header_is_pedantic_c99():
    text = open(os.path.join(INC, HEADER)).read()
    assert "torch" not in text and "hip/" not in text
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(INC, HEADER)])
    # the rule, in the header's own words
    flat = " ".join(text.replace("*", " ").split())
    assert "A ray is occluded iff RT_RAYS_CLOSEST (rt_rays.h) over the same window would report a hit." in flat
    assert "Both window ends are inclusive, the defaults are [0.001, inf), and t is in units of the direction." in flat


def test_library_exports_and_prototypes_match_the_header(rt, occ):
    assert declared_functions(HEADER) == FUNCTIONS
    lib = C.CDLL(rt.LIB_PATH)
    assert [n for n in FUNCTIONS if not hasattr(lib, n)] == []
    assert sorted(occ.PROTOTYPES) == FUNCTIONS
    declared = declared_parameter_counts(HEADER)
    assert sorted(declared) == FUNCTIONS
    assert {n: len(a) for n, (_r, a) in occ.PROTOTYPES.items()} == declared
    assert occ.bound() is rt.lib()
    # the ABI version is untouched by the new header, and the binding's constants are the ray query's
    rays = importlib.import_module("racer-tracer_amd.rays")
    assert rt.lib().rt_abi_version() == rt.abi.ABI_VERSION == 5
    assert not set(FUNCTIONS) & set(rt.abi.PROTOTYPES) and not set(FUNCTIONS) & set(rays.PROTOTYPES)
    assert occ.RtRays is rays.RtRays and occ.RT_RAY_INVALID == rays.RT_RAY_INVALID == -2
    assert occ.RT_RAYS_HOST_CHUNK == rays.RT_RAYS_HOST_CHUNK


def calls(lib):
    return (("rt_trace_occlusion_device", lambda a: lib.rt_trace_occlusion_device(*a, None)),
            ("rt_trace_occlusion", lambda a: lib.rt_trace_occlusion(*a)))


def test_refusals_come_before_a_device_is_touched(rt, abi, occ):
    """Every refusal of the header's list, on a machine that may have no device: RT_ERR_INVALID_ARGUMENT, never
    RT_ERR_NO_DEVICE, each with a message of its own.  (With a NULL scene there is no device to touch; a fake non-NULL
    handle is never dereferenced, because the scene is looked at last.)"""
    lib = occ.bound()
    cam, p, frame = abi.RtCamera(), abi.render_params(16, 16, 1), (C.c_double * (16 * 16 * 3))()
    buf = (C.c_double * 6)()
    out = (C.c_int32 * 2)(7, 7)
    ok_rays = occ.RtRays(C.addressof(buf), C.addressof(buf), None, None, None)
    no_origin = occ.RtRays(None, C.addressof(buf), None, None, None)
    no_direction = occ.RtRays(C.addressof(buf), None, None, None, None)
    fake = C.c_void_p(0x1000)
    cases = {
        "scene": (None, C.byref(ok_rays), 1, out),
        "rays": (fake, None, 1, out),
        "output": (fake, C.byref(ok_rays), 1, None),
        "n < 0": (fake, C.byref(ok_rays), -1, out),
        "n > INT32_MAX": (fake, C.byref(ok_rays), 2 ** 31, out),
        "origin": (fake, C.byref(no_origin), 1, out),
        "direction": (fake, C.byref(no_direction), 1, out),
        # a NULL scene is refused even where there is nothing to do
        "scene, n == 0": (None, C.byref(ok_rays), 0, out),
    }
    messages = {}
    for what, args in cases.items():
        for name, call in calls(lib):
            # (each call follows one that leaves a message of its own)
            assert rt.lib().rt_render_frame_multi(None, 0, C.byref(cam), C.byref(p), 0, frame) == abi.RT_ERR_INVALID_ARGUMENT
            before = rt.lib().rt_last_error_message()
            assert call(args) == abi.RT_ERR_INVALID_ARGUMENT, (name, what)
            message = rt.lib().rt_last_error_message()
            assert message not in (b"", before), (name, what)
            messages[what, name] = message
    # each cause has its own message, the same in both forms
    for name, _ in calls(lib):
        own = {what: messages[what, name] for what in ("scene", "rays", "output", "n < 0", "origin", "direction")}
        assert len(set(own.values())) == len(own), own
        assert messages["n > INT32_MAX", name] == messages["n < 0", name]
        assert messages["scene, n == 0", name] == messages["scene", name]
    assert list(out) == [7, 7]


def test_an_empty_batch_is_ok_and_touches_nothing(abi, occ):
    """n == 0: RT_OK before the scene is dereferenced or a device is touched, the planes of the batch not looked at."""
    lib = occ.bound()
    out = (C.c_int32 * 1)(7)
    empty = occ.RtRays(None, None, None, None, None)
    for name, call in calls(lib):
        assert call((C.c_void_p(0x1000), C.byref(empty), 0, out)) == abi.RT_OK, name
    assert out[0] == 7


def test_eps_outside_half_is_refused_before_the_scene_is_looked_at(occ):
    import numpy as np
    a = np.zeros((1, 3))
    for eps in (0.6, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            occ.visible_between(None, a, a + 1.0, eps=eps)


def test_kernel_and_launcher_exist_in_both_flavours():
    so = os.path.join(ROOT, "racer-tracer_amd", "lib", "libracer_tracer_amd.so")
    symbols = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    exported = {line.split()[-1] for line in symbols.splitlines() if re.search(r"\brtdev_launch_occlusion\w*$", line)}
    assert exported == {"rtdev_launch_occlusion", "rtdev_launch_occlusion_exact"}
    for flavour in ("rtdev_fast", "rtdev_exact"):      # ... and so are the kernels behind them, with and without a tree
        for bvh in (0, 1):
            assert re.search(r"%s\d*14k_occluded_f64ILb%dE" % (flavour, bvh), symbols), (flavour, bvh)
