"""include/rt_rays.h on a machine without a GPU: the header is plain C, the ctypes mirrors match gcc's layouts, the library
exports what the header declares, rays.PROTOTYPES names exactly that, every refusal comes before a device is touched, and
the kernel's launcher exists in both arithmetic flavours.  No compute call is made here."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import pytest

from test_abi_layout import INC, ROOT, declared_functions, declared_parameter_counts

HEADER = "rt_rays.h"
FUNCTIONS = ["rt_ray_query_params_default", "rt_trace_rays", "rt_trace_rays_device"]


@pytest.fixture(scope="module")
def rays():
    return importlib.import_module("racer-tracer_amd.rays")


def test_header_is_pedantic_c99():
    text = open(os.path.join(INC, HEADER)).read()
    assert "torch" not in text and "hip/" not in text
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(INC, HEADER)])


def test_struct_layouts_match_the_c_compiler(rays):
    structs = ["RtRays", "RtRayHits", "RtRayQueryParams"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, 'int main(void){']
    for s in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for name, _ in getattr(rays, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, name, s, name))
    for name in ("RT_RAY_MISS", "RT_RAY_INVALID", "RT_RAYS_CLOSEST", "RT_RAYS_ANY", "RT_RAYS_HOST_CHUNK"):
        lines.append('printf("%s %%d\\n", (int)%s);' % (name, name))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-I", INC, "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    want = dict(l.split() for l in out if l)
    for s in structs:
        cls = getattr(rays, s)
        assert C.sizeof(cls) == int(want[s]), s
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == int(want["%s.%s" % (s, name)]), (s, name)
    for name in ("RT_RAY_MISS", "RT_RAY_INVALID", "RT_RAYS_CLOSEST", "RT_RAYS_ANY", "RT_RAYS_HOST_CHUNK"):
        assert getattr(rays, name) == int(want[name]), name
    assert tuple(rays.HIT_PLANES) == tuple(n for n, _ in rays.RtRayHits._fields_)
    assert tuple(rays.RAY_PLANES) == tuple(n for n, _ in rays.RtRays._fields_)


def test_library_exports_and_prototypes_match_the_header(rt, rays):
    assert declared_functions(HEADER) == FUNCTIONS
    lib = C.CDLL(rt.LIB_PATH)
    assert [n for n in FUNCTIONS if not hasattr(lib, n)] == []
    assert sorted(rays.PROTOTYPES) == FUNCTIONS
    declared = declared_parameter_counts(HEADER)
    assert sorted(declared) == FUNCTIONS
    assert {n: len(a) for n, (_r, a) in rays.PROTOTYPES.items()} == declared
    assert rays.bound() is rt.lib()
    # rt_abi.h is untouched by the new header
    assert rt.lib().rt_abi_version() == rt.abi.ABI_VERSION == 5
    assert not set(FUNCTIONS) & set(rt.abi.PROTOTYPES)


def test_default_query_is_closest(rays):
    q = rays.RtRayQueryParams(7, 7)
    rays.bound().rt_ray_query_params_default(C.byref(q))
    assert (q.mode, q._reserved) == (rays.RT_RAYS_CLOSEST, 0)
    rays.bound().rt_ray_query_params_default(None)


def test_refusals_come_before_a_device_is_touched(rt, abi, rays):
    """Every refusal of the header's list, on a machine that may have no device: RT_ERR_INVALID_ARGUMENT, never
    RT_ERR_NO_DEVICE.  (With a NULL scene there is no device to touch; a fake non-NULL handle is never dereferenced,
    because the scene is looked at last.)"""
    lib = rays.bound()
    cam, p, out = abi.RtCamera(), abi.render_params(16, 16, 1), (C.c_double * (16 * 16 * 3))()
    buf = (C.c_double * 6)()
    ok_rays = rays.RtRays(C.addressof(buf), C.addressof(buf), None, None, None)
    hits = rays.RtRayHits()
    q = rays.query_params()
    fake = C.c_void_p(0x1000)
    bad_mode, bad_reserved = rays.RtRayQueryParams(2, 0), rays.RtRayQueryParams(0, 1)
    no_origin = rays.RtRays(None, C.addressof(buf), None, None, None)
    no_direction = rays.RtRays(C.addressof(buf), None, None, None, None)
    cases = {
        "scene": (None, C.byref(ok_rays), 1, C.byref(q), C.byref(hits)),
        "rays": (fake, None, 1, C.byref(q), C.byref(hits)),
        "hits": (fake, C.byref(ok_rays), 1, C.byref(q), None),
        "query": (fake, C.byref(ok_rays), 1, None, C.byref(hits)),
        "origin": (fake, C.byref(no_origin), 1, C.byref(q), C.byref(hits)),
        "direction": (fake, C.byref(no_direction), 1, C.byref(q), C.byref(hits)),
        "n < 0": (fake, C.byref(ok_rays), -1, C.byref(q), C.byref(hits)),
        "n > INT32_MAX": (fake, C.byref(ok_rays), 2 ** 31, C.byref(q), C.byref(hits)),
        "mode": (fake, C.byref(ok_rays), 1, C.byref(bad_mode), C.byref(hits)),
        "mode -1": (fake, C.byref(ok_rays), 1, C.byref(rays.RtRayQueryParams(-1, 0)), C.byref(hits)),
        "_reserved": (fake, C.byref(ok_rays), 1, C.byref(bad_reserved), C.byref(hits)),
        # a NULL scene is refused even where there is nothing to do
        "scene, n == 0": (None, C.byref(ok_rays), 0, C.byref(q), C.byref(hits)),
    }
    for what, args in cases.items():
        for name, call in (("rt_trace_rays_device", lambda a: lib.rt_trace_rays_device(*a, None)),
                           ("rt_trace_rays", lambda a: lib.rt_trace_rays(*a))):
            # (each call follows one that leaves a message of its own)
            assert rt.lib().rt_render_frame_multi(None, 0, C.byref(cam), C.byref(p), 0, out) == abi.RT_ERR_INVALID_ARGUMENT
            before = rt.lib().rt_last_error_message()
            assert call(args) == abi.RT_ERR_INVALID_ARGUMENT, (name, what)
            assert rt.lib().rt_last_error_message() not in (b"", before), (name, what)


def test_launcher_is_exported_in_both_flavours():
    so = os.path.join(ROOT, "racer-tracer_amd", "lib", "libracer_tracer_amd.so")
    symbols = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    exported = {line.split()[-1] for line in symbols.splitlines() if re.search(r"\brtdev_launch_\w*rays\w*$", line)}
    assert exported == {"rtdev_launch_trace_rays", "rtdev_launch_trace_rays_exact"}
    for flavour in ("rtdev_fast", "rtdev_exact"):      # ... and so are the kernels behind them
        assert re.search(r"%s\d*16k_trace_rays_f64" % flavour, symbols), flavour
