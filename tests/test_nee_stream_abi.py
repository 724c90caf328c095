"""rt_render_nee without a device: exported with the documented signature and bound, the ABI version unchanged, and every
refusal the header lists returned before a device is touched (a NULL scene), each with a message naming its cause."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_exported_and_bound(rt):
    lib = C.CDLL(rt.LIB_PATH)
    assert "rt_render_nee" in rt.abi.PROTOTYPES and hasattr(lib, "rt_render_nee")
    assert rt.lib().rt_abi_version() == rt.abi.ABI_VERSION == 5
    assert hasattr(rt.Scene, "render_tiles_nee")
    assert rt.nee_stream_chunk() >= 1 and rt.nee_stream_chunk(rt.abi.RT_ARITH_REFERENCE) >= 1


def test_the_signature_is_the_documented_one(rt, abi):
    header = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    m = re.search(r"int rt_render_nee\(([^;]*)\);", header)
    assert m, "include/rt_abi.h does not declare rt_render_nee"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["RtScene *scene", "const RtCamera *camera", "const RtRenderParams *params",
                    "const RtLightSamplingParams *light_sampling", "RtTileCallback callback", "void *user",
                    "RtCancelCallback cancelled", "void *cancel_user"]
    res, argtypes = abi.PROTOTYPES["rt_render_nee"]
    assert res is C.c_int
    assert argtypes == [C.c_void_p, C.POINTER(abi.RtCamera), C.POINTER(abi.RtRenderParams), C.POINTER(abi.RtLightSamplingParams),
                        abi.RtTileCallback, C.c_void_p, abi.RtCancelCallback, C.c_void_p]
    assert re.search(r"#define RT_ABI_VERSION 5\b", header)


def test_refusals_come_before_the_device(rt, abi):
    lib, cam = rt.lib(), abi.RtCamera()
    cb = abi.RtTileCallback(lambda *a: None)
    no_cb = C.cast(None, abi.RtTileCallback)
    no_cancel = C.cast(None, abi.RtCancelCallback)
    calls = []
    counting = abi.RtTileCallback(lambda *a: calls.append(a))

    def call(p=None, ls=None, callback=cb):
        p = p or abi.render_params(16, 16, 4)
        ls = ls if ls is not None else rt.light_sampling_params()
        return lib.rt_render_nee(None, C.byref(cam), C.byref(p), C.byref(ls), callback, None, no_cancel, None)

    bad = rt.light_sampling_params()
    bad._reserved[5] = 1
    cases = [(None, rt.light_sampling_params(heuristic=2), b"heuristic"), (None, rt.light_sampling_params(heuristic=-1), b"heuristic"),
             (None, rt.light_sampling_params(max_lights=-1), b"max_lights"), (None, rt.light_sampling_params(max_lights=65), b"max_lights"),
             (None, bad, b"_reserved"),
             (abi.render_params(16, 16, 4, strip_rows=8, strip_count=2), rt.light_sampling_params(), b"strip"),
             (abi.render_params(16, 16, 4, scale=2), rt.light_sampling_params(), b"scale"),
             (None, rt.light_sampling_params(), b"scene is NULL")]
    for p, ls, word in cases:
        assert call(p, ls, counting) == abi.RT_ERR_INVALID_ARGUMENT, word
        assert word in lib.rt_last_error_message(), (word, lib.rt_last_error_message())
    assert not calls
    # NULL camera / params / light_sampling, each on its own, and all at once
    p, ls = abi.render_params(16, 16, 4), rt.light_sampling_params()
    for args in ((None, C.byref(p), C.byref(ls)), (C.byref(cam), None, C.byref(ls)), (C.byref(cam), C.byref(p), None), (None, None, None)):
        assert lib.rt_render_nee(None, args[0], args[1], args[2], cb, None, no_cancel, None) == abi.RT_ERR_INVALID_ARGUMENT
        assert b"NULL" in lib.rt_last_error_message()
    assert call(callback=no_cb) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"callback" in lib.rt_last_error_message()
