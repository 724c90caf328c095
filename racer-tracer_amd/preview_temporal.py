"""ctypes binding of include/rt_preview_temporal.h: jittered preview frames (RtRenderParams.scale > 1) accumulated into a
full-resolution history.

Like preview.py's, the entry points are found by symbol lookup and their prototypes live here, not in abi.PROTOTYPES: the
table is attached to a library object on the first call that needs it, once per library.  Import with
``importlib.import_module("racer-tracer_amd.preview_temporal")``.
"""
import ctypes as C

import numpy as np

from . import _or_default, abi, check, denoise_params, lib, temporal_params

PROTOTYPES = {
    "rt_preview_phase": (C.c_int, [C.POINTER(abi.RtRenderParams), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rt_preview_phase_camera": (C.c_int, [C.POINTER(abi.RtCamera), C.POINTER(abi.RtRenderParams), C.c_int32, C.c_int32,
                                          C.POINTER(abi.RtCamera)]),
    "rt_preview_accumulate_device": (C.c_int, [C.c_void_p, C.POINTER(abi.RtRenderParams), C.POINTER(abi.RtTemporalParams),
                                               C.POINTER(abi.RtDenoiseParams), C.c_int32, C.c_int32, C.c_void_p,
                                               C.POINTER(abi.RtGuides), C.POINTER(abi.RtCamera), C.POINTER(abi.RtHistory),
                                               C.POINTER(abi.RtHistory), C.c_void_p]),
    "rt_render_preview_temporal": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(abi.RtCamera), C.POINTER(abi.RtRenderParams),
                                             C.POINTER(abi.RtTemporalParams), C.POINTER(abi.RtDenoiseParams), C.c_int64,
                                             C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

_bound = []  # the library objects that carry PROTOTYPES (kept alive here: identity is what is compared)


def bound(library=None):
    """`library` (None: the default one) with PROTOTYPES attached; raises AttributeError where it lacks an entry point."""
    library = library if library is not None else lib()
    if not any(b is library for b in _bound):
        abi.bind(library, PROTOTYPES)
        _bound.append(library)
    return library


def phase(params, frame_index):
    """rt_preview_phase -> (jx, jy): the pixel of its block that frame `frame_index` of these params traces.  No device
    needed."""
    library = bound()
    jx, jy = C.c_int32(0), C.c_int32(0)
    check(library.rt_preview_phase(C.byref(params), frame_index, C.byref(jx), C.byref(jy)), "rt_preview_phase", library)
    return jx.value, jy.value


def phase_camera(camera, params, jx, jy):
    """rt_preview_phase_camera -> abi.RtCamera: `camera` shifted so that the preview's anchors trace the pixels of phase
    (jx, jy).  No device needed."""
    library = bound()
    out = abi.RtCamera()
    check(library.rt_preview_phase_camera(C.byref(camera), C.byref(params), jx, jy, C.byref(out)), "rt_preview_phase_camera",
          library)
    return out


def accumulate_device(scene, params, jx, jy, rgb_ptr, guides, out_history, prev_camera=None, prev_history=None, tparams=None,
                      dparams=None, stream=None):
    """rt_preview_accumulate_device on device addresses: rgb_ptr (int) the frame rt_render_frame_device wrote for these
    params (scale > 1) and phase_camera(camera, params, jx, jy); guides an abi.RtGuides of the UNSHIFTED camera's
    full-resolution planes; out_history / prev_history abi.RtHistory; prev_camera and prev_history both None: a first
    frame.  dparams decides the demodulation and the fill's stops (None: the defaults).  Enqueued on `stream`, not
    synchronised."""
    library = bound(scene._lib)
    tp = _or_default(tparams, temporal_params)
    dp = _or_default(dparams, denoise_params)
    check(library.rt_preview_accumulate_device(
        scene._h, C.byref(params), C.byref(tp), C.byref(dp), jx, jy, C.c_void_p(rgb_ptr), C.byref(guides),
        C.byref(prev_camera) if prev_camera is not None else None,
        C.byref(prev_history) if prev_history is not None else None, C.byref(out_history), C.c_void_p(stream or 0)),
        "rt_preview_accumulate_device", library)


def render_preview_temporal(scene, temporal, camera, params, frame_index, tparams=None, dparams=None, with_length=False):
    """rt_render_preview_temporal: the preview frame of (camera, params) at the phase of `frame_index`, accumulated into
    `temporal` (a Temporal) and filtered -> float64 [H, W, 3], or (frame, history length float64 [H, W]) with with_length.
    The caller advances params.seed from frame to frame."""
    library = bound(scene._lib)
    tp = _or_default(tparams, temporal_params)
    dp = _or_default(dparams, denoise_params)
    out = np.zeros((params.height, params.width, 3), dtype=np.float64)
    length = np.zeros((params.height, params.width), dtype=np.float64) if with_length else None
    check(library.rt_render_preview_temporal(scene._h, temporal._h, C.byref(camera), C.byref(params), C.byref(tp), C.byref(dp),
                                             frame_index, out.ctypes.data_as(C.POINTER(C.c_double)),
                                             length.ctypes.data_as(C.POINTER(C.c_double)) if with_length else None),
          "rt_render_preview_temporal", library)
    return (out, length) if with_length else out
