"""racer-tracer_amd — ctypes binding of libracer_tracer_amd.so (MI355X / gfx950).

The package name contains a hyphen like the reference crate's, so import it
with ``importlib.import_module("racer-tracer_amd")``.

This is plumbing over the C ABI of include/rt_abi.h (device path) and
include/rt_host.h (scene/config loading, tone map, PNG).  There is NO CPU
fallback: if the shared library is missing or no GPU is visible, calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# RACER_TRACER_AMD_LIB lets a developer point at another build of the same ABI
LIB_PATH = os.environ.get("RACER_TRACER_AMD_LIB", os.path.join(_HERE, "lib", "libracer_tracer_amd.so"))


class RtError(RuntimeError):
    def __init__(self, code, what, detail):
        super().__init__("%s failed: [%d] %s%s" % (what, code, _strerror(code), (": " + detail) if detail else ""))
        self.code = code


_lib = None


def _open(path):
    """The library at `path` with every prototype of abi.py attached, refused unless it is of the binding's ABI version."""
    library = abi.bind(abi.bind(C.CDLL(path), abi.PROTOTYPES), abi.DEV_PROTOTYPES)
    if library.rt_abi_version() != abi.ABI_VERSION:
        raise ImportError("ABI version mismatch in %s: library %d, binding %d"
                          % (path, library.rt_abi_version(), abi.ABI_VERSION))
    return library


def lib():
    """The loaded C-ABI library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `make -C %s` (or __graft_entry__.build()); "
                "there is no CPU fallback for the render path" % (LIB_PATH, _HERE))
        # torch's ROCm wheels carry their own libamdhip64; whichever HIP runtime a process loads first
        # serves everything after it, and torch cannot see the GPU through /opt/rocm's copy if this
        # library pulled that in first (the other order is fine).  So a process that has torch loads
        # torch's runtime first; one without torch (the C++/Rust hosts, the CLI) never notices.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = _open(LIB_PATH)
    return _lib


def load_library(path):
    """Another build of the same ABI (e.g. build/libracer_tracer_amd_exact.so, the tests' exact-arithmetic
    build) next to the default one: pass the result as Scene(..., library=...)."""
    lib()  # the default library (and torch's HIP runtime) first
    return _open(path)


def _strerror(code):
    try:
        return lib().rt_strerror(code).decode()
    except Exception:  # pragma: no cover - only when the library itself is missing
        return "?"


def check(code, what, library=None):
    if code != abi.RT_OK:
        raise RtError(code, what, (library or lib()).rt_last_error_message().decode())


def classify(desc):
    """rtdev_scene_classify: the kernel selection rule of rt_scene_create_ex on a description, without a device
    -> dict of abi.CLASSIFY_FIELDS."""
    d = desc.desc if hasattr(desc, "desc") else desc
    out = (C.c_int32 * len(abi.CLASSIFY_FIELDS))()
    check(lib().rtdev_scene_classify(C.byref(d), out), "rtdev_scene_classify")
    return dict(zip(abi.CLASSIFY_FIELDS, out))


def radiance_bound(desc):
    """rtdev_scene_radiance_bound: the bound on a finished sample's radiance that rt_scene_create_ex gives a description
    (what sizes the fixed-point sums), or 0.0: the scene has none and keeps f64 sums.  No device needed."""
    d = desc.desc if hasattr(desc, "desc") else desc
    out = C.c_double(0.0)
    check(lib().rtdev_scene_radiance_bound(C.byref(d), C.byref(out)), "rtdev_scene_radiance_bound")
    return out.value


def sum_exponent(bound, samples):
    """rtdev_sum_exponent: the exponent e of the fixed-point sums (sum_scale = 2^(52 - e)) of a render of `samples` samples
    per pixel under a radiance bound, or 0: f64 sums.  Raises RtError (RT_ERR_UNSUPPORTED) where such a render is refused.
    No device needed."""
    e = C.c_int32(0)
    check(lib().rtdev_sum_exponent(float(bound), int(samples), C.byref(e)), "rtdev_sum_exponent")
    return e.value


def progressive_passes(samples, pass_samples):
    """rtdev_progressive_passes: the samples_done of every callback of rt_render_progressive with params.samples = samples
    and this pass_samples, in order (chunk boundaries of the frame's chunk plan).  No device needed."""
    out = (C.c_int32 * 64)()
    n = C.c_int32(0)
    check(lib().rtdev_progressive_passes(int(samples), int(pass_samples), out, len(out), C.byref(n)), "rtdev_progressive_passes")
    if n.value > len(out):
        out = (C.c_int32 * n.value)()
        check(lib().rtdev_progressive_passes(int(samples), int(pass_samples), out, len(out), C.byref(n)), "rtdev_progressive_passes")
    return list(out[:n.value])


def nee_stream_chunk(arithmetic=abi.RT_ARITH_FAST):
    """rtdev_nee_stream_chunk: the samples rt_render_nee's kernel traces between two looks at the cancel word (a tuning
    constant of the build; no pixel depends on it).  No device needed."""
    return lib().rtdev_nee_stream_chunk_exact() if arithmetic == abi.RT_ARITH_REFERENCE else lib().rtdev_nee_stream_chunk()


def _params(struct, default, overrides):
    """A parameter block: `struct` as the default library's function named `default` fills it, then the overrides."""
    p = struct()
    getattr(lib(), default)(C.byref(p))
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def denoise_params(**overrides):
    """rt_denoise_params_default, with fields overridden by keyword (iterations, flags, sigma_color, sigma_normal,
    sigma_plane) -> abi.RtDenoiseParams.  No device needed."""
    return _params(abi.RtDenoiseParams, "rt_denoise_params_default", overrides)


def adaptive_params(**overrides):
    """rt_adaptive_params_default, with fields overridden by keyword (threshold, pass_samples, min_samples)
    -> abi.RtAdaptiveParams.  No device needed."""
    return _params(abi.RtAdaptiveParams, "rt_adaptive_params_default", overrides)


def light_sampling_params(**overrides):
    """rt_light_sampling_params_default, with fields overridden by keyword (heuristic, max_lights)
    -> abi.RtLightSamplingParams.  No device needed."""
    return _params(abi.RtLightSamplingParams, "rt_light_sampling_params_default", overrides)


def light_list_params(**overrides):
    """rt_light_list_params_default, with fields overridden by keyword (kinds, pick) -> abi.RtLightListParams.  No device
    needed."""
    return _params(abi.RtLightListParams, "rt_light_list_params_default", overrides)


def temporal_params(**overrides):
    """rt_temporal_params_default, with fields overridden by keyword (alpha, alpha_moments, max_history, normal_tolerance,
    plane_tolerance, sigma_luminance) -> abi.RtTemporalParams.  No device needed."""
    return _params(abi.RtTemporalParams, "rt_temporal_params_default", overrides)


def variance_filter_params(**overrides):
    """rt_variance_filter_params_default, with fields overridden by keyword (sigma_luminance, min_chunks)
    -> abi.RtVarianceFilterParams.  No device needed."""
    return _params(abi.RtVarianceFilterParams, "rt_variance_filter_params_default", overrides)


def _or_default(block, default):
    """A caller's parameter block, or (None) what `default`, one of the *_params functions above, returns."""
    return block if block is not None else default()


def _light_sampling(heuristic, max_lights):
    return light_sampling_params(**{k: v for k, v in (("heuristic", heuristic), ("max_lights", max_lights)) if v is not None})


def _adaptive(threshold, pass_samples, min_samples):
    return adaptive_params(**{k: v for k, v in (("threshold", threshold), ("pass_samples", pass_samples),
                                                ("min_samples", min_samples)) if v is not None})


def _adaptive_outputs(params):
    """The host arrays an adaptive render fills: (frame [H, W, 3] f64, samples [H, W] int32, tile_error f64, one value
    per 8x8 tile)."""
    h, w = params.height, params.width
    return (np.zeros((h, w, 3), dtype=np.float64), np.zeros((h, w), dtype=np.int32),
            np.zeros(((h + 7) // 8, (w + 7) // 8), dtype=np.float64))


# The three functions below return ctypes callback objects.  The C side keeps only the address, so the caller holds
# what it got in a local until the C call has returned.

def _cancel_hook(cancel):
    """The RtCancelCallback of `cancel` (a callable returning True once the render should stop), or NULL for None."""
    return abi.RtCancelCallback(lambda _user: 1 if cancel() else 0) if cancel is not None else C.cast(None, abi.RtCancelCallback)


def _frame_collector(h, w, on_frame):
    """(RtFrameCallback, frames): every pass appends (samples_done, a copy of its h x w frame) to `frames` and hands the
    same two to `on_frame` (None: nobody)."""
    frames = []

    def on_pass(_user, rgb, samples_done, _samples_total):
        arr = np.ctypeslib.as_array(rgb, shape=(h, w, 3)).copy()  # `rgb` is only valid during the callback
        frames.append((samples_done, arr))
        if on_frame is not None:
            on_frame(samples_done, arr)

    return abi.RtFrameCallback(on_pass), frames


def _nee_tile_assembler(params, on_tile):
    """(RtTileCallback, frame, order): every tile is copied into `frame` (float64 [H, W, 3], zero where none arrived),
    appended to `order` as (r, c, width, height) and handed as those four to `on_tile` (None: nobody)."""
    frame = np.zeros((params.height, params.width, 3), dtype=np.float64)
    order = []

    def on_update(_user, rgb, r, c, w, h):
        if w > 0 and h > 0:  # `rgb` is only valid during the callback
            frame[r:r + h, c:c + w] = np.ctypeslib.as_array(rgb, shape=(h, w, 3))
        order.append((r, c, w, h))
        if on_tile is not None:
            on_tile(r, c, w, h)

    return abi.RtTileCallback(on_update), frame, order


def _tile_collector(tiles):
    def on_tile(_user, rgb, r, c, w, h):
        # `rgb` is only valid during the callback; an empty tile (more tile rows / columns than pixels) carries no pixels
        arr = np.ctypeslib.as_array(rgb, shape=(h, w, 3)).copy() if w > 0 and h > 0 else np.zeros((h, w, 3))
        tiles.append((r, c, w, h, arr))
    return on_tile


def batch_planes_struct(planes):
    """abi.RtBatchPlanes over device tensors (a dict with sums, squares [H, W, 3] f64, samples, chunks [H, W] int32)."""
    return abi.RtBatchPlanes(*[planes[k].data_ptr() for k in ("sums", "squares", "samples", "chunks")])


HISTORY_PLANES = ("radiance", "moments", "length", "normal", "position", "obj_id")


def history_struct(planes):
    """abi.RtHistory over device tensors (a dict with radiance, moments, length, normal, position, obj_id)."""
    return abi.RtHistory(*[planes[k].data_ptr() for k in HISTORY_PLANES])


def guides_struct(planes):
    """abi.RtGuides over device tensors (a dict with normal, position, albedo, footprint, obj_id)."""
    return abi.RtGuides(*[planes[k].data_ptr() for k in ("normal", "position", "albedo", "footprint", "obj_id")])


def device_count():
    return lib().rt_device_count()


def _handles(scenes):
    """(library, RtScene handle array) of a multi-scene call.  The library is the one that made scenes[0]: a handle
    means nothing to another loaded copy, and that copy's last-error text is not this call's.  (No scenes: the default
    library refuses the call.)"""
    return scenes[0]._lib if scenes else lib(), (C.c_void_p * len(scenes))(*[s._h for s in scenes])


def render_frame_multi(scenes, camera, params, strip_rows=0):
    """rt_render_frame_multi: one frame over several Scene objects (one per device share)
    -> float64 [H, W, 3] on the host."""
    library, handles = _handles(scenes)
    out = np.zeros((params.height, params.width, 3), dtype=np.float64)
    check(library.rt_render_frame_multi(handles, len(scenes), C.byref(camera), C.byref(params), strip_rows,
                                        out.ctypes.data_as(C.POINTER(C.c_double))), "rt_render_frame_multi", library)
    return out


def render_frame_multi_device(scenes, camera, params, out_ptr, strip_rows=0):
    """rt_render_frame_multi_device: out_ptr = device address (int) on scenes[0]'s device."""
    library, handles = _handles(scenes)
    check(library.rt_render_frame_multi_device(handles, len(scenes), C.byref(camera), C.byref(params), strip_rows,
                                               C.c_void_p(out_ptr)), "rt_render_frame_multi_device", library)


def render_tiles_multi(scenes, camera, params, strip_rows=0, cancel=None):
    """rt_render_multi: the tile stream of one frame rendered by several Scene objects (one per device share)
    -> list of (r, c, width, height, float64 [height, width, 3]); cancel: None or a callable."""
    library, handles = _handles(scenes)
    tiles = []
    cb = abi.RtTileCallback(_tile_collector(tiles))
    hook = _cancel_hook(cancel)
    check(library.rt_render_multi(handles, len(scenes), C.byref(camera), C.byref(params), strip_rows, cb, None, hook, None),
          "rt_render_multi", library)
    return tiles


def render_frame_nee_multi(scenes, camera, params, strip_rows=0, heuristic=None, max_lights=None):
    """rt_render_frame_nee_multi: one next-event-estimation frame over several Scene objects (one per device share)
    -> float64 [H, W, 3] on the host, bit-identical to Scene.render_frame_nee's.  heuristic and max_lights as there."""
    library, handles = _handles(scenes)
    ls = _light_sampling(heuristic, max_lights)
    out = np.zeros((params.height, params.width, 3), dtype=np.float64)
    check(library.rt_render_frame_nee_multi(handles, len(scenes), C.byref(camera), C.byref(params), C.byref(ls), strip_rows,
                                            out.ctypes.data_as(C.POINTER(C.c_double))), "rt_render_frame_nee_multi", library)
    return out


def render_frame_nee_multi_device(scenes, camera, params, out_ptr, strip_rows=0, heuristic=None, max_lights=None):
    """rt_render_frame_nee_multi_device: out_ptr = device address (int) on scenes[0]'s device."""
    library, handles = _handles(scenes)
    ls = _light_sampling(heuristic, max_lights)
    check(library.rt_render_frame_nee_multi_device(handles, len(scenes), C.byref(camera), C.byref(params), C.byref(ls),
                                                   strip_rows, C.c_void_p(out_ptr)),
          "rt_render_frame_nee_multi_device", library)


def render_tiles_nee_multi(scenes, camera, params, strip_rows=0, heuristic=None, max_lights=None, cancel=None, on_tile=None):
    """rt_render_nee_multi: Scene.render_tiles_nee over several Scene objects (one per device share) -> (frame float64
    [H, W, 3] assembled from the tiles that arrived (zero elsewhere), list of (r, c, width, height) in arrival order)."""
    library, handles = _handles(scenes)
    ls = _light_sampling(heuristic, max_lights)
    cb, frame, order = _nee_tile_assembler(params, on_tile)
    hook = _cancel_hook(cancel)
    check(library.rt_render_nee_multi(handles, len(scenes), C.byref(camera), C.byref(params), C.byref(ls), strip_rows, cb,
                                      None, hook, None), "rt_render_nee_multi", library)
    return frame, order


class Scene:
    """RtScene handle: a scene uploaded to one GPU (rt_scene_create)."""

    def __init__(self, desc, device=0, closest_hit=abi.RT_HIT_AUTO, kernel=abi.RT_KERNEL_POOL, library=None,
                 arithmetic=abi.RT_ARITH_FAST, gather=abi.RT_GATHER_AUTO, launch_blocks=0):
        """closest_hit / kernel / arithmetic / gather / launch_blocks: RtSceneOptions (rt_scene_create_ex) — the
        defaults are rt_scene_create's own; arithmetic=RT_ARITH_REFERENCE selects the reference's IEEE divisions without
        FMA contraction; gather=RT_GATHER_STAGED makes rt_render_frame_multi_device stage and copy this scene's strips
        even on the output's device; launch_blocks > 0 caps the grid of the scene's persistent launches, so that the waves
        of a small frame take work item after work item (a test switch: same pixels).  library: load_library()."""
        self._lib = library or lib()
        self._h = C.c_void_p()
        self._desc_owner = desc  # keep SceneBundle / host session alive
        d = desc.desc if hasattr(desc, "desc") else desc
        opt = abi.RtSceneOptions(closest_hit, kernel, arithmetic, gather, launch_blocks)
        check(self._lib.rt_scene_create_ex(C.byref(d), device, C.byref(opt), C.byref(self._h)), "rt_scene_create_ex", self._lib)
        self.device = device

    def close(self):
        if self._h:
            self._lib.rt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render_frame(self, camera, params):
        """rt_render_frame -> float64 [H, W, 3], gamma-encoded, not tone-mapped."""
        out = np.zeros((params.height, params.width, 3), dtype=np.float64)
        check(self._lib.rt_render_frame(self._h, C.byref(camera), C.byref(params),
                                    out.ctypes.data_as(C.POINTER(C.c_double))), "rt_render_frame", self._lib)
        return out

    def render_frame_nee(self, camera, params, heuristic=None, max_lights=None):
        """rt_render_frame_nee -> float64 [H, W, 3], gamma-encoded, not tone-mapped.  heuristic (abi.RT_MIS_*) and
        max_lights: None keeps rt_light_sampling_params_default's value."""
        ls = _light_sampling(heuristic, max_lights)
        out = np.zeros((params.height, params.width, 3), dtype=np.float64)
        check(self._lib.rt_render_frame_nee(self._h, C.byref(camera), C.byref(params), C.byref(ls),
                                            out.ctypes.data_as(C.POINTER(C.c_double))), "rt_render_frame_nee", self._lib)
        return out

    def render_frame_nee_device(self, camera, params, out_ptr, stream=None, heuristic=None, max_lights=None):
        """rt_render_frame_nee_device: out_ptr = device address (int), stream = hipStream_t (int)."""
        ls = _light_sampling(heuristic, max_lights)
        check(self._lib.rt_render_frame_nee_device(self._h, C.byref(camera), C.byref(params), C.byref(ls), C.c_void_p(out_ptr),
                                                   C.c_void_p(stream or 0)), "rt_render_frame_nee_device", self._lib)

    def render_frame_nee_strips_device(self, camera, params, out_ptr, stream=None, heuristic=None, max_lights=None):
        """rt_render_frame_nee_strips_device: render_frame_nee_device honouring params.strip_*: only the rows this share
        owns are written.  out_ptr = device address (int) of a full frame, stream = hipStream_t (int)."""
        ls = _light_sampling(heuristic, max_lights)
        check(self._lib.rt_render_frame_nee_strips_device(self._h, C.byref(camera), C.byref(params), C.byref(ls),
                                                          C.c_void_p(out_ptr), C.c_void_p(stream or 0)),
              "rt_render_frame_nee_strips_device", self._lib)

    def lights(self):
        """rt_scene_lights -> the listed lights (indices into the description's primitives, table order, uncapped)."""
        n = C.c_int32(0)
        out = (C.c_int32 * 64)()
        check(self._lib.rt_scene_lights(self._h, out, len(out), C.byref(n)), "rt_scene_lights", self._lib)
        return list(out[:n.value])

    def set_lights(self, kinds=abi.RT_LIGHTS_PLAIN, pick=abi.RT_PICK_UNIFORM):
        """rt_scene_set_lights: list the scene's lights again (kinds: abi.RT_LIGHTS_*, or-ed; pick: abi.RT_PICK_*).  The
        defaults restore rt_scene_create's list."""
        lp = light_list_params(kinds=kinds, pick=pick)
        check(self._lib.rt_scene_set_lights(self._h, C.byref(lp)), "rt_scene_set_lights", self._lib)

    def light_weights(self):
        """rt_scene_light_weights -> the pick probabilities of the listed lights (uncapped list)."""
        n = C.c_int32(0)
        out = (C.c_double * 64)()
        check(self._lib.rt_scene_light_weights(self._h, out, len(out), C.byref(n)), "rt_scene_light_weights", self._lib)
        return list(out[:n.value])

    def render_frame_device(self, camera, params, out_ptr, stream=None):
        """rt_render_frame_device: out_ptr = device address (int), stream = hipStream_t (int)."""
        check(self._lib.rt_render_frame_device(self._h, C.byref(camera), C.byref(params),
                                           C.c_void_p(out_ptr), C.c_void_p(stream or 0)),
              "rt_render_frame_device", self._lib)

    def render_frame_rgba8(self, camera, params, tone_map):
        """rt_render_frame_rgba8 -> uint8 [H, W, 4]: render, tone-map and pack on the device."""
        out = np.zeros((params.height, params.width, 4), dtype=np.uint8)
        check(self._lib.rt_render_frame_rgba8(self._h, C.byref(camera), C.byref(params), C.byref(tone_map),
                                          out.ctypes.data_as(C.POINTER(C.c_uint8))), "rt_render_frame_rgba8", self._lib)
        return out

    def post_rgba8_device(self, tone_map, rgb_ptr, n_pixels, rgba_ptr, mapped_ptr=None, stream=None):
        """rt_post_rgba8_device on device addresses (ints)."""
        check(self._lib.rt_post_rgba8_device(self._h, C.byref(tone_map), C.c_void_p(rgb_ptr), n_pixels,
                                         C.c_void_p(rgba_ptr), C.c_void_p(mapped_ptr or 0), C.c_void_p(stream or 0)),
              "rt_post_rgba8_device", self._lib)

    def render_tiles(self, camera, params, cancel=None):
        """rt_render / rt_render_ex -> list of (r, c, width, height, float64 [height, width, 3]).
        cancel: None, a ctypes pointer to an int flag (rt_render), or a callable returning True once the
        render should stop (rt_render_ex's RtCancelCallback — how the reference's SignalEvent binds)."""
        tiles = []
        cb = abi.RtTileCallback(_tile_collector(tiles))
        if callable(cancel):
            hook = _cancel_hook(cancel)
            check(self._lib.rt_render_ex(self._h, C.byref(camera), C.byref(params), cb, None, hook, None), "rt_render_ex", self._lib)
        else:
            cancel_ptr = C.cast(cancel, C.POINTER(C.c_int)) if cancel is not None else None
            check(self._lib.rt_render(self._h, C.byref(camera), C.byref(params), cb, None, cancel_ptr), "rt_render", self._lib)
        return tiles

    def render_progressive(self, camera, params, pass_samples, cancel=None, on_frame=None, denoise=None):
        """rt_render_progressive -> list of (samples_done, float64 [H, W, 3] copy), one per pass, the last one equal to
        render_frame's.  cancel: None or a callable returning True once the render should stop (as render_tiles').
        on_frame: None or a callable(samples_done, frame) run inside each callback, with the copy that is kept.
        denoise: None, True (the defaults) or an abi.RtDenoiseParams: rt_render_progressive_denoised, every frame
        filtered, the last one equal to denoise(camera, params, render_frame(...))."""
        cb, frames = _frame_collector(params.height, params.width, on_frame)
        hook = _cancel_hook(cancel)
        if denoise is None or denoise is False:
            check(self._lib.rt_render_progressive(self._h, C.byref(camera), C.byref(params), int(pass_samples), cb, None, hook,
                                                  None), "rt_render_progressive", self._lib)
        else:
            dp = denoise_params() if denoise is True else denoise
            check(self._lib.rt_render_progressive_denoised(self._h, C.byref(camera), C.byref(params), int(pass_samples),
                                                           C.byref(dp), cb, None, hook, None),
                  "rt_render_progressive_denoised", self._lib)
        return frames

    def render_adaptive(self, camera, params, threshold=None, pass_samples=None, min_samples=None, cancel=None,
                        on_frame=None):
        """rt_render_adaptive -> (frame float64 [H, W, 3], samples int32 [H, W], tile_error float64 [ceil(H/8), ceil(W/8)],
        frames), frames being the list of (samples_done, float64 [H, W, 3] copy) of the callbacks.  threshold, pass_samples,
        min_samples: None keeps rt_adaptive_params_default's value.  cancel and on_frame as render_progressive's."""
        ap = _adaptive(threshold, pass_samples, min_samples)
        frame, samples, tile_error = _adaptive_outputs(params)
        cb, frames = _frame_collector(params.height, params.width, on_frame)
        hook = _cancel_hook(cancel)
        check(self._lib.rt_render_adaptive(self._h, C.byref(camera), C.byref(params), C.byref(ap),
                                           frame.ctypes.data_as(C.POINTER(C.c_double)),
                                           samples.ctypes.data_as(C.POINTER(C.c_int32)),
                                           tile_error.ctypes.data_as(C.POINTER(C.c_double)), cb, None, hook, None),
              "rt_render_adaptive", self._lib)
        return frame, samples, tile_error, frames

    def render_progressive_nee(self, camera, params, pass_samples, heuristic=None, max_lights=None, cancel=None, on_frame=None):
        """rt_render_progressive_nee -> list of (samples_done, float64 [H, W, 3] copy), one per pass, EACH equal to
        render_frame_nee's frame at samples = samples_done.  heuristic and max_lights as render_frame_nee's; cancel and
        on_frame as render_progressive's."""
        ls = _light_sampling(heuristic, max_lights)
        cb, frames = _frame_collector(params.height, params.width, on_frame)
        hook = _cancel_hook(cancel)
        check(self._lib.rt_render_progressive_nee(self._h, C.byref(camera), C.byref(params), C.byref(ls), int(pass_samples), cb,
                                                  None, hook, None), "rt_render_progressive_nee", self._lib)
        return frames

    def render_adaptive_nee(self, camera, params, threshold=None, pass_samples=None, min_samples=None, heuristic=None,
                            max_lights=None, cancel=None, on_frame=None):
        """rt_render_adaptive_nee -> (frame, samples, tile_error, frames) as render_adaptive's, every pixel being
        render_frame_nee's at its own sample count.  heuristic and max_lights as render_frame_nee's."""
        ls = _light_sampling(heuristic, max_lights)
        ap = _adaptive(threshold, pass_samples, min_samples)
        frame, samples, tile_error = _adaptive_outputs(params)
        cb, frames = _frame_collector(params.height, params.width, on_frame)
        hook = _cancel_hook(cancel)
        check(self._lib.rt_render_adaptive_nee(self._h, C.byref(camera), C.byref(params), C.byref(ls), C.byref(ap),
                                               frame.ctypes.data_as(C.POINTER(C.c_double)),
                                               samples.ctypes.data_as(C.POINTER(C.c_int32)),
                                               tile_error.ctypes.data_as(C.POINTER(C.c_double)), cb, None, hook, None),
              "rt_render_adaptive_nee", self._lib)
        return frame, samples, tile_error, frames

    def render_tiles_nee(self, camera, params, heuristic=None, max_lights=None, cancel=None, on_tile=None):
        """rt_render_nee -> (frame float64 [H, W, 3] assembled from the tiles that arrived (zero elsewhere), list of
        (r, c, width, height) in arrival order).  Every tile equals render_frame_nee's pixels.  heuristic and max_lights as
        render_frame_nee's; cancel: None or a callable returning True once the render should stop; on_tile: None or a
        callable(r, c, width, height) run inside each callback."""
        ls = _light_sampling(heuristic, max_lights)
        cb, frame, order = _nee_tile_assembler(params, on_tile)
        hook = _cancel_hook(cancel)
        check(self._lib.rt_render_nee(self._h, C.byref(camera), C.byref(params), C.byref(ls), cb, None, hook, None),
              "rt_render_nee", self._lib)
        return frame, order

    def render_guides(self, camera, params):
        """rt_render_guides_device on device buffers of torch, copied back -> dict of numpy planes: normal, position,
        albedo [H, W, 3] f64, footprint [H, W] f64, obj_id [H, W] int32."""
        import torch
        h, w = params.height, params.width
        dev = torch.device("cuda", self.device)
        planes = {"normal": torch.empty((h, w, 3), dtype=torch.float64, device=dev),
                  "position": torch.empty((h, w, 3), dtype=torch.float64, device=dev),
                  "albedo": torch.empty((h, w, 3), dtype=torch.float64, device=dev),
                  "footprint": torch.empty((h, w), dtype=torch.float64, device=dev),
                  "obj_id": torch.empty((h, w), dtype=torch.int32, device=dev)}
        g = guides_struct(planes)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            check(self._lib.rt_render_guides_device(self._h, C.byref(camera), C.byref(params), C.byref(g),
                                                    C.c_void_p(stream.cuda_stream)), "rt_render_guides_device", self._lib)
            stream.synchronize()
        return {k: v.cpu().numpy() for k, v in planes.items()}

    def denoise_device(self, params, rgb_ptr, guides, out_ptr, dparams=None, stream=None):
        """rt_denoise_device on device addresses (ints); guides: an abi.RtGuides of device addresses."""
        dp = _or_default(dparams, denoise_params)
        check(self._lib.rt_denoise_device(self._h, C.byref(params), C.byref(dp), C.c_void_p(rgb_ptr), C.byref(guides),
                                          C.c_void_p(out_ptr), C.c_void_p(stream or 0)), "rt_denoise_device", self._lib)

    def denoise(self, camera, params, rgb, dparams=None):
        """rt_denoise_frame: the guides of (camera, params) and the filter over a host frame -> float64 [H, W, 3]."""
        dp = _or_default(dparams, denoise_params)
        src = np.ascontiguousarray(rgb, dtype=np.float64)
        if src.shape != (params.height, params.width, 3):
            raise ValueError("rgb must be float64 [H, W, 3] of the params' size")
        out = np.zeros_like(src)
        check(self._lib.rt_denoise_frame(self._h, C.byref(camera), C.byref(params), C.byref(dp),
                                         src.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double))),
              "rt_denoise_frame", self._lib)
        return out

    def temporal_accumulate_device(self, params, rgb_ptr, guides, out_history, prev_camera=None, prev_history=None,
                                   tparams=None, dparams=None, stream=None):
        """rt_temporal_accumulate_device: rgb_ptr = device address (int) of a gamma-encoded frame; guides an abi.RtGuides,
        out_history / prev_history abi.RtHistory of device addresses; prev_camera and prev_history both None: a first frame.
        dparams decides the demodulation (None: the defaults).  Enqueued on `stream`, not synchronised."""
        tp = _or_default(tparams, temporal_params)
        dp = _or_default(dparams, denoise_params)
        check(self._lib.rt_temporal_accumulate_device(
            self._h, C.byref(params), C.byref(tp), C.byref(dp), C.c_void_p(rgb_ptr), C.byref(guides),
            C.byref(prev_camera) if prev_camera is not None else None,
            C.byref(prev_history) if prev_history is not None else None, C.byref(out_history), C.c_void_p(stream or 0)),
            "rt_temporal_accumulate_device", self._lib)

    def denoise_history_device(self, params, history, guides, out_ptr, dparams=None, tparams=None, stream=None):
        """rt_denoise_history_device: the variance-guided filter of a history's radiance into out_ptr (device address),
        gamma-encoded.  Enqueued on `stream`, not synchronised."""
        tp = _or_default(tparams, temporal_params)
        dp = _or_default(dparams, denoise_params)
        check(self._lib.rt_denoise_history_device(self._h, C.byref(params), C.byref(dp), C.byref(tp), C.byref(history),
                                                  C.byref(guides), C.c_void_p(out_ptr), C.c_void_p(stream or 0)),
              "rt_denoise_history_device", self._lib)

    def batch_variance_device(self, params, planes, guides, radiance_ptr, variance_ptr, dparams=None, fparams=None,
                              stream=None):
        """rt_batch_variance_device: planes an abi.RtBatchPlanes, guides an abi.RtGuides of device addresses; the radiance
        C (W*H*3 f64) and its variance (W*H f64) go to the two device addresses.  Enqueued on `stream`, not synchronised."""
        dp = _or_default(dparams, denoise_params)
        fp = _or_default(fparams, variance_filter_params)
        check(self._lib.rt_batch_variance_device(self._h, C.byref(params), C.byref(dp), C.byref(fp), C.byref(planes),
                                                 C.byref(guides), C.c_void_p(radiance_ptr), C.c_void_p(variance_ptr),
                                                 C.c_void_p(stream or 0)), "rt_batch_variance_device", self._lib)

    def denoise_variance_device(self, params, radiance_ptr, variance_ptr, guides, out_ptr, dparams=None, fparams=None,
                                stream=None):
        """rt_denoise_variance_device: the variance-guided levels over (radiance, variance) and the re-modulation into
        out_ptr (device address), gamma-encoded.  Enqueued on `stream`, not synchronised."""
        dp = _or_default(dparams, denoise_params)
        fp = _or_default(fparams, variance_filter_params)
        check(self._lib.rt_denoise_variance_device(self._h, C.byref(params), C.byref(dp), C.byref(fp), C.c_void_p(radiance_ptr),
                                                   C.c_void_p(variance_ptr), C.byref(guides), C.c_void_p(out_ptr),
                                                   C.c_void_p(stream or 0)), "rt_denoise_variance_device", self._lib)

    def render_adaptive_filtered(self, camera, params, threshold=None, pass_samples=None, min_samples=None, nee=False,
                                 heuristic=None, max_lights=None, dparams=None, fparams=None, cancel=None, on_frame=None):
        """rt_render_adaptive_filtered -> (filtered frame float64 [H, W, 3], outputs, frames): outputs a dict of every
        RtBatchOutputs plane (raw_rgb, sums, squares [H, W, 3] f64; samples, chunks [H, W] int32; tile_error
        [ceil(H/8), ceil(W/8)] f64; variance [H, W] f64), frames the callbacks' (samples_done, unfiltered copy).  nee: the
        next-event estimator with heuristic / max_lights as render_frame_nee's.  threshold, pass_samples, min_samples as
        render_adaptive's (threshold 0: the still frame); cancel and on_frame as render_progressive's."""
        ap = _adaptive(threshold, pass_samples, min_samples)
        dp = _or_default(dparams, denoise_params)
        fp = _or_default(fparams, variance_filter_params)
        ls = _light_sampling(heuristic, max_lights) if nee else None
        h, w = params.height, params.width
        frame, samples, tile_error = _adaptive_outputs(params)
        out = {"raw_rgb": np.zeros((h, w, 3)), "sums": np.zeros((h, w, 3)), "squares": np.zeros((h, w, 3)),
               "samples": samples, "chunks": np.zeros((h, w), dtype=np.int32), "tile_error": tile_error,
               "variance": np.zeros((h, w))}
        bo = abi.RtBatchOutputs(*[out[k].ctypes.data_as(t) for k, t in abi.RtBatchOutputs._fields_])
        cb, frames = _frame_collector(h, w, on_frame)
        hook = _cancel_hook(cancel)
        check(self._lib.rt_render_adaptive_filtered(self._h, C.byref(camera), C.byref(params),
                                                    C.byref(ls) if ls is not None else None, C.byref(ap), C.byref(dp),
                                                    C.byref(fp), frame.ctypes.data_as(C.POINTER(C.c_double)), C.byref(bo), cb,
                                                    None, hook, None), "rt_render_adaptive_filtered", self._lib)
        return frame, out, frames

    def variant(self):
        """rtdev_scene_variant: which trace kernel rt_scene_create_ex chose -> dict of abi.VARIANT_FIELDS."""
        out = (C.c_int32 * len(abi.VARIANT_FIELDS))()
        rc = self._lib.rtdev_scene_variant(self._h, out, len(out))
        if rc != abi.RT_OK:
            raise RtError(rc, "rtdev_scene_variant", "")
        return dict(zip(abi.VARIANT_FIELDS, out))

    def last_stats(self):
        st = abi.RtRenderStats()
        check(self._lib.rt_scene_last_stats(self._h, C.byref(st)), "rt_scene_last_stats", self._lib)
        return st


class Temporal:
    """RtTemporal handle: the history of a width x height stream of frames on one device (rt_temporal_create)."""

    def __init__(self, width, height, device=0, library=None):
        self._lib = library or lib()
        self._h = C.c_void_p()
        check(self._lib.rt_temporal_create(device, width, height, C.byref(self._h)), "rt_temporal_create", self._lib)
        self.width, self.height, self.device = width, height, device

    def render(self, scene, camera, params, tparams=None, dparams=None, with_length=False):
        """rt_render_temporal: the frame of (camera, params) accumulated into the history and filtered -> float64 [H, W, 3],
        or (frame, history length float64 [H, W]) with with_length.  The caller advances params.seed from frame to frame:
        equal seeds trace equal samples."""
        tp = _or_default(tparams, temporal_params)
        dp = _or_default(dparams, denoise_params)
        out = np.zeros((params.height, params.width, 3), dtype=np.float64)
        length = np.zeros((params.height, params.width), dtype=np.float64) if with_length else None
        check(self._lib.rt_render_temporal(scene._h, self._h, C.byref(camera), C.byref(params), C.byref(tp), C.byref(dp),
                                           out.ctypes.data_as(C.POINTER(C.c_double)),
                                           length.ctypes.data_as(C.POINTER(C.c_double)) if with_length else None),
              "rt_render_temporal", self._lib)
        return (out, length) if with_length else out

    def reset(self):
        """rt_temporal_reset: the next frame starts a new history."""
        check(self._lib.rt_temporal_reset(self._h), "rt_temporal_reset", self._lib)

    def close(self):
        if self._h:
            self._lib.rt_temporal_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
