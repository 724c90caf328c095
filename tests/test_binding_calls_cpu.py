"""The ctypes binding (racer-tracer_amd/__init__.py) held to abi.PROTOTYPES, without a GPU and without the built library.

A stub stands in for the loaded library.  It answers every symbol of abi.PROTOTYPES / abi.DEV_PROTOTYPES with a recorder
that checks the call against the symbol's argtypes (count, and from_param of every argument, which is what ctypes itself
would do at a real call), and nothing else.  The tests then look at what the wrappers handed over: which symbol, which
library, NULL or not, which struct values, and what the callbacks they built do when the "library" invokes them.
tests/test_abi_layout.py holds PROTOTYPES itself to include/rt_abi.h."""
import ctypes as C
import importlib

import numpy as np
import pytest

abi = importlib.import_module("racer-tracer_amd.abi")

W, H = 4, 3
CAM = abi.RtCamera()
P = abi.render_params(W, H, 2)
ALL_PROTOTYPES = dict(abi.PROTOTYPES, **abi.DEV_PROTOTYPES)
CREATE = ("rt_scene_create", "rt_scene_create_ex", "rt_temporal_create")


def public_fields(struct):
    return [k for k, _ in struct._fields_ if not k.startswith("_")]


def stub_default(struct, field):
    """The recognisable value the stub's *_default functions give a field."""
    return 41 + [k for k, _ in struct._fields_].index(field)


class StubLibrary:
    """Stands in for a loaded libracer_tracer_amd.so: see the module docstring.  `calls` is the log of (symbol, args);
    `rc` what the int-returning functions return; `message` the last-error text; `during[symbol]` a function(args) run
    inside a call, where the real library would invoke the callbacks it was given."""

    def __init__(self, message=b""):
        self.calls, self.rc, self.message, self.during, self.version = [], abi.RT_OK, message, {}, abi.ABI_VERSION

    def __getattr__(self, name):
        if name not in ALL_PROTOTYPES:
            raise AttributeError(name)
        restype, argtypes = ALL_PROTOTYPES[name]

        def recorder(*args):
            assert len(args) == len(argtypes), "%s takes %d arguments, got %d" % (name, len(argtypes), len(args))
            for i, (t, a) in enumerate(zip(argtypes, args)):
                try:
                    t.from_param(a)
                except (TypeError, C.ArgumentError) as e:
                    raise AssertionError("%s argument %d: %r is no %s (%s)" % (name, i, a, t.__name__, e))
            self.calls.append((name, args))
            if name == "rt_abi_version":
                return self.version
            if restype is C.c_char_p:
                return self.message if name == "rt_last_error_message" else b"stub error"
            if name.endswith("_default"):
                for k in public_fields(type(args[0]._obj)):
                    setattr(args[0]._obj, k, stub_default(type(args[0]._obj), k))
            if name in CREATE and self.rc == abi.RT_OK:
                args[-1]._obj.value = 1
            if name in self.during:
                self.during[name](args)
            return None if restype is None else self.rc
        return recorder

    def symbols(self):
        return [name for name, _ in self.calls]

    def last(self, name):
        return [args for n, args in self.calls if n == name][-1]


@pytest.fixture
def stub(rt, monkeypatch):
    """The default library of the binding, for one test (the session's `rt` module gets its own back)."""
    s = StubLibrary(b"first says no")
    monkeypatch.setattr(rt, "_lib", s)
    return s


def arg_of(name, args, argtype):
    """The one argument of a recorded call whose declared type is `argtype`."""
    argtypes = ALL_PROTOTYPES[name][1]
    assert argtypes.count(argtype) == 1, (name, argtype)
    return args[argtypes.index(argtype)]


# ---- the wrappers, by what they take ------------------------------------------------------------------------------
# name -> (call(rt, scene, **keywords), the symbol it must reach)

MULTI = {
    "render_frame_multi": (lambda rt, sc, **kw: rt.render_frame_multi([sc, sc], CAM, P, **kw), "rt_render_frame_multi"),
    "render_frame_multi_device": (lambda rt, sc, **kw: rt.render_frame_multi_device([sc, sc], CAM, P, 0x1000, **kw),
                                  "rt_render_frame_multi_device"),
    "render_tiles_multi": (lambda rt, sc, **kw: rt.render_tiles_multi([sc, sc], CAM, P, **kw), "rt_render_multi"),
    "render_frame_nee_multi": (lambda rt, sc, **kw: rt.render_frame_nee_multi([sc, sc], CAM, P, **kw),
                               "rt_render_frame_nee_multi"),
    "render_frame_nee_multi_device": (lambda rt, sc, **kw: rt.render_frame_nee_multi_device([sc, sc], CAM, P, 0x1000, **kw),
                                      "rt_render_frame_nee_multi_device"),
    "render_tiles_nee_multi": (lambda rt, sc, **kw: rt.render_tiles_nee_multi([sc, sc], CAM, P, **kw), "rt_render_nee_multi"),
}
METHODS = {
    "render_frame": (lambda rt, sc, **kw: sc.render_frame(CAM, P, **kw), "rt_render_frame"),
    "render_frame_nee": (lambda rt, sc, **kw: sc.render_frame_nee(CAM, P, **kw), "rt_render_frame_nee"),
    "render_frame_nee_device": (lambda rt, sc, **kw: sc.render_frame_nee_device(CAM, P, 0x1000, **kw),
                                "rt_render_frame_nee_device"),
    "render_frame_nee_strips_device": (lambda rt, sc, **kw: sc.render_frame_nee_strips_device(CAM, P, 0x1000, **kw),
                                       "rt_render_frame_nee_strips_device"),
    "lights": (lambda rt, sc, **kw: sc.lights(**kw), "rt_scene_lights"),
    "set_lights": (lambda rt, sc, **kw: sc.set_lights(abi.RT_LIGHTS_ALL, abi.RT_PICK_POWER, **kw), "rt_scene_set_lights"),
    "light_weights": (lambda rt, sc, **kw: sc.light_weights(**kw), "rt_scene_light_weights"),
    "render_frame_device": (lambda rt, sc, **kw: sc.render_frame_device(CAM, P, 0x1000, **kw), "rt_render_frame_device"),
    "render_frame_rgba8": (lambda rt, sc, **kw: sc.render_frame_rgba8(CAM, P, abi.RtToneMap(), **kw), "rt_render_frame_rgba8"),
    "post_rgba8_device": (lambda rt, sc, **kw: sc.post_rgba8_device(abi.RtToneMap(), 0x1000, W * H, 0x2000, **kw),
                          "rt_post_rgba8_device"),
    "render_tiles": (lambda rt, sc, **kw: sc.render_tiles(CAM, P, **kw), "rt_render"),
    "render_progressive": (lambda rt, sc, **kw: sc.render_progressive(CAM, P, 1, **kw), "rt_render_progressive"),
    "render_adaptive": (lambda rt, sc, **kw: sc.render_adaptive(CAM, P, **kw), "rt_render_adaptive"),
    "render_progressive_nee": (lambda rt, sc, **kw: sc.render_progressive_nee(CAM, P, 1, **kw), "rt_render_progressive_nee"),
    "render_adaptive_nee": (lambda rt, sc, **kw: sc.render_adaptive_nee(CAM, P, **kw), "rt_render_adaptive_nee"),
    "render_tiles_nee": (lambda rt, sc, **kw: sc.render_tiles_nee(CAM, P, **kw), "rt_render_nee"),
    "denoise_device": (lambda rt, sc, **kw: sc.denoise_device(P, 0x1000, abi.RtGuides(), 0x2000, **kw), "rt_denoise_device"),
    "denoise": (lambda rt, sc, **kw: sc.denoise(CAM, P, np.zeros((H, W, 3)), **kw), "rt_denoise_frame"),
    "temporal_accumulate_device": (lambda rt, sc, **kw: sc.temporal_accumulate_device(P, 0x1000, abi.RtGuides(),
                                                                                       abi.RtHistory(), **kw),
                                   "rt_temporal_accumulate_device"),
    "denoise_history_device": (lambda rt, sc, **kw: sc.denoise_history_device(P, abi.RtHistory(), abi.RtGuides(), 0x2000, **kw),
                               "rt_denoise_history_device"),
    "batch_variance_device": (lambda rt, sc, **kw: sc.batch_variance_device(P, abi.RtBatchPlanes(), abi.RtGuides(), 0x1000,
                                                                             0x2000, **kw), "rt_batch_variance_device"),
    "denoise_variance_device": (lambda rt, sc, **kw: sc.denoise_variance_device(P, 0x1000, 0x2000, abi.RtGuides(), 0x3000, **kw),
                                "rt_denoise_variance_device"),
    "render_adaptive_filtered": (lambda rt, sc, **kw: sc.render_adaptive_filtered(CAM, P, **kw), "rt_render_adaptive_filtered"),
    "variant": (lambda rt, sc, **kw: sc.variant(**kw), "rtdev_scene_variant"),
    "last_stats": (lambda rt, sc, **kw: sc.last_stats(**kw), "rt_scene_last_stats"),
}
SITES = dict(MULTI, **METHODS)
# the other forms of three of them: the keywords that select the form, and the symbol then
FORMS = {
    "render_tiles(flag)": ("render_tiles", {"cancel": C.pointer(C.c_int(0))}, "rt_render"),
    "render_tiles(callable)": ("render_tiles", {"cancel": lambda: False}, "rt_render_ex"),
    "render_progressive(False)": ("render_progressive", {"denoise": False}, "rt_render_progressive"),
    "render_progressive(True)": ("render_progressive", {"denoise": True}, "rt_render_progressive_denoised"),
    "render_adaptive_filtered(nee)": ("render_adaptive_filtered", {"nee": True}, "rt_render_adaptive_filtered"),
}
MODULE_HELPERS = {
    "classify": (lambda rt: rt.classify(abi.RtSceneDesc()), "rtdev_scene_classify"),
    "radiance_bound": (lambda rt: rt.radiance_bound(abi.RtSceneDesc()), "rtdev_scene_radiance_bound"),
    "sum_exponent": (lambda rt: rt.sum_exponent(2.0, 64), "rtdev_sum_exponent"),
    "progressive_passes": (lambda rt: rt.progressive_passes(64, 8), "rtdev_progressive_passes"),
    "nee_stream_chunk": (lambda rt: rt.nee_stream_chunk(), "rtdev_nee_stream_chunk"),
    "device_count": (lambda rt: rt.device_count(), "rt_device_count"),
}
PARAMS = {
    "denoise_params": (abi.RtDenoiseParams, "rt_denoise_params_default"),
    "adaptive_params": (abi.RtAdaptiveParams, "rt_adaptive_params_default"),
    "light_sampling_params": (abi.RtLightSamplingParams, "rt_light_sampling_params_default"),
    "light_list_params": (abi.RtLightListParams, "rt_light_list_params_default"),
    "temporal_params": (abi.RtTemporalParams, "rt_temporal_params_default"),
    "variance_filter_params": (abi.RtVarianceFilterParams, "rt_variance_filter_params_default"),
}
# The only names of abi.PROTOTYPES that no test of this file reaches, with the reason.  Nothing else belongs here.
NOT_REACHED = {
    "rt_scene_create": "the binding always calls rt_scene_create_ex",
    "rt_release_cached_buffers": "no wrapper; tests/test_abi_layout.py calls it on the library",
    "rt_render_guides_device": "Scene.render_guides allocates on a torch device; tests/test_gpu_denoise.py covers it",
}


def names_in_docstring(rt, name, symbol):
    """Where a wrapper has a docstring, that names the symbol it reaches."""
    owner = getattr(rt, name, None) or getattr(rt.Scene, name)
    return owner.__doc__ is None or symbol in owner.__doc__


# ---- every wrapper reaches its symbol; every symbol is reached ----------------------------------------------------

def test_every_wrapper_reaches_the_symbol_its_docstring_names_and_every_symbol_is_reached(rt, stub, monkeypatch):
    reached = set()

    def reaches(call, symbol):
        before = len(stub.calls)
        call()
        assert symbol in stub.symbols()[before:], (symbol, stub.symbols()[before:])
        reached.update(stub.symbols()[before:])

    bundle = abi.SceneBundle([], [], [], abi.sky())
    scene = rt.Scene(bundle, device=2, closest_hit=abi.RT_HIT_BVH, kernel=abi.RT_KERNEL_V1, arithmetic=abi.RT_ARITH_REFERENCE,
                     gather=abi.RT_GATHER_STAGED, launch_blocks=3)
    desc, device, opt, handle = stub.last("rt_scene_create_ex")
    assert C.addressof(desc._obj) == C.addressof(bundle.desc) and device == 2 and handle._obj is scene._h
    assert (opt._obj.closest_hit, opt._obj.kernel, opt._obj.arithmetic, opt._obj.gather) == (2, 1, 1, 1)
    assert opt._obj.launch_blocks == 3 and list(opt._obj._reserved) == [0, 0, 0]
    assert scene._h.value == 1 and scene._lib is stub and scene._desc_owner is bundle and scene.device == 2
    assert "rt_scene_create_ex" in rt.Scene.__init__.__doc__
    for name, (call, symbol) in SITES.items():
        reaches(lambda: call(rt, scene), symbol)
        assert names_in_docstring(rt, name, symbol), name
    for label, (name, keywords, symbol) in FORMS.items():
        reaches(lambda: SITES[name][0](rt, scene, **keywords), symbol)
        assert names_in_docstring(rt, name, symbol), label
    for name, (call, symbol) in MODULE_HELPERS.items():
        reaches(lambda: call(rt), symbol)
        assert names_in_docstring(rt, name, symbol), name
    reaches(lambda: rt.nee_stream_chunk(abi.RT_ARITH_REFERENCE), "rtdev_nee_stream_chunk_exact")
    for name, (_struct, symbol) in PARAMS.items():
        reaches(lambda: getattr(rt, name)(), symbol)
        assert names_in_docstring(rt, name, symbol), name

    temporal = rt.Temporal(W, H, device=1)
    assert stub.last("rt_temporal_create")[:3] == (1, W, H) and temporal._h.value == 1
    assert (temporal.width, temporal.height, temporal.device) == (W, H, 1) and "rt_temporal_create" in rt.Temporal.__doc__
    reaches(lambda: temporal.render(scene, CAM, P), "rt_render_temporal")
    assert "rt_render_temporal" in rt.Temporal.render.__doc__
    reaches(temporal.reset, "rt_temporal_reset")
    assert "rt_temporal_reset" in rt.Temporal.reset.__doc__
    # close() hands the handle to the destroy function once, and only while there is one
    for obj, destroy in ((temporal, "rt_temporal_destroy"), (scene, "rt_scene_destroy")):
        reaches(obj.close, destroy)
        assert stub.last(destroy)[0].value == 1 and not obj._h
        obj.close()
        assert stub.symbols().count(destroy) == 1

    # a refused call reads the error name and the last-error text
    stub.rc = abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(rt.RtError) as e:
        rt.Scene(bundle)
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
    assert str(e.value) == "rt_scene_create_ex failed: [102] stub error: first says no"
    assert stub.last("rt_strerror") == (abi.RT_ERR_INVALID_ARGUMENT,)
    stub.rc = abi.RT_OK

    # load_library: the default library first, then the other one bound and asked for its version
    other = StubLibrary()
    monkeypatch.setattr(rt.C, "CDLL", lambda path: other)
    assert rt.load_library("/elsewhere/lib.so") is other and other.symbols() == ["rt_abi_version"]
    other.version = abi.ABI_VERSION + 1
    with pytest.raises(ImportError, match="ABI version mismatch"):
        rt.load_library("/elsewhere/lib.so")

    reached.update(stub.symbols() + other.symbols())
    assert set(abi.DEV_PROTOTYPES) <= reached, sorted(set(abi.DEV_PROTOTYPES) - reached)
    assert set(abi.PROTOTYPES) - reached == set(NOT_REACHED), sorted(set(abi.PROTOTYPES) - reached ^ set(NOT_REACHED))


def test_a_description_goes_in_bare_or_in_a_bundle(rt, stub):
    bundle, bare = abi.SceneBundle([], [], [], abi.sky()), abi.RtSceneDesc()
    stub.during["rtdev_scene_classify"] = lambda args: args[1].__setitem__(slice(0, 4), [3, 1, 0, 1])
    stub.during["rtdev_scene_radiance_bound"] = lambda args: setattr(args[1]._obj, "value", 15.5)
    for given, desc in ((bundle, bundle.desc), (bare, bare)):
        assert rt.classify(given) == {"prims_class": 3, "textured": 1, "specular": 0, "has_moving": 1}
        assert C.addressof(stub.last("rtdev_scene_classify")[0]._obj) == C.addressof(desc)
        assert len(stub.last("rtdev_scene_classify")[1]) == len(abi.CLASSIFY_FIELDS)
        assert rt.radiance_bound(given) == 15.5
        assert C.addressof(stub.last("rtdev_scene_radiance_bound")[0]._obj) == C.addressof(desc)
        scene = rt.Scene(given)
        assert C.addressof(stub.last("rt_scene_create_ex")[0]._obj) == C.addressof(desc)
        opt = stub.last("rt_scene_create_ex")[2]._obj    # the defaults are rt_scene_create's own: no cap on the grid
        assert (opt.closest_hit, opt.kernel, opt.arithmetic, opt.gather, opt.launch_blocks, list(opt._reserved)) == (0, 0, 0, 0, 0, [0, 0, 0])
        scene.close()


def test_the_small_helpers_hand_over_and_return_what_they_say(rt, stub):
    stub.during["rtdev_sum_exponent"] = lambda args: setattr(args[2]._obj, "value", 9)
    assert rt.sum_exponent(2, 64.0) == 9 and stub.last("rtdev_sum_exponent")[:2] == (2.0, 64)

    def passes(args):  # 70 boundaries: more than the first call's 64 slots, so the wrapper asks again with 70
        samples, pass_samples, out, capacity, n = args
        n._obj.value = 70
        for i in range(min(capacity, 70)):
            out[i] = i + 1
    stub.during["rtdev_progressive_passes"] = passes
    assert rt.progressive_passes(70, 1) == list(range(1, 71))
    assert [args[3] for name, args in stub.calls if name == "rtdev_progressive_passes"] == [64, 70]

    scene = rt.Scene(abi.RtSceneDesc())

    def listed(values):
        def fill(args):
            _scene, out, capacity, n = args
            assert capacity == 64 == len(out)
            out[0:len(values)] = values
            n._obj.value = len(values)
        return fill
    stub.during["rt_scene_lights"] = listed([5, 3])
    stub.during["rt_scene_light_weights"] = listed([0.25, 0.75])
    assert scene.lights() == [5, 3] and scene.light_weights() == [0.25, 0.75]
    scene.set_lights()
    lp = stub.last("rt_scene_set_lights")[1]._obj
    assert (lp.kinds, lp.pick) == (abi.RT_LIGHTS_PLAIN, abi.RT_PICK_UNIFORM)
    scene.set_lights(kinds=abi.RT_LIGHTS_BOXES, pick=abi.RT_PICK_POWER)
    lp = stub.last("rt_scene_set_lights")[1]._obj
    assert (lp.kinds, lp.pick) == (abi.RT_LIGHTS_BOXES, abi.RT_PICK_POWER)

    stub.during["rtdev_scene_variant"] = lambda args: args[1].__setitem__(slice(0, len(args[1])), range(len(args[1])))
    assert scene.variant() == dict(zip(abi.VARIANT_FIELDS, range(len(abi.VARIANT_FIELDS))))
    assert stub.last("rtdev_scene_variant")[2] == len(abi.VARIANT_FIELDS) == 16
    # the grid of the scene's last persistent launch follows the 14 fields of the kernel choice, in this order
    assert abi.VARIANT_FIELDS[12:] == ("blocks_per_cu", "blocks_per_cu_lens", "last_launch_blocks", "last_launch_items")
    stub.during["rt_scene_last_stats"] = lambda args: setattr(args[1]._obj, "segments", 123)
    assert scene.last_stats().segments == 123
    # the streams and optional addresses: None is NULL / stream 0
    scene.render_frame_device(CAM, P, 0x1000)
    assert [a.value for a in stub.last("rt_render_frame_device")[3:]] == [0x1000, None]
    scene.render_frame_device(CAM, P, 0x1000, stream=0x20)
    assert [a.value for a in stub.last("rt_render_frame_device")[3:]] == [0x1000, 0x20]
    scene.post_rgba8_device(abi.RtToneMap(), 0x1000, 12, 0x2000)
    assert [getattr(a, "value", a) for a in stub.last("rt_post_rgba8_device")[2:]] == [0x1000, 12, 0x2000, None, None]
    scene.temporal_accumulate_device(P, 0x1000, abi.RtGuides(), abi.RtHistory())
    assert stub.last("rt_temporal_accumulate_device")[6:8] == (None, None)
    scene.temporal_accumulate_device(P, 0x1000, abi.RtGuides(), abi.RtHistory(), prev_camera=CAM, prev_history=abi.RtHistory())
    assert None not in stub.last("rt_temporal_accumulate_device")[6:8]
    with pytest.raises(ValueError):
        scene.denoise(CAM, P, np.zeros((H + 1, W, 3)))
    # the output arrays: shape and dtype
    assert (scene.render_frame(CAM, P).shape, scene.render_frame(CAM, P).dtype) == ((H, W, 3), np.float64)
    rgba = scene.render_frame_rgba8(CAM, P, abi.RtToneMap())
    assert (rgba.shape, rgba.dtype) == ((H, W, 4), np.uint8)
    big = abi.render_params(17, 9, 1)
    frame, samples, tile_error, frames = scene.render_adaptive(CAM, big)
    assert [(a.shape, a.dtype) for a in (frame, samples, tile_error)] == [((9, 17, 3), np.float64), ((9, 17), np.int32),
                                                                          ((2, 3), np.float64)] and frames == []
    assert [(a.shape, a.dtype) for a in scene.render_adaptive_nee(CAM, big)[:3]] == [((9, 17, 3), np.float64), ((9, 17), np.int32),
                                                                                     ((2, 3), np.float64)]
    frame, out, frames = scene.render_adaptive_filtered(CAM, big)
    assert (frame.shape, frame.dtype, frames) == ((9, 17, 3), np.float64, [])
    assert {k: (v.shape, v.dtype) for k, v in out.items()} == {
        "raw_rgb": ((9, 17, 3), np.float64), "sums": ((9, 17, 3), np.float64), "squares": ((9, 17, 3), np.float64),
        "samples": ((9, 17), np.int32), "chunks": ((9, 17), np.int32), "tile_error": ((2, 3), np.float64),
        "variance": ((9, 17), np.float64)}
    bo = stub.last("rt_render_adaptive_filtered")[8]._obj
    for k, v in out.items():
        assert C.cast(getattr(bo, k), C.c_void_p).value == v.ctypes.data, k


def test_variant_raises_with_an_empty_detail_and_does_not_read_the_last_error(rt, stub):
    scene = rt.Scene(abi.RtSceneDesc())
    stub.rc = abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(rt.RtError) as e:
        scene.variant()
    assert str(e.value) == "rtdev_scene_variant failed: [102] stub error" and e.value.code == abi.RT_ERR_INVALID_ARGUMENT
    assert "rt_last_error_message" not in stub.symbols()


@pytest.mark.parametrize("name", sorted(MULTI))
def test_no_scenes_at_all_is_for_the_default_library_to_refuse(rt, stub, name):
    symbol = MULTI[name][1]
    stub.rc = abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(rt.RtError, match="first says no"):
        getattr(rt, name)([], *([CAM, P, 0x1000] if name.endswith("_device") else [CAM, P]))
    handles, count = stub.last(symbol)[:2]
    assert count == 0 and len(handles) == 0


# ---- the cancel hook, at each of its nine sites -------------------------------------------------------------------

CANCEL_SITES = {"render_tiles_multi": "rt_render_multi", "render_tiles_nee_multi": "rt_render_nee_multi",
                "render_tiles": "rt_render_ex", "render_progressive": "rt_render_progressive",
                "render_adaptive": "rt_render_adaptive", "render_progressive_nee": "rt_render_progressive_nee",
                "render_adaptive_nee": "rt_render_adaptive_nee", "render_tiles_nee": "rt_render_nee",
                "render_adaptive_filtered": "rt_render_adaptive_filtered"}


@pytest.mark.parametrize("name", sorted(CANCEL_SITES))
def test_cancel_none_is_a_null_hook_and_a_callable_is_asked(rt, stub, name):
    scene, symbol = rt.Scene(abi.RtSceneDesc()), CANCEL_SITES[name]
    SITES[name][0](rt, scene, cancel=None)
    if name == "render_tiles":  # no hook to be NULL: rt_render, with a NULL flag
        assert stub.symbols()[-1] == "rt_render" and stub.last("rt_render")[-1] is None
    else:
        assert stub.symbols()[-1] == symbol and not arg_of(symbol, stub.last(symbol), abi.RtCancelCallback)
    answers, asked = iter([True, False, 1, 0, None]), []

    def ask_five_times(args):
        hook = arg_of(symbol, args, abi.RtCancelCallback)
        for _ in range(5):
            asked.append(hook(None))
    stub.during[symbol] = ask_five_times
    SITES[name][0](rt, scene, cancel=lambda: next(answers))
    assert stub.symbols()[-1] == symbol and arg_of(symbol, stub.last(symbol), abi.RtCancelCallback)
    assert asked == [1, 0, 1, 0, 0]


def test_render_tiles_has_three_forms_of_cancel(rt, stub):
    scene = rt.Scene(abi.RtSceneDesc())
    scene.render_tiles(CAM, P)
    assert stub.symbols()[-1] == "rt_render" and stub.last("rt_render")[-1] is None
    flag = C.c_int(0)
    for pointer in (C.pointer(flag), C.cast(C.pointer(flag), C.c_void_p)):
        scene.render_tiles(CAM, P, cancel=pointer)
        assert stub.symbols()[-1] == "rt_render"
        assert C.addressof(stub.last("rt_render")[-1].contents) == C.addressof(flag)
    scene.render_tiles(CAM, P, cancel=lambda: True)
    assert stub.symbols()[-1] == "rt_render_ex" and stub.last("rt_render_ex")[5](None) == 1


# ---- the frame callback --------------------------------------------------------------------------------------------

FRAME_SITES = {"render_progressive": ({}, "rt_render_progressive"),
               "render_progressive(True)": ({"denoise": True}, "rt_render_progressive_denoised"),
               "render_adaptive": ({}, "rt_render_adaptive"), "render_progressive_nee": ({}, "rt_render_progressive_nee"),
               "render_adaptive_nee": ({}, "rt_render_adaptive_nee"),
               "render_adaptive_filtered": ({}, "rt_render_adaptive_filtered")}


@pytest.mark.parametrize("label", sorted(FRAME_SITES))
@pytest.mark.parametrize("with_on_frame", [False, True])
def test_frames_are_independent_copies_and_on_frame_gets_those_objects(rt, stub, label, with_on_frame):
    scene, (keywords, symbol) = rt.Scene(abi.RtSceneDesc()), FRAME_SITES[label]
    buffer = (C.c_double * (H * W * 3))()

    def two_passes(args):  # one buffer, overwritten between the passes and after them, as the library's pinned frame is
        callback = arg_of(symbol, args, abi.RtFrameCallback)
        for samples_done in (1, 2):
            buffer[:] = [samples_done + i / 100.0 for i in range(len(buffer))]
            callback(None, buffer, samples_done, 2)
        buffer[:] = [-1.0] * len(buffer)
    stub.during[symbol] = two_passes
    seen = []
    if with_on_frame:
        keywords = dict(keywords, on_frame=lambda samples_done, frame: seen.append((samples_done, frame)))
    result = SITES[label.split("(")[0]][0](rt, scene, **keywords)
    frames = result if label.startswith("render_progressive") else result[-1]
    assert [n for n, _ in frames] == [1, 2]
    for n, frame in frames:
        assert frame.shape == (H, W, 3) and frame.dtype == np.float64 and frame.flags.owndata
        assert np.array_equal(frame.ravel(), [n + i / 100.0 for i in range(H * W * 3)])
    assert not np.shares_memory(frames[0][1], frames[1][1])
    assert len(seen) == (2 if with_on_frame else 0)
    for (n, frame), (seen_n, seen_frame) in zip(frames, seen):
        assert seen_n == n and seen_frame is frame


# ---- the tile callbacks --------------------------------------------------------------------------------------------

def two_tiles(symbol):
    """The library's side of a tile stream: one 2x2 tile at row 1, column 1, from a buffer it then overwrites, and one
    empty tile (no pixels, no buffer)."""
    def during(args):
        callback = arg_of(symbol, args, abi.RtTileCallback)
        buffer = (C.c_double * 12)(*[10.0 + i for i in range(12)])
        callback(None, buffer, 1, 1, 2, 2)
        buffer[:] = [-1.0] * 12
        callback(None, None, 0, 3, 0, 2)
    return during


@pytest.mark.parametrize("name", ["render_tiles_nee", "render_tiles_nee_multi"])
@pytest.mark.parametrize("with_on_tile", [False, True])
def test_nee_tiles_are_assembled_and_an_empty_tile_is_still_reported(rt, stub, name, with_on_tile):
    scene, symbol = rt.Scene(abi.RtSceneDesc()), SITES[name][1]
    stub.during[symbol] = two_tiles(symbol)
    seen = []
    frame, order = SITES[name][0](rt, scene, **({"on_tile": lambda *tile: seen.append(tile)} if with_on_tile else {}))
    want = np.zeros((H, W, 3))
    want[1:3, 1:3] = np.arange(10.0, 22.0).reshape(2, 2, 3)
    assert frame.dtype == np.float64 and np.array_equal(frame, want)
    assert order == [(1, 1, 2, 2), (0, 3, 0, 2)]
    assert seen == (order if with_on_tile else [])


@pytest.mark.parametrize("name,keywords,symbol", [("render_tiles", {}, "rt_render"),
                                                  ("render_tiles", {"cancel": lambda: False}, "rt_render_ex"),
                                                  ("render_tiles_multi", {}, "rt_render_multi")])
def test_tile_lists_hold_copies_and_a_zero_sized_array_for_an_empty_tile(rt, stub, name, keywords, symbol):
    scene = rt.Scene(abi.RtSceneDesc())
    stub.during[symbol] = two_tiles(symbol)
    tiles = SITES[name][0](rt, scene, **keywords)
    assert [t[:4] for t in tiles] == [(1, 1, 2, 2), (0, 3, 0, 2)]
    assert np.array_equal(tiles[0][4], np.arange(10.0, 22.0).reshape(2, 2, 3)) and tiles[0][4].flags.owndata
    assert tiles[1][4].shape == (2, 0, 3) and tiles[1][4].dtype == np.float64


# ---- None keeps the default, a value overrides its own field -------------------------------------------------------

def assert_fields(struct, **given):
    for k in public_fields(type(struct)):
        assert getattr(struct, k) == given.get(k, stub_default(type(struct), k)), (k, given)


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_params_functions_fill_the_defaults_and_override_by_keyword(rt, stub, name):
    struct, symbol = PARAMS[name]
    got = getattr(rt, name)()
    assert type(got) is struct and stub.symbols() == [symbol]
    assert_fields(got)
    for k in public_fields(struct):
        assert_fields(getattr(rt, name)(**{k: 7}), **{k: 7})
    everything = {k: i for i, k in enumerate(public_fields(struct))}
    assert_fields(getattr(rt, name)(**everything), **everything)
    with pytest.raises(AttributeError):
        stub.no_such_symbol


LIGHT_SAMPLING_SITES = ["render_frame_nee_multi", "render_frame_nee_multi_device", "render_tiles_nee_multi", "render_frame_nee",
                        "render_frame_nee_device", "render_frame_nee_strips_device", "render_progressive_nee",
                        "render_adaptive_nee", "render_tiles_nee", "render_adaptive_filtered"]


@pytest.mark.parametrize("name", LIGHT_SAMPLING_SITES)
def test_heuristic_and_max_lights_none_keep_the_defaults(rt, stub, name):
    scene, (call, symbol) = rt.Scene(abi.RtSceneDesc()), SITES[name]
    always = {"nee": True} if name == "render_adaptive_filtered" else {}
    for given in ({}, {"heuristic": None, "max_lights": None}, {"heuristic": abi.RT_MIS_BALANCE}, {"max_lights": 7},
                  {"heuristic": abi.RT_MIS_POWER, "max_lights": 0}):
        call(rt, scene, **dict(given, **always))
        ls = arg_of(symbol, stub.last(symbol), C.POINTER(abi.RtLightSamplingParams))
        assert_fields(ls._obj, **{k: v for k, v in given.items() if v is not None})


@pytest.mark.parametrize("name", ["render_adaptive", "render_adaptive_nee", "render_adaptive_filtered"])
def test_the_adaptive_triple_none_keeps_the_defaults(rt, stub, name):
    scene, (call, symbol) = rt.Scene(abi.RtSceneDesc()), SITES[name]
    for given in ({}, {"threshold": None, "pass_samples": None, "min_samples": None}, {"threshold": 0.0}, {"threshold": 0.125},
                  {"pass_samples": 16}, {"min_samples": 0}, {"threshold": 0.5, "pass_samples": 8, "min_samples": 24}):
        call(rt, scene, **given)
        ap = arg_of(symbol, stub.last(symbol), C.POINTER(abi.RtAdaptiveParams))
        assert_fields(ap._obj, **{k: v for k, v in given.items() if v is not None})


BLOCK_SITES = {  # name -> the keywords it has for parameter blocks
    "denoise_device": ("dparams",), "denoise": ("dparams",), "temporal_accumulate_device": ("tparams", "dparams"),
    "denoise_history_device": ("dparams", "tparams"), "batch_variance_device": ("dparams", "fparams"),
    "denoise_variance_device": ("dparams", "fparams"), "render_adaptive_filtered": ("dparams", "fparams"),
    "Temporal.render": ("tparams", "dparams")}
BLOCKS = {"dparams": abi.RtDenoiseParams, "tparams": abi.RtTemporalParams, "fparams": abi.RtVarianceFilterParams}


@pytest.mark.parametrize("name", sorted(BLOCK_SITES))
def test_a_parameter_block_is_the_callers_or_the_defaults(rt, stub, name):
    scene = rt.Scene(abi.RtSceneDesc())
    if name == "Temporal.render":
        temporal = rt.Temporal(W, H)
        call, symbol = lambda rt, sc, **kw: temporal.render(sc, CAM, P, **kw), "rt_render_temporal"
    else:
        call, symbol = SITES[name]
    call(rt, scene)
    for keyword in BLOCK_SITES[name]:
        assert_fields(arg_of(symbol, stub.last(symbol), C.POINTER(BLOCKS[keyword]))._obj)
    for keyword in BLOCK_SITES[name]:
        mine = BLOCKS[keyword]()
        call(rt, scene, **{keyword: mine})
        for k in BLOCK_SITES[name]:
            block = arg_of(symbol, stub.last(symbol), C.POINTER(BLOCKS[k]))._obj
            if k == keyword:
                assert block is mine
            else:
                assert_fields(block)


# ---- the forms of three calls --------------------------------------------------------------------------------------

def test_render_progressive_has_four_forms_of_denoise(rt, stub):
    scene = rt.Scene(abi.RtSceneDesc())
    for denoise in (None, False):
        before = len(stub.calls)
        assert scene.render_progressive(CAM, P, 3, denoise=denoise) == []
        assert stub.symbols()[before:] == ["rt_render_progressive"] and stub.last("rt_render_progressive")[3] == 3
    scene.render_progressive(CAM, P, 3, denoise=True)
    assert stub.symbols()[-2:] == ["rt_denoise_params_default", "rt_render_progressive_denoised"]
    assert stub.last("rt_render_progressive_denoised")[3] == 3
    assert_fields(stub.last("rt_render_progressive_denoised")[4]._obj)
    mine = abi.RtDenoiseParams(iterations=2)
    before = len(stub.calls)
    scene.render_progressive(CAM, P, 3, denoise=mine)
    assert stub.symbols()[before:] == ["rt_render_progressive_denoised"]
    assert stub.last("rt_render_progressive_denoised")[4]._obj is mine


def test_render_adaptive_filtered_passes_no_light_sampling_without_nee(rt, stub):
    scene = rt.Scene(abi.RtSceneDesc())
    scene.render_adaptive_filtered(CAM, P, heuristic=abi.RT_MIS_BALANCE, max_lights=3)
    assert stub.last("rt_render_adaptive_filtered")[3] is None
    assert "rt_light_sampling_params_default" not in stub.symbols()
    scene.render_adaptive_filtered(CAM, P, nee=True, heuristic=abi.RT_MIS_BALANCE, max_lights=3)
    assert_fields(stub.last("rt_render_adaptive_filtered")[3]._obj, heuristic=abi.RT_MIS_BALANCE, max_lights=3)


def test_temporal_render_passes_a_length_plane_only_when_asked(rt, stub):
    scene, temporal = rt.Scene(abi.RtSceneDesc()), rt.Temporal(W, H)
    stub.during["rt_render_temporal"] = lambda args: [p.__setitem__(0, 0.5) for p in args[6:] if p is not None]
    out = temporal.render(scene, CAM, P)
    assert stub.last("rt_render_temporal")[7] is None
    assert (out.shape, out.dtype, out[0, 0, 0]) == ((H, W, 3), np.float64, 0.5)
    out, length = temporal.render(scene, CAM, P, with_length=True)
    assert stub.last("rt_render_temporal")[7] is not None
    assert (out.shape, out.dtype, length.shape, length.dtype, length[0, 0]) == ((H, W, 3), np.float64, (H, W), np.float64, 0.5)
    assert [a.value for a in stub.last("rt_render_temporal")[:2]] == [1, 1]


# ---- a scene of another loaded library ------------------------------------------------------------------------------

def test_a_scene_of_another_library_sends_every_call_there(rt, stub):
    """Every method of a Scene / Temporal made with library=..., and all six multi-scene functions given such scenes, call
    that library and read its last-error text.  The one thing the default library still does is fill parameter blocks:
    the *_params functions are the default library's, whatever scene their result goes to (they touch no handle)."""
    second = StubLibrary(b"second says no")
    scene, temporal = rt.Scene(abi.RtSceneDesc(), library=second), rt.Temporal(W, H, library=second)
    assert scene._lib is second and temporal._lib is second and second.symbols() == ["rt_scene_create_ex", "rt_temporal_create"]
    calls = dict(SITES)
    calls.update({label: (lambda rt, sc, name=name, kw=kw: SITES[name][0](rt, sc, **kw), symbol)
                  for label, (name, kw, symbol) in FORMS.items()})
    calls["Temporal.render"] = (lambda rt, sc: temporal.render(sc, CAM, P), "rt_render_temporal")
    calls["Temporal.reset"] = (lambda rt, sc: temporal.reset(), "rt_temporal_reset")
    for label, (call, symbol) in calls.items():
        before = len(second.calls)
        call(rt, scene)
        assert second.symbols()[before:] == [symbol], label
        if label in MULTI:
            handles, count = second.last(symbol)[:2]
            assert count == 2 and list(handles) == [1, 1], label
    assert set(stub.symbols()) <= {symbol for _struct, symbol in PARAMS.values()}, stub.symbols()

    second.rc = abi.RT_ERR_UNSUPPORTED
    for label, (call, symbol) in calls.items():
        if symbol == "rtdev_scene_variant":  # reads no last-error text: its own test
            continue
        with pytest.raises(rt.RtError) as e:
            call(rt, scene)
        assert str(e.value) == "%s failed: [103] stub error: second says no" % symbol, label
    assert "rt_last_error_message" not in stub.symbols()
    second.rc = abi.RT_OK
    for obj, destroy in ((temporal, "rt_temporal_destroy"), (scene, "rt_scene_destroy")):
        obj.close()
        assert second.symbols()[-1] == destroy
    assert not [s for s in stub.symbols() if s.endswith("_destroy")]
