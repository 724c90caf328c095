"""rt_render_progressive_nee and rt_render_adaptive_nee without a device: exported and bound, and every refusal the header
lists returned before a device is touched (a NULL scene), each with a message naming its cause."""
import ctypes as C

NEW = ("rt_render_progressive_nee", "rt_render_adaptive_nee")


def test_the_entry_points_are_exported_and_bound(rt):
    lib = C.CDLL(rt.LIB_PATH)
    for name in NEW:
        assert name in rt.abi.PROTOTYPES and hasattr(lib, name), name
    assert rt.lib().rt_abi_version() == rt.abi.ABI_VERSION
    assert hasattr(rt.Scene, "render_progressive_nee") and hasattr(rt.Scene, "render_adaptive_nee")


def _light_cases(rt, abi):
    """What rt_render_frame_nee refuses: (params or None, light sampling, word of the message)."""
    bad = rt.light_sampling_params()
    bad._reserved[5] = 1
    return [(None, rt.light_sampling_params(heuristic=2), b"heuristic"), (None, rt.light_sampling_params(heuristic=-1), b"heuristic"),
            (None, rt.light_sampling_params(max_lights=-1), b"max_lights"), (None, rt.light_sampling_params(max_lights=65), b"max_lights"),
            (None, bad, b"_reserved"),
            (abi.render_params(16, 16, 4, strip_rows=8, strip_count=2), rt.light_sampling_params(), b"strip"),
            (abi.render_params(16, 16, 4, scale=2), rt.light_sampling_params(), b"scale"),
            (None, rt.light_sampling_params(), b"scene is NULL")]


def test_progressive_refusals_come_before_the_device(rt, abi):
    lib, cam = rt.lib(), abi.RtCamera()
    cb = abi.RtFrameCallback(lambda *a: None)
    no_cb = C.cast(None, abi.RtFrameCallback)
    no_cancel = C.cast(None, abi.RtCancelCallback)

    def call(p=None, ls=None, pass_samples=4, callback=cb):
        p = p or abi.render_params(16, 16, 4)
        ls = ls if ls is not None else rt.light_sampling_params()
        return lib.rt_render_progressive_nee(None, C.byref(cam), C.byref(p), C.byref(ls), pass_samples, callback, None, no_cancel, None)

    for p, ls, word in _light_cases(rt, abi):
        assert call(p, ls) == abi.RT_ERR_INVALID_ARGUMENT, word
        assert word in lib.rt_last_error_message(), (word, lib.rt_last_error_message())
    for kw, word in ((dict(pass_samples=0), b"pass_samples"), (dict(pass_samples=-3), b"pass_samples"), (dict(callback=no_cb), b"callback")):
        assert call(**kw) == abi.RT_ERR_INVALID_ARGUMENT, kw
        assert word in lib.rt_last_error_message(), (kw, lib.rt_last_error_message())
    assert lib.rt_render_progressive_nee(None, None, None, None, 4, cb, None, no_cancel, None) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"NULL" in lib.rt_last_error_message()


def test_adaptive_refusals_come_before_the_device(rt, abi):
    lib, cam = rt.lib(), abi.RtCamera()
    out = (C.c_double * (16 * 16 * 3))()
    no_cb = C.cast(None, abi.RtFrameCallback)
    no_cancel = C.cast(None, abi.RtCancelCallback)

    def call(p=None, ls=None, ap=None, out_rgb=out, null_adaptive=False):
        p = p or abi.render_params(16, 16, 4)
        ls = ls if ls is not None else rt.light_sampling_params()
        ap = ap if ap is not None else rt.adaptive_params()
        return lib.rt_render_adaptive_nee(None, C.byref(cam), C.byref(p), C.byref(ls), None if null_adaptive else C.byref(ap), out_rgb,
                                          None, None, no_cb, None, no_cancel, None)

    for p, ls, word in _light_cases(rt, abi):
        assert call(p, ls) == abi.RT_ERR_INVALID_ARGUMENT, word
        assert word in lib.rt_last_error_message(), (word, lib.rt_last_error_message())
    reserved = rt.adaptive_params()
    reserved._reserved[3] = 1
    cases = [(dict(null_adaptive=True), b"adaptive is NULL"), (dict(out_rgb=None), b"out_rgb"),
             (dict(ap=rt.adaptive_params(threshold=float("nan"))), b"threshold"),
             (dict(ap=rt.adaptive_params(threshold=float("inf"))), b"threshold"),
             (dict(ap=rt.adaptive_params(pass_samples=0)), b"pass_samples"), (dict(ap=rt.adaptive_params(min_samples=-1)), b"min_samples"),
             (dict(ap=reserved), b"_reserved")]
    for kw, word in cases:
        assert call(**kw) == abi.RT_ERR_INVALID_ARGUMENT, kw
        assert word in lib.rt_last_error_message(), (kw, lib.rt_last_error_message())
