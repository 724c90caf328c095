"""rt_render_progressive without a device: the entry point is exported and bound, refuses a NULL scene and a pass size
that is not positive, and cuts passes on the chunk boundaries that include/rt_abi.h documents."""
import ctypes as C

import pytest


def _call(rt, scene, pass_samples, callback=True):
    abi = rt.abi
    cam, params = abi.RtCamera(), abi.render_params(64, 36, 96)
    cb = abi.RtFrameCallback(lambda *_: None) if callback else C.cast(None, abi.RtFrameCallback)
    return rt.lib().rt_render_progressive(scene, C.byref(cam), C.byref(params), pass_samples, cb, None,
                                          C.cast(None, abi.RtCancelCallback), None)


def test_the_entry_point_is_exported_and_bound(rt):
    assert "rt_render_progressive" in rt.abi.PROTOTYPES
    assert hasattr(C.CDLL(rt.LIB_PATH), "rt_render_progressive")


@pytest.mark.parametrize("pass_samples", [1, 0, -5])
def test_a_null_scene_is_refused(rt, pass_samples):
    assert _call(rt, None, pass_samples) == rt.abi.RT_ERR_INVALID_ARGUMENT
    assert b"scene is NULL" in rt.lib().rt_last_error_message()


def test_pass_samples_must_be_positive(rt):
    for pass_samples in (0, -1):
        with pytest.raises(rt.RtError) as err:
            rt.progressive_passes(96, pass_samples)
        assert err.value.code == rt.abi.RT_ERR_INVALID_ARGUMENT


def test_passes_end_on_the_documented_chunk_boundaries(rt):
    # N = 96: chunk boundaries 0, 24, 48, 72, 84, 92, 96 (rt_abi.h)
    assert rt.progressive_passes(96, 1) == [24, 48, 72, 84, 92, 96]
    assert rt.progressive_passes(96, 30) == [48, 84, 96]
    assert rt.progressive_passes(96, 96) == [96]
    assert rt.progressive_passes(96, 10 ** 6) == [96]
    # C3's 1024 spp: sixteen chunks of 64 and a taper of 32, 16, 8, 8
    assert rt.progressive_passes(1024, 256) == [256, 512, 768, 1024]
    assert rt.progressive_passes(1024, 1)[-5:] == [960, 992, 1008, 1016, 1024]
    for n in (1, 7, 8, 9, 24, 100, 1000, 4096, 40000):
        for pass_samples in (1, 3, 64, n):
            done = rt.progressive_passes(n, pass_samples)
            assert done[-1] == n and done == sorted(set(done))
            assert done[:-1] == [d for d in rt.progressive_passes(n, 1) if d in done[:-1]]   # chunk boundaries only
            if pass_samples >= n:
                assert done == [n]
