"""The preview upsampler without a device: include/rt_preview.h against the library and the binding's own
table, rt_preview_grid against the formula, every refusal that comes before a device is touched, the numpy model
(tests/upsample_model.py) on hand-made input, and what the definition buys on oracle renders."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import scenes_py as S
import upsample_model as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
abi = S.abi
INVALID = abi.RT_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def pv():
    return importlib.import_module("racer-tracer_amd.preview")


def declared(header):
    """{function: number of parameters} of the prototypes a header declares."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INC, header)).read(), flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(rt_\w+)\s*\(([^)]*)\)\s*;", text)}


# ---- header and prototypes ------------------------------------------------------------------------------------------

def test_the_library_exports_what_the_header_declares_and_the_table_agrees(rt, pv):
    want = declared("rt_preview.h")
    assert sorted(want) == ["rt_preview_grid", "rt_render_preview_upsampled", "rt_upsample_preview_device"]
    lib = C.CDLL(rt.LIB_PATH)
    for name, n_args in want.items():
        assert hasattr(lib, name), name
        assert len(pv.PROTOTYPES[name][1]) == n_args and pv.PROTOTYPES[name][0] is C.c_int, name
    assert sorted(pv.PROTOTYPES) == sorted(want)
    # a table of its own: the binding's two tables and the ABI version are what they were
    assert not set(want) & (set(abi.PROTOTYPES) | set(abi.DEV_PROTOTYPES))
    assert not set(want) & set(declared("rt_abi.h"))


def test_the_header_compiles_as_c():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "p.c")
        open(src, "w").write('#include "rt_preview.h"\n#include "rt_preview.h"\n'
                             "int (*grid)(const RtRenderParams *, int32_t *, int32_t *, int32_t *, int32_t *) = rt_preview_grid;\n"
                             "int main(void) { return grid == 0; }\n")
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INC, "-c", "-o", os.path.join(d, "p.o"), src])


def test_the_table_is_attached_lazily_and_once_per_library(rt, pv):
    class Recorder:
        """A library object that counts how often each symbol is looked up."""
        def __init__(self):
            self.lookups = []

        def __getattr__(self, name):
            if name not in pv.PROTOTYPES:
                raise AttributeError(name)
            self.lookups.append(name)
            fn = lambda *a: abi.RT_OK   # noqa: E731
            self.__dict__[name] = fn
            return fn
    a, b = Recorder(), Recorder()
    assert pv.bound(a) is a and pv.bound(a) is a and sorted(a.lookups) == sorted(pv.PROTOTYPES) and b.lookups == []
    assert a.rt_preview_grid.argtypes == pv.PROTOTYPES["rt_preview_grid"][1]
    assert pv.bound(b) is b and sorted(b.lookups) == sorted(pv.PROTOTYPES)

    class Scene:
        _lib, _h = b, C.c_void_p(1)
    p = abi.render_params(8, 6, 1, scale=2)
    pv.upsample_preview_device(Scene, p, 0x1000, abi.RtGuides(), 0x2000, dparams=abi.RtDenoiseParams())
    out = pv.render_preview_upsampled(Scene, abi.RtCamera(), p, dparams=abi.RtDenoiseParams())
    assert out.shape == (6, 8, 3) and out.dtype == np.float64
    out, preview = pv.render_preview_upsampled(Scene, abi.RtCamera(), p, dparams=abi.RtDenoiseParams(), with_preview=True)
    assert preview.shape == (6, 8, 3) and not np.shares_memory(out, preview)
    assert len(b.lookups) == len(pv.PROTOTYPES)   # still once

    class Old:
        def __getattr__(self, name):
            raise AttributeError(name)
    with pytest.raises(AttributeError):
        pv.bound(Old())


def test_the_default_block_is_the_upsample_alone(rt, pv):
    dp = pv._default_block(None)
    ref = rt.denoise_params()
    assert dp.iterations == 0 and (dp.flags, dp.sigma_normal, dp.sigma_plane) == (ref.flags, ref.sigma_normal, ref.sigma_plane)
    mine = abi.RtDenoiseParams()
    assert pv._default_block(mine) is mine


# ---- rt_preview_grid ------------------------------------------------------------------------------------------------

GRIDS = [((100, 45, 10, 5, 4), None), ((103, 47, 10, 5, 4), (2, 3, 102, 45)), ((64, 36, 1, 1, 7), (4, 6, 64, 36)),
         ((400, 225, 10, 10, 4), (4, 2, 400, 224)), ((96, 54, 10, 10, 1), (1, 1, 96, 54)), ((13, 7, 1, 1, 4), (1, 1, 13, 7))]


def formula(w, h, tw, th, scale):
    """DESIGN.md 4.13, written out on its own."""
    if scale <= 1:
        return 1, 1, w, h
    sx = max(d for d in range(1, scale + 1) if (w // max(tw, 1)) % d == 0)
    sy = max(d for d in range(1, scale + 1) if (h // max(th, 1)) % d == 0)
    return sx, sy, w // sx * sx, h // sy * sy


@pytest.mark.parametrize("case,stated", GRIDS, ids=["x".join(map(str, c)) for c, _ in GRIDS])
def test_the_grid_follows_the_formula(pv, case, stated):
    w, h, tw, th, scale = case
    got = pv.preview_grid(abi.render_params(w, h, 1, tiles_w=tw, tiles_h=th, scale=scale))
    assert got == formula(*case) == U.preview_grid(*case)
    if stated is not None:
        assert got == stated
    assert pv.preview_grid(abi.render_params(w, h, 1, tiles_w=tw, tiles_h=th, scale=0)) == (1, 1, w, h)
    # tiles_w = 0 counts as 1
    assert pv.preview_grid(abi.render_params(w, h, 1, tiles_w=0, tiles_h=0, scale=scale)) == formula(w, h, 1, 1, scale)


def _message(rt):
    return rt.lib().rt_last_error_message().decode()


def test_the_grid_refuses_what_a_render_refuses_about_its_fields(rt, pv):
    lib = pv.bound()
    out = [C.c_int32(0) for _ in range(4)]
    refs = [C.byref(v) for v in out]
    for what, p in (("width and height", abi.render_params(1, 45, 1, scale=4)), ("width and height", abi.render_params(100, 1, 1, scale=4)),
                    ("scale", abi.render_params(100, 45, 1, scale=-1)),
                    ("strip", abi.render_params(100, 45, 1, scale=4, strip_rows=8, strip_count=2, strip_index=0))):
        assert lib.rt_preview_grid(C.byref(p), *refs) == INVALID, what
        assert what in _message(rt)
    ok = abi.render_params(100, 45, 1, scale=4)
    assert lib.rt_preview_grid(None, *refs) == INVALID and "NULL" in _message(rt)
    for hole in range(4):
        holed = list(refs)
        holed[hole] = None
        assert lib.rt_preview_grid(C.byref(ok), *holed) == INVALID and "NULL" in _message(rt)
    assert lib.rt_preview_grid(C.byref(ok), *refs) == abi.RT_OK
    # strips without a preview scale are a render's business, not the grid's
    assert lib.rt_preview_grid(C.byref(abi.render_params(100, 45, 1, strip_rows=8, strip_count=2)), *refs) == abi.RT_OK
    assert [v.value for v in out] == [1, 1, 100, 45]


# ---- every refusal, without a device --------------------------------------------------------------------------------

def _dp(**kw):
    dp = abi.RtDenoiseParams()
    dp.iterations, dp.flags, dp.sigma_normal, dp.sigma_plane = 0, 1, 0.1, 1.0
    for k, v in kw.items():
        setattr(dp, k, v)
    return dp


def _calls(pv, params, dp, rgb="a", out="b", guides=None, host_out="b", camera=True):
    """Both upsampling entry points with a NULL scene (every refusal listed in rt_preview.h comes before the scene's)."""
    lib = pv.bound()
    bufs = {"a": (C.c_double * 3)(), "b": (C.c_double * 3)(), None: None}
    g = guides if guides is not None else abi.RtGuides(1, 2, 3, 4, 5)   # never dereferenced: the calls are refused first
    cam = abi.RtCamera()
    ptr = lambda k: C.cast(bufs[k], C.c_void_p) if k else None   # noqa: E731
    return {
        "rt_upsample_preview_device": lambda: lib.rt_upsample_preview_device(
            None, C.byref(params) if params else None, C.byref(dp) if dp else None, ptr(rgb), C.byref(g) if g else None,
            ptr(out), None),
        "rt_render_preview_upsampled": lambda: lib.rt_render_preview_upsampled(
            None, C.byref(cam) if camera else None, C.byref(params) if params else None, C.byref(dp) if dp else None,
            bufs[host_out], None),
    }


def _bad():
    ok = abi.render_params(64, 36, 8, scale=4)
    cases = [("scale", abi.render_params(64, 36, 8, scale=s), _dp()) for s in (0, 1, -3)]
    cases.append(("strip_count", abi.render_params(64, 36, 8, scale=4, strip_rows=8, strip_count=2, strip_index=0), _dp()))
    cases += [("iterations", ok, _dp(iterations=it)) for it in (-1, 11)]
    cases += [("finite", ok, _dp(**{name: v})) for name in ("sigma_color", "sigma_normal", "sigma_plane")
              for v in (float("nan"), float("inf"), -float("inf"))]
    bad = _dp()
    bad._reserved[1] = 1
    cases.append(("_reserved", ok, bad))
    cases.append(("width and height", abi.render_params(1, 36, 8, scale=4), _dp()))
    cases.append(("anchor", abi.render_params(3, 36, 8, tiles_w=8, scale=4), _dp()))   # width / tiles_w = 0: a 4-wide block
    return cases


@pytest.mark.parametrize("case", range(len(_bad())))
def test_bad_parameters_are_refused_before_a_device(rt, pv, case):
    what, params, dp = _bad()[case]
    for name, call in _calls(pv, params, dp).items():
        assert call() == INVALID, (name, what)
        msg = _message(rt)
        assert what in msg and "scene is NULL" not in msg, (name, msg)


def test_null_pointers_incomplete_guides_and_aliases_are_refused(rt, pv):
    ok, dp = abi.render_params(64, 36, 8, scale=4), _dp()
    for kw, what in ((dict(params=None), "NULL"), (dict(dp=None), "NULL")):
        for name, call in _calls(pv, **dict(dict(params=ok, dp=dp), **kw)).items():
            assert call() == INVALID and what in _message(rt), (name, kw)
    dev = lambda **kw: _calls(pv, ok, dp, **kw)["rt_upsample_preview_device"]()   # noqa: E731
    assert dev(rgb=None) == INVALID and "rgb_device" in _message(rt)
    assert dev(out=None) == INVALID and "out_device" in _message(rt)
    assert dev(out="a") == INVALID and "must differ" in _message(rt)
    for hole in range(5):
        ptrs = [1, 2, 3, 4, 5]
        ptrs[hole] = 0
        assert dev(guides=abi.RtGuides(*ptrs)) == INVALID and "guides_device" in _message(rt)
    assert pv.bound().rt_upsample_preview_device(None, C.byref(ok), C.byref(dp), C.c_void_p(8), None, C.c_void_p(16),
                                                 None) == INVALID and "guides_device" in _message(rt)
    host = lambda **kw: _calls(pv, ok, dp, **kw)["rt_render_preview_upsampled"]()   # noqa: E731
    assert host(host_out=None) == INVALID and "out_rgb_host" in _message(rt)
    assert host(camera=False) == INVALID and "camera" in _message(rt)
    # with everything else in order, the scene is what is missing: no device has been asked for
    for name, call in _calls(pv, ok, dp).items():
        assert call() == INVALID and "scene is NULL" in _message(rt), name


def test_the_wrappers_raise_with_the_message(rt, pv):
    class Scene:
        _lib, _h = rt.lib(), C.c_void_p(None)
    with pytest.raises(rt.RtError, match="scale") as e:
        pv.render_preview_upsampled(Scene, abi.RtCamera(), abi.render_params(64, 36, 8))
    assert e.value.code == INVALID
    with pytest.raises(rt.RtError, match="scene is NULL"):
        pv.upsample_preview_device(Scene, abi.render_params(64, 36, 8, scale=4), 8, abi.RtGuides(1, 2, 3, 4, 5), 16)
    with pytest.raises(rt.RtError, match="width and height"):
        pv.preview_grid(abi.render_params(1, 1, 1))


# ---- the model ------------------------------------------------------------------------------------------------------

def flat_guides(h, w, oid=1):
    g = {"normal": np.zeros((h, w, 3)), "position": np.zeros((h, w, 3)), "albedo": np.ones((h, w, 3)),
         "footprint": np.full((h, w), 0.01), "obj_id": np.full((h, w), oid, dtype=np.int32)}
    g["normal"][..., 2] = 1.0
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    g["position"][..., 0], g["position"][..., 1] = 0.01 * xs, 0.01 * ys
    return g


def as_misses(g, where):
    g["obj_id"][where] = -1
    g["normal"][where] = 0.0
    g["position"][where] = 0.0
    g["albedo"][where] = 1.0
    g["footprint"][where] = np.inf


def test_a_flat_object_is_interpolated_bilinearly_in_the_squares():
    w, h, sx, sy = 14, 11, 4, 3   # GX = 3 (two uncovered columns), GY = 3 (two uncovered rows)
    rng = np.random.default_rng(5)
    frame = U.replicate(rng.uniform(0.1, 2.0, (h, w, 3)), sx, sy, 12, 9)
    got = U.upsample(frame, flat_guides(h, w), sx, sy, flags=0, sigma_normal=0.0, sigma_plane=0.0)
    a = frame[0:9:sy, 0:12:sx] ** 2   # the anchors' squares [3, 3, 3]
    for y in range(h):
        for x in range(w):
            i0, j0 = min(x // sx, 2), min(y // sy, 2)
            i1, j1 = min(i0 + 1, 2), min(j0 + 1, 2)
            tx = (x - i0 * sx) / sx if i1 != i0 else 0.0
            ty = (y - j0 * sy) / sy if j1 != j0 else 0.0
            want = (1 - ty) * ((1 - tx) * a[j0, i0] + tx * a[j0, i1]) + ty * ((1 - tx) * a[j1, i0] + tx * a[j1, i1])
            assert np.allclose(got[y, x] ** 2, want, rtol=1e-14, atol=0.0), (x, y)
    # anchors come back as they are, and the last block of a row or column, like the uncovered edge behind it, repeats its anchor
    assert np.allclose(got[0:9:sy, 0:12:sx], frame[0:9:sy, 0:12:sx], rtol=1e-15)
    assert np.array_equal(got[:, 8:], np.repeat(got[:, 8:9], w - 8, axis=1))
    assert np.array_equal(got[6:, :], np.repeat(got[6:7, :], h - 6, axis=0))
    # the stops, on: a flat object at a constant normal loses nothing to them
    assert np.allclose(U.upsample(frame, flat_guides(h, w), sx, sy, flags=0), got, rtol=1e-13)


def test_a_pixel_none_of_whose_anchors_shares_its_id_keeps_its_input_bit_for_bit():
    w, h, s = 12, 12, 4
    g = flat_guides(h, w)
    g["obj_id"][5, 6] = 9     # an island inside block (1, 1): anchors (4,4) (4,8) (8,4) (8,8) are object 1
    g["obj_id"][10, 11] = 9   # ... and one in the last block
    rng = np.random.default_rng(6)
    frame = U.replicate(rng.uniform(0.1, 2.0, (h, w, 3)), s, s, w, h)
    for flags in (0, U.DEMODULATE):
        got = U.upsample(frame, g, s, s, flags=flags)
        assert np.array_equal(got[5, 6], frame[4, 4]) and np.array_equal(got[5, 6], frame[5, 6])
        assert np.array_equal(got[10, 11], frame[8, 8])
    # an anchor of another object gives nothing to its neighbours: changing it changes only pixels of its own id
    other = frame.copy()
    g["obj_id"][4, 4] = 9
    other[4, 4] *= 3.0
    a, b = U.upsample(frame, g, s, s), U.upsample(other, g, s, s)
    changed = np.any(a != b, axis=-1)
    assert changed[5, 6] and not changed[g["obj_id"] == 1].any()


def test_misses_interpolate_between_misses_only():
    w, h, s = 12, 8, 4
    g = flat_guides(h, w)
    sky = np.zeros((h, w), dtype=bool)
    sky[:, :6] = True   # anchors in columns 0 and 4 are sky, column 8 is the object
    as_misses(g, sky)
    full = np.zeros((h, w, 3))
    full[..., :] = np.linspace(0.2, 1.0, w)[None, :, None]
    full[~sky] = 5.0
    frame = U.replicate(full, s, s, w, h)
    got = U.upsample(frame, g, s, s)   # demodulation on: albedo 1 on a miss
    for x in range(4):   # between two sky anchors: the blend of their squares
        t = x / 4.0
        assert np.allclose(got[0, x] ** 2, (1 - t) * frame[0, 0] ** 2 + t * frame[0, 4] ** 2, rtol=1e-14)
    for x in (4, 5):     # sky pixels whose right anchor is the object: the sky anchor alone
        assert np.allclose(got[:, x], frame[:, 4], rtol=1e-14)
    for x in (6, 7):     # object pixels whose left anchor is sky: the object anchor alone
        assert np.allclose(got[:, x], 5.0, rtol=1e-14)
    # a frame of misses only: plain bilinear interpolation, nothing skipped
    as_misses(g, np.ones((h, w), dtype=bool))
    got = U.upsample(frame, g, s, s)
    want = U.upsample(frame, flat_guides(h, w), s, s, flags=0, sigma_normal=0.0, sigma_plane=0.0)
    assert np.array_equal(got, want)


def test_demodulation_restores_albedo_detail_at_full_resolution():
    w, h, s = 16, 12, 4
    g = flat_guides(h, w)
    rng = np.random.default_rng(7)
    g["albedo"] = rng.uniform(0.05, 1.0, (h, w, 3))   # texture detail finer than the preview's blocks
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    smooth = (0.3 + 0.02 * xs + 0.01 * ys)[..., None] * np.ones(3)   # linear in the image: bilinear blending is exact
    truth = np.sqrt(g["albedo"] * smooth)
    frame = U.replicate(truth, s, s, w, h)
    got = U.upsample(frame, g, s, s, sigma_normal=0.0, sigma_plane=0.0)
    inner = (slice(0, h - s + 1), slice(0, w - s + 1))   # between anchors; the last blocks repeat their anchor's radiance
    assert np.max(np.abs(got[inner] - truth[inner])) < 1e-13
    plain = U.upsample(frame, g, s, s, flags=0, sigma_normal=0.0, sigma_plane=0.0)
    assert U.gamma_rmse(plain[inner], truth[inner]) > 0.05   # without it the detail is gone


# ---- what it buys on the oracle -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bound", [("three_balls", 1.8), ("two_balls", 2.0)])
def test_the_upsampled_preview_is_closer_to_the_converged_frame_than_the_replicated_one(orc, name, bound):
    """Gamma RMSE against 256 spp (seed 7) of the 40-spp scale-4 preview (seed 1) at 128x72, replicated / upsampled.
    Measured with this model: three_balls 0.0913 / 0.0439 = 2.08, two_balls 0.1039 / 0.0425 = 2.44; the
    bounds sit below them so that the difference to a plain block fill is what is tested, not the seed."""
    w, h, scale = 128, 72, 4
    bundle, cam, _ = getattr(S, name)()
    c = S.camera_for(cam, w, h)
    guides = U.oracle_guides(orc, bundle, c, w, h)
    ref, _ = orc.render(bundle.desc, c, abi.render_params(w, h, 256, max_depth=10, tiles_w=1, tiles_h=1, seed=7))
    preview, _ = orc.render(bundle.desc, c, abi.render_params(w, h, 40, max_depth=10, tiles_w=1, tiles_h=1, seed=1, scale=scale))
    sx, sy, cw, ch = U.preview_grid(w, h, 1, 1, scale)
    assert (sx, sy, cw, ch) == (4, 4, w, h) and np.array_equal(preview, U.replicate(preview, sx, sy, cw, ch))
    up = U.upsample(preview, guides, sx, sy)
    replicated, upsampled = U.gamma_rmse(preview, ref), U.gamma_rmse(up, ref)
    print("%s: replicated %.4f upsampled %.4f ratio %.3f" % (name, replicated, upsampled, replicated / upsampled))
    assert replicated / upsampled >= bound, (replicated, upsampled)
