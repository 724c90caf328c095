"""Jittered preview accumulation on the device (csrc/rt_preview_temporal.hip): k_preview_accumulate
against its numpy model (tests/preview_temporal_model.py) on the caller-made inputs of tests/preview_temporal_inputs.py,
the two identities that tie it to rt_temporal_accumulate_device and rt_upsample_preview_device, the camera shift, the
stateful rt_render_preview_temporal against the composition of the device calls, and the picture quality it buys."""
import ctypes as C
import importlib
import os
import shutil
import tempfile

import numpy as np
import pytest

import preview_temporal_inputs as I
import preview_temporal_model as PT
import scenes_py as S
import temporal_model as T
import upsample_model as U

pytestmark = pytest.mark.gpu
abi = S.abi
F64_PLANES = ("radiance", "moments", "length", "normal", "position")


@pytest.fixture(scope="module")
def pt():
    return importlib.import_module("racer-tracer_amd.preview_temporal")


@pytest.fixture(scope="module")
def pv():
    return importlib.import_module("racer-tracer_amd.preview")


@pytest.fixture(scope="module")
def scene(rt, gpu):
    bundle, _, _ = S.three_balls()
    s = rt.Scene(bundle)
    yield s
    s.close()


def close(got, want):
    """The temporal tests' tolerance: |got - want| <= 1e-10 max(1, |want|), per value."""
    return np.abs(got - want) <= 1e-10 * np.maximum(1.0, np.abs(want))


# ---- plumbing: numpy planes <-> device tensors ----------------------------------------------------------------------

def _up(planes, dev):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in planes.items()}


def _down(planes):
    return {k: v.cpu().numpy() for k, v in planes.items()}


def _blank_history(h, w, dev):
    """NaN in every plane (and an id no scene has): whatever the call does not write shows."""
    import torch
    nan = float("nan")
    t = {k: torch.full((h, w, n), nan, dtype=torch.float64, device=dev) for k, n in (("radiance", 3), ("moments", 2), ("normal", 3), ("position", 3))}
    t["length"] = torch.full((h, w), nan, dtype=torch.float64, device=dev)
    t["obj_id"] = torch.full((h, w), -5, dtype=torch.int32, device=dev)
    return t


def _blank_guides(h, w, dev):
    import torch
    g = {k: torch.full((h, w, 3), float("nan"), dtype=torch.float64, device=dev) for k in ("normal", "position", "albedo")}
    g["footprint"] = torch.full((h, w), float("nan"), dtype=torch.float64, device=dev)
    g["obj_id"] = torch.full((h, w), -5, dtype=torch.int32, device=dev)
    return g


def _accumulate(rt, pt, scene, params, jx, jy, rgb, guides, prev=None, prev_cam=None, tp=None, dp=None):
    """rt_preview_accumulate_device on torch copies -> the out history as numpy planes."""
    import torch
    dev = torch.device("cuda", scene.device)
    g, src = _up(guides, dev), _up({"rgb": rgb}, dev)["rgb"]
    pp = _up(prev, dev) if prev is not None else None
    out = _blank_history(params.height, params.width, dev)
    torch.cuda.synchronize(dev)
    pt.accumulate_device(scene, params, jx, jy, src.data_ptr(), rt.guides_struct(g), rt.history_struct(out), prev_cam,
                         rt.history_struct(pp) if pp is not None else None, tp, dp)
    torch.cuda.synchronize(dev)
    return _down(out)


def _resolve(rt, scene, full_params, hist, guides, dp, tp=None):
    """rt_denoise_history_device on torch copies -> numpy."""
    import torch
    dev = torch.device("cuda", scene.device)
    g, hp = _up(guides, dev), _up(hist, dev)
    out = torch.full((full_params.height, full_params.width, 3), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    scene.denoise_history_device(full_params, rt.history_struct(hp), rt.guides_struct(g), out.data_ptr(), dp, tp)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


def _params(shape, spp=1, **kw):
    w, h, tw, th, scale = shape
    return abi.render_params(w, h, spp, tiles_w=tw, tiles_h=th, scale=scale, **kw)


# ---- the kernel against the model -----------------------------------------------------------------------------------

@pytest.mark.parametrize("with_prev", [True, False], ids=["history", "first-frame"])
@pytest.mark.parametrize("demod", [1, 0], ids=["demod", "plain"])
@pytest.mark.parametrize("case", I.CASES, ids=lambda c: "%dx%d" % c[0][:2])
def test_the_kernel_matches_the_model_on_caller_made_inputs(rt, pt, pv, scene, case, demod, with_prev):
    shape, steps, phases = case
    made = I.make(shape)
    params = _params(shape)
    assert pv.preview_grid(params)[:2] == steps == made["steps"]
    sx, sy = steps
    dp, tp = rt.denoise_params(flags=demod), rt.temporal_params()
    prev, cam_prev = (made["prev"], made["cam_prev"]) if with_prev else (None, None)
    for jx, jy in phases:
        frame = I.frame_of(made, jx, jy)
        got = _accumulate(rt, pt, scene, params, jx, jy, frame, made["guides"], prev, cam_prev, tp, dp)
        want, info = PT.accumulate(frame, made["guides"], prev, T.camera_vectors(cam_prev) if with_prev else None, sx, sy, jx, jy,
                                   flags=demod, sigma_normal=dp.sigma_normal, sigma_plane=dp.sigma_plane, **T.temporal_kwargs(tp))
        keep = info["margin"] >= 1e-9
        assert np.mean(~keep) <= 0.005
        worst = 0.0
        for k in F64_PLANES:
            assert np.all(np.isfinite(got[k])), k
            err = np.abs(got[k] - want[k]) / np.maximum(1.0, np.abs(want[k]))
            worst = max(worst, float(err.reshape(err.shape[0], err.shape[1], -1).max(axis=-1)[keep].max()))
            bad = ~close(got[k], want[k])
            bad = bad.reshape(bad.shape[0], bad.shape[1], -1).any(axis=-1) & keep
            assert not bad.any(), "%s phase (%d, %d): %s differs on %d pixels, first at %s" % (shape, jx, jy, k, bad.sum(), np.argwhere(bad)[0])
        print("%s phase (%d, %d) demod %d prev %d: worst error %.3g; %d fresh, %d blended, %d carried, %d filled"
              % (shape, jx, jy, demod, with_prev, worst, info["fresh"].sum(), (info["sampled"] & ~info["fresh"]).sum(),
                 info["carried"].sum(), info["fill"].sum()))
        assert np.array_equal(got["obj_id"], made["guides"]["obj_id"])
        for k in ("normal", "position"):
            assert np.array_equal(got[k], made["guides"][k]), k
        # fresh pixels, carried lengths and the 0.0 of fills: bit for bit.  (A carried length is sum(w L) / sum(w), which
        # the kernel forms without fused multiply-adds; where blocks exist the inputs give every tap the one length
        # I.CARRIED_LENGTH, so the quotient is that length itself whatever the weights' last bits: preview_temporal_inputs.)
        fresh, carried, fill = info["fresh"] & keep, info["carried"] & keep, info["fill"] & keep
        C_ = T.demodulate(frame, made["guides"], demod)
        assert np.array_equal(got["radiance"][fresh], C_[fresh]) and np.all(got["length"][fresh] == 1.0)
        assert np.array_equal(got["length"][carried], want["length"][carried])
        if with_prev and sx * sy > 1:
            assert carried.any() and np.all(got["length"][carried] == I.CARRIED_LENGTH[shape[:2]])
        else:
            assert not info["carried"].any()   # a first frame, or steps of 1: every pixel is sampled
        assert np.all(got["length"][fill] == 0.0) and not np.signbit(got["length"][fill]).any()
        assert np.array_equal(info["fill"] | ~keep, (got["length"] == 0.0) | ~keep)
        if not with_prev:
            assert not info["carried"].any() and np.array_equal(info["fill"], ~info["sampled"])


# ---- identity (b): steps of one are rt_temporal_accumulate_device ---------------------------------------------------

@pytest.mark.parametrize("demod", [1, 0], ids=["demod", "plain"])
def test_with_steps_of_one_the_history_is_rt_temporal_accumulate_devices_bit_for_bit(rt, pt, pv, scene, demod):
    shape = (13, 7, 1, 1, 4)
    made = I.make(shape)
    params = _params(shape)
    assert pv.preview_grid(params)[:2] == (1, 1)
    full = abi.render_params(13, 7, 1)
    dp = rt.denoise_params(flags=demod)
    live = dict(made["prev"], length=np.maximum(made["prev"]["length"], 1.0))   # 4.11 has no condition on a tap's length
    for tp in (rt.temporal_params(), rt.temporal_params(alpha=0.0, alpha_moments=0.0, max_history=2.0)):
        for prev, cam_prev in ((live, made["cam_prev"]), (None, None)):
            got = _accumulate(rt, pt, scene, params, 0, 0, made["full"], made["guides"], prev, cam_prev, tp, dp)
            import torch
            dev = torch.device("cuda", scene.device)
            g, src = _up(made["guides"], dev), _up({"rgb": made["full"]}, dev)["rgb"]
            pp = _up(prev, dev) if prev is not None else None
            out = _blank_history(7, 13, dev)
            torch.cuda.synchronize(dev)
            scene.temporal_accumulate_device(full, src.data_ptr(), rt.guides_struct(g), rt.history_struct(out), cam_prev,
                                             rt.history_struct(pp) if pp is not None else None, tp, dp)
            torch.cuda.synchronize(dev)
            want = _down(out)
            for k in F64_PLANES:
                differ = got[k] != want[k]
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel = np.max(np.where(differ, np.abs(got[k] - want[k]) / np.abs(want[k]), 0.0))
                print("13x7 demod %d history %d %s: %d of %d values differ, worst relative difference %.3g"
                      % (demod, prev is not None, k, differ.sum(), differ.size, rel))
            for k in T.PLANES:
                assert np.array_equal(got[k], want[k]), (k, prev is not None)
            if prev is not None:
                assert (want["length"] > 1.0).any() and (want["length"] == 1.0).any()


# ---- identity (a): phase (0, 0) without a history resolves to rt_upsample_preview_device's frame --------------------

@pytest.mark.parametrize("demod", [1, 0], ids=["demod", "plain"])
@pytest.mark.parametrize("shape", [(103, 47, 10, 5, 4), (33, 17, 1, 1, 16), (8, 6, 1, 1, 2)], ids=lambda s: "%dx%d" % s[:2])
def test_phase_zero_without_a_history_resolves_to_the_upsampled_preview(rt, pt, pv, scene, shape, demod):
    """On all pixels, at 1e-12 relative.  With demodulation the albedo is kept off the clamp (a pixel none
    of whose anchors qualifies is stored demodulated, which gives its input back only where the clamp does not bite)."""
    import torch
    w, h, tw, th, scale = shape
    g, rng = U.synthetic_guides(h, w, seed=100 * w + h)
    if demod:
        g = dict(g, albedo=np.maximum(g["albedo"], 0.05))
    sx, sy, cw, ch = U.preview_grid(w, h, tw, th, scale)
    frame = U.replicate(U.synthetic_frame(g, rng), sx, sy, cw, ch)
    params, full = _params(shape), abi.render_params(w, h, 1, tiles_w=tw, tiles_h=th)
    dp = rt.denoise_params(iterations=0, flags=demod)
    hist = _accumulate(rt, pt, scene, params, 0, 0, frame, g, dp=dp)
    got = _resolve(rt, scene, full, hist, g, dp)
    dev = torch.device("cuda", scene.device)
    planes = _up(dict(g, rgb=frame), dev)
    out = torch.full_like(planes["rgb"], float("nan"))
    torch.cuda.synchronize(dev)
    pv.upsample_preview_device(scene, params, planes["rgb"].data_ptr(), rt.guides_struct(planes), out.data_ptr(), dp)
    torch.cuda.synchronize(dev)
    want = out.cpu().numpy()
    assert np.all(np.isfinite(got)) and U.mismatch(got, want, 1e-12) == 0
    assert (hist["length"] == 0.0).sum() == w * h - (w // sx) * (h // sy)


# ---- the shift is right ---------------------------------------------------------------------------------------------

def test_the_phase_cameras_guides_are_the_callers_guides_shifted_by_the_phase(rt, pt, scene):
    w, h, jx, jy = 100, 45, 3, 2
    _, cam, _ = S.three_balls()
    camera = S.camera_for(cam, w, h)
    params = abi.render_params(w, h, 1, tiles_w=1, tiles_h=1, scale=4)   # steps 4x3
    full = abi.render_params(w, h, 1, tiles_w=1, tiles_h=1)
    shifted = pt.phase_camera(camera, params, jx, jy)
    a, b = scene.render_guides(shifted, full), scene.render_guides(camera, full)
    assert np.array_equal(a["obj_id"][:h - jy, :w - jx], b["obj_id"][jy:, jx:])
    assert (b["obj_id"] >= 0).any() and (b["obj_id"] < 0).any()
    assert not np.array_equal(a["obj_id"], b["obj_id"])
    for k in ("position", "normal"):
        x, y = a[k][:h - jy, :w - jx], b[k][jy:, jx:]
        assert np.all(np.abs(x - y) <= 1e-10 * np.maximum(1.0, np.abs(y))), k


# ---- the stateful form ----------------------------------------------------------------------------------------------

class Composer:
    """What rt_render_preview_temporal and rt_render_temporal do per frame, with the device calls, on torch buffers."""

    def __init__(self, rt, pt, scene, w, h):
        import torch
        self.rt, self.pt, self.scene = rt, pt, scene
        self.dev = torch.device("cuda", scene.device)
        self.frame = torch.zeros((h, w, 3), dtype=torch.float64, device=self.dev)
        self.out = torch.zeros_like(self.frame)
        self.guides = _blank_guides(h, w, self.dev)
        self.hist = [_blank_history(h, w, self.dev), _blank_history(h, w, self.dev)]
        self.g = rt.guides_struct(self.guides)
        self.n, self.prev_cam = 0, None

    def _finish(self, full, cur, camera, tp, dp):
        import torch
        self.scene.denoise_history_device(full, self.rt.history_struct(cur), self.g, self.out.data_ptr(), dp, tp)
        torch.cuda.synchronize(self.dev)
        self.n, self.prev_cam = self.n + 1, camera
        return self.out.cpu().numpy(), cur["length"].cpu().numpy()

    def _guides(self, camera, full):
        self.rt.check(self.scene._lib.rt_render_guides_device(self.scene._h, C.byref(camera), C.byref(full), C.byref(self.g), None),
                      "rt_render_guides_device", self.scene._lib)

    def preview(self, camera, params, full, frame_index, tp, dp):
        rt, pt = self.rt, self.pt
        cur, old = self.hist[self.n & 1], self.hist[(self.n & 1) ^ 1]
        jx, jy = pt.phase(params, frame_index)
        self.scene.render_frame_device(pt.phase_camera(camera, params, jx, jy), params, self.frame.data_ptr())
        stats = None
        self._guides(camera, full)
        pt.accumulate_device(self.scene, params, jx, jy, self.frame.data_ptr(), self.g, rt.history_struct(cur), self.prev_cam,
                             rt.history_struct(old) if self.prev_cam is not None else None, tp, dp)
        out = self._finish(full, cur, camera, tp, dp)
        stats = self.scene.last_stats()
        return out + ((stats.samples, stats.segments),)

    def plain(self, camera, full, tp, dp):
        rt = self.rt
        cur, old = self.hist[self.n & 1], self.hist[(self.n & 1) ^ 1]
        self.scene.render_frame_device(camera, full, self.frame.data_ptr())
        self._guides(camera, full)
        self.scene.temporal_accumulate_device(full, self.frame.data_ptr(), self.g, rt.history_struct(cur), self.prev_cam,
                                              rt.history_struct(old) if self.prev_cam is not None else None, tp, dp)
        return self._finish(full, cur, camera, tp, dp)

    def reset(self):
        self.prev_cam = None


W, H, SPP = 100, 45, 5


def _frame_params(k):
    return (abi.render_params(W, H, SPP, max_depth=10, tiles_w=10, tiles_h=5, seed=31 + k, scale=4),
            abi.render_params(W, H, SPP, max_depth=10, tiles_w=10, tiles_h=5, seed=31 + k))


@pytest.mark.parametrize("levels", [0, 2])
def test_render_preview_temporal_is_the_composition_of_the_device_calls(rt, pt, pv, scene, levels):
    _, cam, _ = S.three_balls()
    tp, dp = rt.temporal_params(), rt.denoise_params(iterations=levels)
    assert pv.preview_grid(_frame_params(0)[0])[:2] == (2, 3)
    cameras = [S.camera_for(T.orbit(cam, 0.5 * k), W, H) for k in range(12)]   # two cycles of six frames
    comp = Composer(rt, pt, scene, W, H)
    t = rt.Temporal(W, H, device=scene.device)
    try:
        lengths = []
        for k in range(12):
            p, full = _frame_params(k)
            want, want_len, want_stats = comp.preview(cameras[k], p, full, k, tp, dp)
            got, got_len = pt.render_preview_temporal(scene, t, cameras[k], p, k, tp, dp, with_length=True)
            stats = scene.last_stats()
            assert np.array_equal(got, want), k
            assert np.array_equal(got_len, want_len), k
            assert (stats.samples, stats.segments) == want_stats and stats.samples == (W // 2) * (H // 3) * SPP, k
            lengths.append(got_len)
        assert (lengths[0] == 0.0).sum() == W * H - (W // 2) * (H // 3)
        assert (lengths[-1] == 0.0).sum() < (lengths[0] == 0.0).sum() and lengths[-1].max() > 1.5
        # after a reset the next frame is a first frame
        t.reset()
        comp.reset()
        p, full = _frame_params(0)
        want, want_len, _ = comp.preview(cameras[0], p, full, 0, tp, dp)
        got, got_len = pt.render_preview_temporal(scene, t, cameras[0], p, 0, tp, dp, with_length=True)
        assert np.array_equal(got, want) and np.array_equal(got_len, want_len) and np.array_equal(got_len, lengths[0])
    finally:
        t.close()


def test_preview_and_full_resolution_frames_alternate_on_one_state(rt, pt, scene):
    """Moving (preview frames), still (rt_render_temporal), moving again: one history, no reset."""
    _, cam, _ = S.three_balls()
    tp, dp = rt.temporal_params(), rt.denoise_params(iterations=1)
    kinds = ["preview", "preview", "preview", "plain", "plain", "preview", "plain", "preview"]
    cameras = [S.camera_for(T.orbit(cam, 0.5 * min(k, 3)), W, H) for k in range(len(kinds))]
    comp = Composer(rt, pt, scene, W, H)
    t = rt.Temporal(W, H, device=scene.device)
    try:
        for k, kind in enumerate(kinds):
            p, full = _frame_params(k)
            if kind == "preview":
                want, want_len, _ = comp.preview(cameras[k], p, full, k, tp, dp)
                got, got_len = pt.render_preview_temporal(scene, t, cameras[k], p, k, tp, dp, with_length=True)
            else:
                want, want_len = comp.plain(cameras[k], full, tp, dp)
                got, got_len = t.render(scene, cameras[k], full, tp, dp, with_length=True)
                assert (got_len >= 1.0).all()
            assert np.array_equal(got, want), (k, kind)
            assert np.array_equal(got_len, want_len), (k, kind)
        assert got_len.max() > 3.0   # the history lived through the switches
    finally:
        t.close()


def test_refusals_with_a_state_and_a_scene(rt, pt, scene):
    _, cam, _ = S.three_balls()
    camera = S.camera_for(cam, W, H)
    p, full = _frame_params(0)
    t = rt.Temporal(W, H, device=scene.device)
    bundle, _, _ = S.three_balls()
    v1 = rt.Scene(bundle, kernel=abi.RT_KERNEL_V1)
    try:
        for bad in (abi.render_params(W + 2, H, SPP, tiles_w=1, tiles_h=1, scale=2), abi.render_params(W, H + 3, SPP, tiles_w=1, tiles_h=1, scale=3)):
            with pytest.raises(rt.RtError, match="RtTemporal") as e:
                pt.render_preview_temporal(scene, t, camera, bad, 0)
            assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
        with pytest.raises(rt.RtError, match="scale") as e:
            pt.render_preview_temporal(scene, t, camera, full, 0)
        assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
        with pytest.raises(rt.RtError, match="v1") as e:
            pt.render_preview_temporal(v1, t, camera, p, 0)
        assert e.value.code == abi.RT_ERR_UNSUPPORTED
        # none of the refusals left a history behind
        _, length = pt.render_preview_temporal(scene, t, camera, p, 0, with_length=True)
        assert (length == 0.0).sum() == W * H - (W // 2) * (H // 3) and np.all(length[0:45:3, 0:100:2] == 1.0)
    finally:
        v1.close()
        t.close()


def test_a_scene_of_another_loaded_library_is_served_by_that_library(rt, pt, scene):
    _, cam, _ = S.three_balls()
    camera = S.camera_for(cam, W, H)
    t = rt.Temporal(W, H, device=scene.device)
    try:
        want = [pt.render_preview_temporal(scene, t, camera, _frame_params(k)[0], k) for k in range(3)]
    finally:
        t.close()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "libracer_tracer_amd_second.so")
        shutil.copyfile(rt.LIB_PATH, path)
        second = rt.load_library(path)
        assert not any(b is second for b in pt._bound)
        bundle, _, _ = S.three_balls()
        other = rt.Scene(bundle, library=second)
        state = rt.Temporal(W, H, device=other.device, library=second)
        try:
            for k in range(3):
                assert np.array_equal(pt.render_preview_temporal(other, state, camera, _frame_params(k)[0], k), want[k]), k
            assert any(b is second for b in pt._bound)
            with pytest.raises(rt.RtError, match="no preview to upsample"):
                pt.render_preview_temporal(other, state, camera, _frame_params(0)[1], 0)
            assert b"no preview to upsample" in second.rt_last_error_message()
        finally:
            state.close()
            other.close()


# ---- it helps where it should ---------------------------------------------------------------------------------------

def test_two_cycles_of_a_still_camera_beat_the_upsampled_last_frame(rt, pt, pv, scene):
    """Still camera, three_balls 128x72, tiles 1x1, scale 4 (blocks of 4x4), 4 spp, 32 frames at seeds 1..32, alpha 0 (a
    still camera's setting: the mean of a pixel's samples), no levels on either side.  Gamma RMSE against a 1024-spp full
    frame."""
    w, h, spp = 128, 72, 4
    _, cam, _ = S.three_balls()
    camera = S.camera_for(cam, w, h)
    tp, dp = rt.temporal_params(alpha=0.0, alpha_moments=0.0, max_history=1e9), rt.denoise_params(iterations=0)
    t = rt.Temporal(w, h, device=scene.device)
    try:
        for k in range(32):
            p = abi.render_params(w, h, spp, max_depth=10, tiles_w=1, tiles_h=1, seed=1 + k, scale=4)
            got, length = pt.render_preview_temporal(scene, t, camera, p, k, tp, dp, with_length=True)
    finally:
        t.close()
    alone = pv.render_preview_upsampled(scene, camera, p, dp)
    truth = scene.render_frame(camera, abi.render_params(w, h, 1024, max_depth=10, tiles_w=1, tiles_h=1, seed=99))
    e_t, e_a = U.gamma_rmse(got, truth), U.gamma_rmse(alone, truth)
    print("gamma RMSE against 1024 spp: 32 accumulated preview frames %.5f, rt_render_preview_upsampled on the last frame %.5f; "
          "mean history length %.2f" % (e_t, e_a, length.mean()))
    assert e_t < e_a


# ---- CLI ------------------------------------------------------------------------------------------------------------

def test_cli_preview_temporal_writes_a_png_and_reports_the_history(rt, gpu):
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "racer-tracer_amd", "bin", "racer-tracer-amd")
    config, scene_yml = os.path.join(root, "scenes", "config_c1.yml"), os.path.join(root, "scenes", "three_balls.yml")
    with tempfile.TemporaryDirectory(prefix="rt_cli_preview_temporal_") as out:
        r = subprocess.run([exe, "-c", config, "-s", scene_yml, "--image-action", "png", "--seed", "1", "--preview-temporal", "3"],
                           capture_output=True, text=True, cwd=out, timeout=120)
        assert r.returncode == 0, r.stderr
        path = re.search(r"Saved image to: (.+)", r.stderr).group(1).strip()
        path = path if os.path.isabs(path) else os.path.join(out, path)
        assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
        m = re.search(r"mean history length ([0-9]+\.[0-9]+), ([0-9]+\.[0-9]+) % of the pixels with length 0", r.stderr)
        assert m and 0.0 < float(m.group(1)) and 0.0 < float(m.group(2)) < 100.0, r.stderr
        for bad in (["--preview-temporal", "0"], ["--preview-temporal", "2", "--nee"], ["--preview-temporal", "2", "--temporal", "2"]):
            r = subprocess.run([exe, "-c", config, "-s", scene_yml] + bad, capture_output=True, text=True, cwd=out, timeout=60)
            assert r.returncode != 0 and "--preview-temporal" in r.stderr
