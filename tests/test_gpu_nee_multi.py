"""Next-event-estimation frames over several shares (include/rt_abi.h): rt_render_frame_nee_multi,
rt_render_frame_nee_multi_device, rt_render_nee_multi and rt_render_frame_nee_strips_device.  Every test runs on ONE card:
the shares are several scenes of the same description on device 0.  The oracle of every pixel is rt_render_frame_nee on
the same card — itself held to tests/nee_model.py by tests/test_gpu_nee.py — and the comparison is np.array_equal
throughout: sums are per pixel, in f64, in sample order, and every draw is addressed by the pixel's index in the whole
image, so neither the number of shares nor the strip height may change a bit.  No test asserts a time."""
import hashlib
import os
import re
import subprocess
import tempfile
import threading

import numpy as np
import pytest

import nee_variant_frames as NVF
import scenes_py as S
import variant_scenes as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 75, 37, 12   # neither size a multiple of 8: the last strip hangs over the image


def _params(abi, w=W, h=H, spp=SPP, tiles=(10, 10), depth=10, seed=5):
    p = abi.render_params(w, h, spp, max_depth=depth, tiles_w=tiles[0], tiles_h=tiles[1])
    p.seed = seed
    return p


@pytest.fixture(scope="module")
def cornell(rt, abi, gpu):
    """Four scenes of cornell_box on device 0, three more with the staged gather, and the one-shot frame of the ragged
    shape (read-only) with its segment count."""
    bundle, cam, _ = S.cornell_box()
    scenes = [rt.Scene(bundle) for _ in range(4)]
    staged = [rt.Scene(bundle, gather=abi.RT_GATHER_STAGED) for _ in range(3)]
    camera = S.camera_for(cam, W, H)
    want = scenes[0].render_frame_nee(camera, _params(abi))
    want.setflags(write=False)
    segments = int(scenes[0].last_stats().segments)
    yield dict(scenes=scenes, staged=staged, cam=cam, camera=camera, want=want, segments=segments)
    for s in scenes + staged:
        s.close()


def _owned_rows(h, strip_rows, n, i):
    return [r for r in range(h) if n == 1 or (r // strip_rows) % n == i]


# ---- 1. whole frames, ragged shape ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("strip_rows", [0, 16, 5, 12])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_whole_frames_over_shares(rt, abi, cornell, n, strip_rows):
    scenes, p = cornell["scenes"][:n], _params(abi)
    got = rt.render_frame_nee_multi(scenes, cornell["camera"], p, strip_rows)
    assert np.array_equal(got, cornell["want"])
    stats = [s.last_stats() for s in scenes]
    assert sum(int(st.samples) for st in stats) == W * H * SPP
    assert sum(int(st.segments) for st in stats) == cornell["segments"]
    for i, st in enumerate(stats):  # a share counts its own rows
        assert st.samples == len(_owned_rows(H, strip_rows or 8, n, i)) * W * SPP
        assert st.kernel_launches == 1


# ---- 2. the strips entry point ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strip_rows", [8, 5])
def test_strips_into_one_device_buffer(rt, abi, cornell, strip_rows):
    import torch
    dev = torch.device("cuda", 0)
    out = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev)
    want = cornell["want"]
    with torch.cuda.stream(stream):
        for i in range(3):
            p = _params(abi)
            p.strip_rows, p.strip_count, p.strip_index = strip_rows, 3, i
            cornell["scenes"][i].render_frame_nee_strips_device(cornell["camera"], p, out.data_ptr(), stream=stream.cuda_stream)
            if i == 0:
                stream.synchronize()
                first = out.cpu().numpy()
                mine = _owned_rows(H, strip_rows, 3, 0)
                others = [r for r in range(H) if r not in mine]
                assert np.array_equal(first[mine], want[mine])
                assert not first[others].any()  # rows not owned are not written
                st = cornell["scenes"][0].last_stats()
                assert st.samples == len(mine) * W * SPP and st.kernel_launches == 1
    stream.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    # strip_count <= 1: rt_render_frame_nee_device
    out.zero_()
    with torch.cuda.stream(stream):
        cornell["scenes"][0].render_frame_nee_strips_device(cornell["camera"], _params(abi), out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def test_a_strip_index_below_the_image_writes_nothing(rt, abi, cornell):
    import torch
    dev = torch.device("cuda", 0)
    out = torch.full((H, W, 3), -1.0, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev)
    p = _params(abi)
    p.strip_rows, p.strip_count, p.strip_index = 16, 4, 3  # its first strip starts at row 48 of 37
    with torch.cuda.stream(stream):
        cornell["scenes"][1].render_frame_nee_strips_device(cornell["camera"], p, out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert (out.cpu().numpy() == -1.0).all()
    st = cornell["scenes"][1].last_stats()
    assert st.samples == 0 and st.segments == 0 and st.kernel_launches == 0


# ---- 3. the device gather ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strip_rows", [0, 12])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("gather", ["default", "staged"])
def test_device_gather(rt, abi, cornell, gather, n, strip_rows):
    import torch
    scenes = cornell["scenes" if gather == "default" else "staged"][:n]
    out = torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rt.render_frame_nee_multi_device(scenes, cornell["camera"], _params(abi), out.data_ptr(), strip_rows)
    assert np.array_equal(out.cpu().numpy(), cornell["want"])
    stats = [s.last_stats() for s in scenes]
    assert sum(int(st.samples) for st in stats) == W * H * SPP
    assert sum(int(st.segments) for st in stats) == cornell["segments"]


# ---- 4. the tile stream ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("tiles", [(7, 3), (1, 1), (4, 5)], ids=lambda t: "%dx%d" % t)
def test_tile_stream_over_shares(rt, abi, cornell, tiles, n):
    scenes, p = cornell["scenes"][:n], _params(abi, tiles=tiles)
    _, want_order = cornell["scenes"][3].render_tiles_nee(cornell["camera"], p)
    seen = []
    frame, order = rt.render_tiles_nee_multi(scenes, cornell["camera"], p, strip_rows=(0, 5, 12)[n - 1],
                                             on_tile=lambda *t: seen.append(t))
    assert order == want_order and len(order) == tiles[0] * tiles[1] and seen == order
    for r, c, w, h in order:  # every tile's pixels are the frame's
        assert np.array_equal(frame[r:r + h, c:c + w], cornell["want"][r:r + h, c:c + w])
    assert np.array_equal(frame, cornell["want"])
    stats = [s.last_stats() for s in scenes]
    assert sum(int(st.samples) for st in stats) == W * H * SPP
    assert sum(int(st.segments) for st in stats) == cornell["segments"]
    assert all(st.kernel_launches == 1 for st in stats)


def test_a_grid_wider_than_the_image(rt, abi, cornell):
    """No delivering launch: one scene falls back as rt_render_nee does, several are refused as rt_render_multi refuses."""
    p = _params(abi, tiles=(80, 2))
    frame, order = rt.render_tiles_nee_multi(cornell["scenes"][:1], cornell["camera"], p)
    assert order == cornell["scenes"][3].render_tiles_nee(cornell["camera"], p)[1] and np.array_equal(frame, cornell["want"])
    with pytest.raises(rt.RtError) as e:
        rt.render_tiles_nee_multi(cornell["scenes"][:2], cornell["camera"], p)
    assert e.value.code == abi.RT_ERR_UNSUPPORTED


# ---- 5. shares that own nothing ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 4])
def test_shares_that_own_nothing(rt, abi, cornell, n):
    w, h, spp = 64, 16, 12   # two strips of 8 rows: shares 2 and 3 own none
    camera, p = S.camera_for(cornell["cam"], w, h), _params(abi, w, h, spp, tiles=(4, 2))
    want = cornell["scenes"][3].render_frame_nee(camera, p)
    want_order = cornell["scenes"][3].render_tiles_nee(camera, p)[1]
    scenes = cornell["scenes"][:n]

    def check_stats():
        stats = [s.last_stats() for s in scenes]
        assert [int(st.samples) for st in stats[:2]] == [w * 8 * spp] * 2
        assert [st.kernel_launches for st in stats[:2]] == [1, 1]
        for st in stats[2:]:
            assert st.kernel_launches == 0 and st.samples == 0 and st.segments == 0

    assert np.array_equal(rt.render_frame_nee_multi(scenes, camera, p), want)
    check_stats()
    frame, order = rt.render_tiles_nee_multi(scenes, camera, p)
    assert np.array_equal(frame, want) and order == want_order
    check_stats()


# ---- 6. every compiled variant, both flavours ----------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", ["fast", "exact"])
@pytest.mark.parametrize("form", sorted(V.SPECS), ids=lambda f: "p%d-t%d-s%d-b%d" % f)
def test_every_variant_over_two_shares(rt, abi, gpu, form, flavour):
    bundle, camera = NVF.case(abi, form)
    p = NVF.params(abi, V.DEPTH)
    options = dict(closest_hit=abi.RT_HIT_BVH if form[3] else abi.RT_HIT_LINEAR,
                   arithmetic=abi.RT_ARITH_REFERENCE if flavour == "exact" else abi.RT_ARITH_FAST)
    scenes = [rt.Scene(bundle, **options) for _ in range(2)]
    try:
        for s in scenes:
            v = s.variant()
            assert (v["prims_class"], v["textured"], v["specular"], v["use_bvh"]) == form and v["exact"] == (flavour == "exact")
        want = scenes[0].render_frame_nee(camera, p)
        segments = int(scenes[0].last_stats().segments)
        assert np.array_equal(rt.render_frame_nee_multi(scenes, camera, p, 8), want)
        assert sum(int(s.last_stats().segments) for s in scenes) == segments
        p.tiles_w, p.tiles_h = 3, 2
        frame, order = rt.render_tiles_nee_multi(scenes, camera, p, 5)
        assert len(order) == 6 and np.array_equal(frame, want)
        assert sum(int(s.last_stats().segments) for s in scenes) == segments
    finally:
        for s in scenes:
            s.close()


# ---- 7. RT_KERNEL_V1 scenes ------------------------------------------------------------------------------------------------------

def test_v1_scenes_render_through_both_host_forms(rt, abi, cornell):
    bundle, _, _ = S.cornell_box()
    scenes = [rt.Scene(bundle, kernel=abi.RT_KERNEL_V1) for _ in range(2)]
    try:
        assert all(s.variant()["kernel"] == 1 for s in scenes)
        p = _params(abi, tiles=(4, 5))
        assert np.array_equal(rt.render_frame_nee_multi(scenes, cornell["camera"], p), cornell["want"])
        frame, order = rt.render_tiles_nee_multi(scenes, cornell["camera"], p, 5)
        assert len(order) == 20 and np.array_equal(frame, cornell["want"])
    finally:
        for s in scenes:
            s.close()


# ---- 8. cancel -----------------------------------------------------------------------------------------------------------------------

def test_cancel_ends_every_share(rt, abi, cornell):
    """1920x1080 at 4096 spp over two shares is more than a second of work (profiles/nee_timings.json: 322 ms at 1024 spp);
    the hook rises after 50 ms.  RT_OK, fewer than all tiles, both launches ended long before their work was done, and the
    same scenes then render as fresh ones."""
    w, h, n = 1920, 1080, 4096
    scenes = cornell["scenes"][:2]
    camera, p = S.camera_for(cornell["cam"], w, h), _params(abi, w, h, n)
    # one sample per pixel first: the pinned 1080p frame and the counters are allocated, so the 50 ms fall into the render
    rt.render_tiles_nee_multi(scenes, camera, _params(abi, w, h, 1), cancel=lambda: False)
    up = threading.Event()
    timer = threading.Timer(0.05, up.set)
    timer.start()
    try:
        _, order = rt.render_tiles_nee_multi(scenes, camera, p, cancel=up.is_set)
    finally:
        timer.cancel()
    started = sum(int(s.last_stats().samples) for s in scenes)
    print("cancelled after %d of 100 tiles; %.2f %% of the primary rays were started" % (len(order), 100.0 * started / (w * h * n)))
    assert len(order) < 100
    assert started < w * h * n // 2
    small = _params(abi, tiles=(7, 3))
    frame, order = rt.render_tiles_nee_multi(scenes, cornell["camera"], small, 5)
    assert len(order) == 21 and np.array_equal(frame, cornell["want"])
    assert np.array_equal(rt.render_frame_nee_multi(scenes, cornell["camera"], small), cornell["want"])
    for s in scenes:
        assert np.array_equal(s.render_frame_nee(cornell["camera"], small), cornell["want"])


def test_cancel_on_entry_and_a_repeated_scene(rt, abi, cornell):
    scenes, p = cornell["scenes"][:2], _params(abi)
    seen = []
    with pytest.raises(rt.RtError) as e:
        rt.render_tiles_nee_multi(scenes, cornell["camera"], p, cancel=lambda: True, on_tile=lambda *t: seen.append(t))
    assert e.value.code == abi.RT_ERR_CANCEL_EVENT and not seen
    for call in (lambda twice: rt.render_tiles_nee_multi(twice, cornell["camera"], p),
                 lambda twice: rt.render_frame_nee_multi(twice, cornell["camera"], p)):
        with pytest.raises(rt.RtError) as e:
            call([scenes[0], scenes[0]])
        assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
    assert np.array_equal(rt.render_tiles_nee_multi(scenes, cornell["camera"], p)[0], cornell["want"])


# ---- 9. the CLI ------------------------------------------------------------------------------------------------------------------------

def test_cli_nee_devices_writes_the_bytes_of_nee(rt, gpu):
    exe = os.path.join(ROOT, "racer-tracer_amd", "bin", "racer-tracer-amd")
    config, scene_yml = os.path.join(ROOT, "scenes", "config_c1.yml"), os.path.join(ROOT, "scenes", "cornell_box.yml")
    digests = {}
    for flags in (("--nee",), ("--nee-devices", "1")):
        out = tempfile.mkdtemp(prefix="rt_cli_nee_devices_")
        r = subprocess.run([exe, "-c", config, "-s", scene_yml, "--image-action", "png", "--seed", "1"] + list(flags),
                           capture_output=True, text=True, cwd=out, timeout=600)
        assert r.returncode == 0, r.stderr
        m = re.search(r"Saved image to: (.+)", r.stderr)
        assert m, r.stderr
        path = m.group(1).strip()
        path = path if os.path.isabs(path) else os.path.join(out, path)
        digests[flags[0]] = hashlib.sha256(open(path, "rb").read()).hexdigest()
    assert digests["--nee"] == digests["--nee-devices"]
