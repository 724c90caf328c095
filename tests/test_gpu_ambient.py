"""The ambient-occlusion query (include/rt_ambient.h) on the GPU.  The kernel hands out the rays it walked:
its counts are held, bit for bit and with no ray excused, to rt_trace_occlusion_device on exactly those rays, on every scene
form, both arithmetic flavours, four sample counts and two windows; the rays themselves are held to tests/ambient_model.py;
scenes with a closed form; addressing (halves, chunks, seeds, launch shapes); invalid points; the frame and the CLI flag."""
import importlib
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ambient_model as A
import ray_query_model as Q
import scenes_py as S

pytestmark = pytest.mark.gpu
abi = Q.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = "form-2-0-0-1"      # a tree (staged in LDS by renders) with moving and wrapped primitives
FLAVOURS = {"fast": {}, "exact": dict(arithmetic=abi.RT_ARITH_REFERENCE)}
INVALID = A.INVALID
SENTINEL = -777


@pytest.fixture(scope="module")
def amb():
    return importlib.import_module("racer-tracer_amd.ambient")


@pytest.fixture(scope="module")
def occ():
    return importlib.import_module("racer-tracer_amd.occlusion")


@pytest.fixture(scope="module")
def rays():
    return importlib.import_module("racer-tracer_amd.rays")


@pytest.fixture(scope="module")
def identity_draws(orc):
    """u [256, 256, 3] of the identity tests' seed: sample s of point g draws the same whatever S and n are.  Computed once,
    never written to."""
    seed, base, n, samples = A.IDENTITY
    u = A.draws(orc, seed, base, n, samples)[0]
    u.setflags(write=False)
    return u


def open_scene(rt, bundle, closest_hit=abi.RT_HIT_AUTO, in_lds=None, **options):
    scene = rt.Scene(bundle, closest_hit=closest_hit, **options)
    variant = scene.variant()
    assert variant["use_bvh"] == int(in_lds is not None)
    assert variant["exact"] == int("arithmetic" in options)
    return scene


def up(scene, a):
    import torch
    return None if a is None else torch.tensor(np.asarray(a), dtype=torch.float64, device=torch.device("cuda", scene.device))


def sync(scene):
    import torch
    torch.cuda.synchronize(torch.device("cuda", scene.device))


def first_hits(rays, scene, o, d, time):
    """The device's own closest hits of these rays -> numpy planes t, point, normal, prim."""
    got = rays.trace_rays_torch(scene, up(scene, o), up(scene, d), time=up(scene, time), planes=("t", "point", "normal", "prim"))
    sync(scene)
    return {k: v.cpu().numpy() for k, v in got.items()}


def ambient(amb, scene, points, normals, t_min=None, t_max=None, time=None, **kw):
    """ambient_torch on numpy points -> numpy int32 (and, with export=True, the dict of numpy ray planes)."""
    got = amb.ambient_torch(scene, up(scene, points), up(scene, normals), t_min=up(scene, t_min), t_max=up(scene, t_max),
                            time=up(scene, time), **kw)
    sync(scene)
    if kw.get("export"):
        return got[0].cpu().numpy(), {k: v.cpu().numpy() for k, v in got[1].items()}
    return got.cpu().numpy()


def hit_points(rt, rays, name, n, **options):
    """-> (scene, points, normals, time, hit, t * |d|): the device's closest hits of THE random ray set on scene `name`."""
    bundle, cam, spread, closest_hit, in_lds = Q.scene(name)
    o, d, time = Q.random_rays(cam, n, spread)
    scene = open_scene(rt, bundle, closest_hit, in_lds, **options)
    first = first_hits(rays, scene, o, d, time)
    distance = first["t"] * np.sqrt((d * d).sum(axis=1))
    return scene, first["point"], first["normal"], time, first["prim"] >= 0, distance


# ---- 1, 2: the counts are the occlusion query's on the exported rays; the rays are the model's -----------------------------------

# The fast flavour's directions against the model's (RT_ARITH_REFERENCE's arithmetic), per component.  nhat and unit(u)
# carry at most 4.5 * 2^-53 each on the device (l2: three roundings, halved by the root: 1.5; the reciprocal root: 1 ulp = 2;
# the product: 1) and 3.5 * 2^-53 in the model (1.5; the root: 1; the division: 1): 2^-50 between them, each.  Step 3 adds the
# two and rounds on either side: 2^-49 + 2^-51 in a component of dir.  Step 5 divides by |dir|, which lies anywhere in (0, 2]:
# sqrt(3) * (2^-49 + 2^-51) / |dir| from dir's error, and 2^-50 from the two units' own roundings.  At |dir| = 2 that is
# 0.8 * 2^-48, the eight operations of at most an ulp on values of at most 2; for a sample that grazes the surface it grows
# as 1 / |dir| does.  So: 2^-48 * 2 / |dir| (>= 2^-48), |dir| the model's.
# Measured on the MI355X over this file's 152 fast cases, 1 751 750 rays: 544 rays above a flat 2^-48, all grazing, the worst
# 11.9 x 2^-48; the worst against this bound 0.090 (DESIGN.md 4.18 records both).
def fast_direction_bound(length):
    return 2.0 ** -48 * 2.0 / length


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("name", Q.SCENES)
def test_counts_are_the_occlusion_query_on_the_exported_rays(rt, orc, amb, occ, rays, gpu, identity_draws, name, flavour):
    """No ray excused: open[p] == S - (the occlusion query's 1s among rays p S .. p S + S - 1), the rays being the ones the
    kernel exported — it walked those very values with the occlusion kernel's walk.  The rays of an invalid point (here: a
    ray of the set that missed, point = normal = 0) are invalid to the occlusion query.  Origins, windows and times are the
    inputs' own; the directions are the model's, bit for bit in RT_ARITH_REFERENCE, within fast_direction_bound otherwise."""
    seed = A.IDENTITY[0]
    n = 64 if name == "large_bvh" else 256
    scene, points, normals, time, hit, distance = hit_points(rt, rays, name, n, **FLAVOURS[flavour])
    try:
        assert hit.sum() >= n // 4
        median = float(np.median(distance[hit]))
        seen = set()
        for radius in (math.inf, median):
            for samples in (1, 4, 64, 256):
                counts, walked = ambient(amb, scene, points, normals, time=time, samples=samples, radius=radius, seed=seed, export=True)
                verdict = occ.occluded_torch(scene, *[up(scene, walked[k]) for k in ("origin", "direction", "t_min", "t_max", "time")])
                sync(scene)
                verdict = verdict.cpu().numpy().reshape(n, samples)
                assert counts.dtype == np.int32 and counts.shape == (n,)
                assert np.array_equal(counts != INVALID, hit)
                assert np.isin(verdict[hit], (0, 1)).all() and (verdict[~hit] == INVALID).all()
                want = samples - (verdict == 1).sum(axis=1)
                differ = hit & (counts != want)
                print("%s %s S = %d radius %g: open %d of %d rays, %d points differ from the occlusion query"
                      % (name, flavour, samples, radius, counts[hit].sum(), hit.sum() * samples, differ.sum()))
                assert not differ.any(), (samples, radius, np.nonzero(differ)[0][:8])
                seen.update(np.unique(counts[hit] / samples).tolist())
                # the rays
                model = A.rays(orc, points, normals, samples, radius=radius, time=time, u=identity_draws[:n, :samples])
                assert np.array_equal(model["valid"], hit)
                for plane in ("origin", "t_min", "t_max", "time"):
                    assert np.array_equal(walked[plane], model[plane]), plane
                assert (walked["direction"][~np.repeat(hit, samples)] == 0).all()
                rows = np.repeat(hit, samples)
                err = np.abs(walked["direction"][rows] - model["direction"][rows]).max(axis=1)
                length = model["length"][rows]
                print("    directions: largest |device - model| = %.3g = %.3f x 2^-48; largest over its bound %.3f; %d of %d rays above 2^-48"
                      % (err.max(), err.max() / 2.0 ** -48, (err / fast_direction_bound(length)).max(), (err > 2.0 ** -48).sum(), err.size))
                if flavour == "exact":
                    assert np.array_equal(walked["direction"], model["direction"])
                else:
                    assert (err <= fast_direction_bound(length)).all()
        assert len(seen) > 2      # some hemispheres are partly open: the counts are not all 0 or S
    finally:
        scene.close()


# ---- 3: closed forms ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_closed_forms(rt, amb, gpu, flavour):
    floor, box = A.floor_and_box()
    rng = np.random.default_rng(3)
    n, samples = 256, 64
    # a lone floor, normals up: nothing above it
    scene = open_scene(rt, floor, **FLAVOURS[flavour])
    try:
        on_floor = np.column_stack([rng.uniform(-5, 5, n), np.zeros(n), rng.uniform(-5, 5, n)])
        got = ambient(amb, scene, on_floor, np.tile([0.0, 2.5, 0.0], (n, 1)), samples=samples, seed=1)
        assert (got == samples).all()
    finally:
        scene.close()
    # inside a closed box of side 2: nothing is open, unless the radius ends before the nearest wall
    scene = open_scene(rt, box, **FLAVOURS[flavour])
    try:
        inside, any_way = rng.uniform(-0.5, 0.5, (n, 3)), rng.normal(size=(n, 3))
        assert (ambient(amb, scene, inside, any_way, samples=samples, seed=1) == 0).all()
        assert (ambient(amb, scene, inside, any_way, samples=samples, seed=1, radius=0.4) == samples).all()
    finally:
        scene.close()


def test_a_wall_beside_the_points_hides_half_of_the_hemisphere(rt, amb, gpu):
    """A floor and a wall of side 10^6 at 10^-2 beside the points: every sample that leans towards the wall meets it (all but
    ~10^-8 of them), every other one is open, and the cosine law is symmetric about the wall's plane: open / S has mean
    1/2 and, per ray, variance 1/4."""
    seed, base, n, samples = A.WALL
    tex, mat = [abi.solid((0.5, 0.5, 0.5))], [abi.material(abi.RT_MAT_LAMBERTIAN, 0)]
    prims = [abi.rect(abi.RT_PRIM_XZ_RECT, -5e5, 5e5, -5e5, 5e5, 0.0, 0, 1), abi.rect(abi.RT_PRIM_YZ_RECT, 0.0, 1e6, -5e5, 5e5, 0.0, 0, 2)]
    scene = open_scene(rt, abi.SceneBundle(prims, mat, tex, abi.sky()))
    try:
        rng = np.random.default_rng(4)
        points = np.column_stack([np.full(n, -1e-2), np.zeros(n), rng.uniform(-100, 100, n)])
        got = ambient(amb, scene, points, np.tile([0.0, 1.0, 0.0], (n, 1)), samples=samples, seed=seed, index_base=base)
    finally:
        scene.close()
    mean = (got / samples).mean()
    print("mean open / S = %.6f (1/2 +- %.2g)" % (mean, 5 * math.sqrt(0.25 / (n * samples))))
    assert (got >= 0).all() and (got <= samples).all()
    assert abs(mean - 0.5) <= 5 * math.sqrt(0.25 / (n * samples))


# ---- 4: addressing --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three_balls", TREE])
def test_halves_seeds_and_shapes(rt, amb, rays, gpu, name):
    import torch
    n, samples = 1000, 16
    scene, points, normals, time, hit, _ = hit_points(rt, rays, name, n)
    dev = torch.device("cuda", scene.device)
    try:
        whole = ambient(amb, scene, points, normals, time=time, samples=samples, seed=5)
        assert np.array_equal(whole != INVALID, hit) and (whole[hit] >= 0).all() and (whole[hit] <= samples).all()
        assert len(np.unique(whole[hit])) > 3
        # two halves, the second from index n / 2, are the whole batch
        half = n // 2
        a = ambient(amb, scene, points[:half], normals[:half], time=time[:half], samples=samples, seed=5)
        b = ambient(amb, scene, points[half:], normals[half:], time=time[half:], samples=samples, seed=5, index_base=half)
        assert np.array_equal(np.concatenate([a, b]), whole)
        unshifted = ambient(amb, scene, points[half:], normals[half:], time=time[half:], samples=samples, seed=5)
        assert not np.array_equal(unshifted, whole[half:])
        # another seed draws other rays
        assert not np.array_equal(ambient(amb, scene, points, normals, time=time, samples=samples, seed=6), whole)
        # shapes: nothing written past n, for every way a batch can end inside a wave (G = 16: four points a wave)
        tp, tn, tt = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (points, normals, time))
        for m in (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000):
            out = torch.full((m + 64,), SENTINEL, dtype=torch.int32, device=dev)
            got = amb.ambient_torch(scene, tp[:m].contiguous(), tn[:m].contiguous(), time=tt[:m].contiguous(), samples=samples, seed=5, out=out)
            torch.cuda.synchronize(dev)
            assert got is out
            assert np.array_equal(out[:m].cpu().numpy(), whole[:m]), m
            assert bool((out[m:] == SENTINEL).all()), m
        # S = 1 and S = 1024 at n = 3: one lane a point, and sixteen rounds of a whole wave a point
        few = np.nonzero(hit)[0][:3]
        for s_count in (1, 64, 1024):
            out = torch.full((3 + 64,), SENTINEL, dtype=torch.int32, device=dev)
            got, walked = amb.ambient_torch(scene, tp[few].contiguous(), tn[few].contiguous(), time=tt[few].contiguous(), samples=s_count,
                                            seed=5, out=out, export=True)
            verdict = importlib.import_module("racer-tracer_amd.occlusion").occluded_torch(
                scene, walked["origin"], walked["direction"], walked["t_min"], walked["t_max"], walked["time"])
            torch.cuda.synchronize(dev)
            assert bool((out[3:] == SENTINEL).all())
            verdict = verdict.cpu().numpy().reshape(3, s_count)
            assert np.array_equal(out[:3].cpu().numpy(), s_count - (verdict == 1).sum(axis=1)), s_count
            if s_count == 64:
                first = walked["direction"].cpu().numpy().reshape(3, 64, 3)
            if s_count == 1024:      # sample s of a point is the same ray whatever S is
                assert np.array_equal(walked["direction"].cpu().numpy().reshape(3, 1024, 3)[:, :64], first)
        # n == 0: RT_OK, nothing launched, nothing written
        out = torch.full((64,), SENTINEL, dtype=torch.int32, device=dev)
        assert amb.ambient_torch(scene, tp[:0].contiguous(), tn[:0].contiguous(), out=out) is out
        torch.cuda.synchronize(dev)
        assert bool((out == SENTINEL).all())
        assert amb.ambient(scene, points[:0], normals[:0]).shape == (0,)
        # what the binding refuses: another dtype, a view that is not contiguous, host memory, a short output
        with pytest.raises(ValueError):
            amb.ambient_torch(scene, tp.float(), tn)
        with pytest.raises(ValueError):
            amb.ambient_torch(scene, tp[::2], tn[::2])
        with pytest.raises(ValueError):
            amb.ambient_torch(scene, tp.cpu(), tn.cpu())
        with pytest.raises(ValueError):
            amb.ambient_torch(scene, tp, tn, out=torch.zeros(999, dtype=torch.int32, device=dev))
        with pytest.raises(rt.RtError):
            amb.ambient_torch(scene, tp, tn, samples=3)
    finally:
        scene.close()


def test_host_form_equals_device_form_across_a_chunk(rt, amb, rays, gpu):
    n = amb.RT_RAYS_HOST_CHUNK + 37
    scene, points, normals, time, hit, distance = hit_points(rt, rays, "three_balls", n)
    try:
        radius = np.where(np.arange(n) % 3 == 0, float(np.median(distance[hit])), np.inf)
        dev = ambient(amb, scene, points, normals, t_max=radius, time=time, samples=1, seed=9)
        host = amb.ambient(scene, points, normals, t_max=radius, time=time, samples=1, seed=9)
        plain_dev = ambient(amb, scene, points, normals, samples=1, seed=9)
        plain_host = amb.ambient(scene, points, normals, samples=1, seed=9)      # no optional plane: none staged
        # a chunk that forgot its index would repeat the first chunk's draws
        tail = ambient(amb, scene, points[-37:], normals[-37:], samples=1, seed=9)
    finally:
        scene.close()
    assert host.dtype == np.int32 and np.array_equal(host, dev)
    assert np.array_equal(plain_host, plain_dev)
    assert 0.2 < (dev[hit] == 1).mean() < 0.98 and np.array_equal(dev != INVALID, hit)
    assert not np.array_equal(tail, plain_dev[-37:])


# ---- 5: invalid points ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three_balls", TREE])
def test_invalid_points_are_marked_in_their_lane(rt, amb, rays, gpu, name):
    nan, inf = math.nan, math.inf
    kinds = [("origin", 0, nan), ("origin", 1, inf), ("origin", 2, -inf), ("normal", 0, nan), ("normal", 1, inf),
             ("normal", 2, -inf), ("time", None, nan), ("time", None, inf), ("t_min", None, nan), ("t_min", None, inf),
             ("t_min", None, -1e-3), ("t_max", None, nan), ("t_max", None, 0.5e-3), ("zero", None, 0.0)]
    n, samples = 2 * len(kinds) + 70, 16
    scene, points, normals, time, hit, _ = hit_points(rt, rays, name, 4 * n)
    keep = np.nonzero(hit)[0][:n]
    assert len(keep) == n
    clean = dict(origin=points[keep], normal=normals[keep], t_min=np.full(n, A.BIAS), t_max=np.full(n, inf), time=time[keep])
    dirty = {k: v.copy() for k, v in clean.items()}
    bad = np.zeros(n, dtype=bool)
    for k, (plane, axis, value) in enumerate(kinds):
        i = 2 * k + 1
        bad[i] = True
        if plane == "zero":
            dirty["normal"][i] = 0.0
        elif axis is None:
            dirty[plane][i] = value
        else:
            dirty[plane][i, axis] = value
    ask = lambda s, **kw: ambient(amb, scene, s["origin"], s["normal"], s["t_min"], s["t_max"], s["time"], samples=samples, seed=8, **kw)      # noqa: E731
    try:
        want = ask(clean)
        got, walked = ask(dirty, export=True)
        host = amb.ambient(scene, dirty["origin"], dirty["normal"], samples=samples, seed=8, t_min=dirty["t_min"], t_max=dirty["t_max"],
                           time=dirty["time"])
        # the planes override the params, point by point: params that would leave every sample open change nothing
        overridden = ask(clean, bias=0.25e-3, radius=0.5e-3)
        from_params = ambient(amb, scene, clean["origin"], clean["normal"], time=clean["time"], samples=samples, seed=8)
        tiny = ambient(amb, scene, clean["origin"], clean["normal"], time=clean["time"], samples=samples, seed=8, bias=0.25e-3, radius=0.5e-3)
    finally:
        scene.close()
    assert (want >= 0).all() and (want < samples).any()
    assert (got[bad] == INVALID).all()
    assert np.array_equal(got[~bad], want[~bad])
    assert np.array_equal(host, got)
    rows = np.repeat(bad, samples)
    assert (walked["direction"][rows] == 0).all() and (np.abs(walked["direction"][~rows]).max(axis=1) > 0.5).all()
    assert np.array_equal(walked["origin"], np.repeat(dirty["origin"], samples, axis=0), equal_nan=True)
    assert np.array_equal(walked["t_min"], np.repeat(dirty["t_min"], samples), equal_nan=True)
    assert np.array_equal(walked["t_max"], np.repeat(dirty["t_max"], samples), equal_nan=True)
    assert np.array_equal(overridden, want) and np.array_equal(from_params, want)
    assert (tiny == samples).all()


# ---- 6: the frame ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three_balls", TREE])
def test_frame_is_the_query_at_the_guides(rt, amb, gpu, name):
    import torch
    bundle, cam, _spread, closest_hit, in_lds = Q.scene(name)
    w, h, samples = 64, 48, 16
    p = abi.render_params(w, h, 8)
    camera = S.camera_for(cam, w, h)
    scene = open_scene(rt, bundle, closest_hit, in_lds)
    dev = torch.device("cuda", scene.device)
    try:
        before = scene.render_frame(camera, p)
        frame, guides = amb.ambient_frame_torch(scene, camera, p, samples=samples, seed=3)
        torch.cuda.synchronize(dev)
        mid = torch.full((w * h,), (camera.time_a + camera.time_b) * 0.5, dtype=torch.float64, device=dev)
        counts = amb.ambient_torch(scene, guides["position"].reshape(-1, 3), guides["normal"].reshape(-1, 3), samples=samples, seed=3, time=mid)
        torch.cuda.synchronize(dev)
        own = scene.render_guides(camera, p)
        host = amb.ambient_frame(scene, camera, p, samples=samples, seed=3)
        # the caller's own tensors are written in place
        mine = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        assert amb.ambient_frame_torch(scene, camera, p, samples=samples, seed=3, out=mine, guides=guides)[0] is mine
        torch.cuda.synchronize(dev)
        after = scene.render_frame(camera, p)
        with pytest.raises(rt.RtError):
            amb.ambient_frame(scene, camera, abi.render_params(w, h, 8, strip_count=2, strip_rows=24), samples=samples)
    finally:
        scene.close()
    never = open_scene(rt, bundle, closest_hit, in_lds)
    try:
        untouched = never.render_frame(camera, p)
    finally:
        never.close()
    frame, counts = frame.cpu().numpy(), counts.cpu().numpy().reshape(h, w)
    for plane, want in own.items():
        assert np.array_equal(guides[plane].cpu().numpy(), want, equal_nan=True), plane
    hit = own["obj_id"] != -1
    assert 0.1 < hit.mean() < 1.0 or name != "three_balls"
    assert np.array_equal(counts != INVALID, hit)
    want = np.sqrt(counts[hit].astype(np.float64) / samples)
    for c in range(3):
        assert np.array_equal(frame[..., c][hit], want), c
    assert (frame[~hit] == 1.0).all()
    assert len(np.unique(want)) > 3      # partly open hemispheres among them
    assert np.array_equal(host, frame) and np.array_equal(mine.cpu().numpy(), frame)
    assert np.array_equal(before, untouched, equal_nan=True) and np.array_equal(after, untouched, equal_nan=True)


def test_cli_ao_writes_the_frames_rgba8(rt, host, amb, gpu):
    """--ao 16: the PNG's decoded pixels are grey, and they are the tone-mapped ambient frame's RGBA8."""
    import torch
    exe = os.path.join(ROOT, "racer-tracer_amd", "bin", "racer-tracer-amd")
    config, scene_yml = os.path.join(ROOT, "scenes", "config_c1.yml"), os.path.join(ROOT, "scenes", "three_balls.yml")
    with tempfile.TemporaryDirectory(prefix="rt_ao_") as out:
        run = subprocess.run([exe, "-c", config, "-s", scene_yml, "--image-action", "png", "--seed", "1", "--ao", "16"],
                             capture_output=True, text=True, cwd=out, timeout=600)
        assert run.returncode == 0 and "Saved image to" in run.stderr, run.stderr[-2000:]
        pngs = [f for f in os.listdir(out) if f.endswith(".png")]
        assert len(pngs) == 1
        img = host.decode_image(os.path.join(out, pngs[0]))
    s = host.Session(config, scene=scene_yml, seed=1)
    scene = rt.Scene(s, device=0)
    dev = torch.device("cuda", scene.device)
    try:
        frame, _guides = amb.ambient_frame_torch(scene, s.camera, s.params, samples=16, seed=s.params.seed)
        n = s.params.width * s.params.height
        rgba = torch.zeros((s.params.height, s.params.width, 4), dtype=torch.uint8, device=dev)
        scene.post_rgba8_device(s.tone_map_desc, frame.data_ptr(), n, rgba.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        rgba, frame = rgba.cpu().numpy(), frame.cpu().numpy()
    finally:
        scene.close()
    assert img.shape == rgba.shape == (s.params.height, s.params.width, 4)
    assert (img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all() and (img[..., 3] == 255).all()
    assert len(np.unique(img[..., 0])) > 3
    assert np.array_equal(img, rgba)
    assert np.array_equal(img, host.pack_rgba8(s.tone_map(frame)))
    # a radius shorter than anything in reach leaves every hemisphere open: a white frame
    with tempfile.TemporaryDirectory(prefix="rt_ao_") as out:
        run = subprocess.run([exe, "-c", config, "-s", scene_yml, "--image-action", "png", "--seed", "1", "--ao", "4,0.002"],
                             capture_output=True, text=True, cwd=out, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        white = host.decode_image(os.path.join(out, [f for f in os.listdir(out) if f.endswith(".png")][0]))
    assert (white == 255).all()
