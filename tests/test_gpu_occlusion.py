"""The occlusion query (include/rt_occlusion.h) on the GPU: bit-for-bit agreement with the closest query's
"prim >= 0" on every scene form, both arithmetic flavours and both ray sets of tests/occlusion_model.py; agreement with
that model; the window's ends; launch shapes and what the binding refuses; invalid rays; the host form across a chunk
boundary; queries next to renders of a tree that is re-ordered per camera; the visibility helper and the CLI flag."""
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import occlusion_model as M
import ray_query_model as Q
import scenes_py as S

pytestmark = pytest.mark.gpu
abi = Q.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 0.9999       # tests/test_gpu_rays.py: the share of THE random set's rays on which device and model name the same primitive
TREE = "form-2-0-0-1"      # a tree (staged in LDS by renders) with moving and wrapped primitives
FLAVOURS = {"fast": {}, "exact": dict(arithmetic=abi.RT_ARITH_REFERENCE)}


@pytest.fixture(scope="module")
def occ():
    return importlib.import_module("racer-tracer_amd.occlusion")


@pytest.fixture(scope="module")
def rays():
    return importlib.import_module("racer-tracer_amd.rays")


@pytest.fixture(scope="module")
def sets(orc):
    """(name, "A" | "B") -> the set of tests/occlusion_model.py at this file's n; computed once, never written to."""
    cache = {}

    def get(name, which):
        if (name, which) not in cache:
            cache[name, which] = M.set_a(orc, name, M.N_A) if which == "A" else M.set_b(orc, name, M.N_B)
        return cache[name, which]
    return get


def open_scene(rt, s, **options):
    scene = rt.Scene(s["bundle"], closest_hit=s["closest_hit"], **options)
    variant = scene.variant()
    assert variant["use_bvh"] == int(s["in_lds"] is not None)
    if s["in_lds"] is not None:
        assert variant["bvh_nodes_in_lds"] == s["in_lds"]
    assert variant["exact"] == int("arithmetic" in options)
    return scene


def up(scene, a):
    import torch
    return None if a is None else torch.tensor(np.asarray(a), dtype=torch.float64, device=torch.device("cuda", scene.device))


def occluded(occ, scene, o, d, t_min=None, t_max=None, time=None):
    """occluded_torch on numpy rays -> numpy int32."""
    import torch
    got = occ.occluded_torch(scene, up(scene, o), up(scene, d), up(scene, t_min), up(scene, t_max), up(scene, time))
    torch.cuda.synchronize(torch.device("cuda", scene.device))
    return got.cpu().numpy()


def closest(rays, scene, o, d, t_min=None, t_max=None, time=None, planes=("t", "prim")):
    """rt_trace_rays_device, RT_RAYS_CLOSEST, on numpy rays -> numpy planes."""
    import torch
    got = rays.trace_rays_torch(scene, up(scene, o), up(scene, d), up(scene, t_min), up(scene, t_max), up(scene, time), planes=planes)
    torch.cuda.synchronize(torch.device("cuda", scene.device))
    return {k: v.cpu().numpy() for k, v in got.items()}


# ---- the rule: occluded == the closest query reports a hit, bit for bit; and the model -----------------------------------------

@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("name", Q.SCENES)
def test_occluded_is_the_closest_query_reporting_a_hit(rt, occ, rays, gpu, sets, name, flavour):
    """No ray excused.  On a linear scene the first acceptance happens with the window at t_max in both loops; on a tree both
    walks visit the same nodes in the same order until the first acceptance, and make the same decisions when there is
    none: a disagreement is a bug in the new walk, not rounding.  Against the model: the cap of tests/test_gpu_rays.py."""
    a, b = sets(name, "A"), sets(name, "B")
    scene = open_scene(rt, a, **FLAVOURS[flavour])
    try:
        for which, s in (("A", a), ("B", b)):
            got = occluded(occ, scene, s["origin"], s["direction"], t_max=s["t_max"], time=s["time"])
            near = closest(rays, scene, s["origin"], s["direction"], t_max=s["t_max"], time=s["time"], planes=("prim",))["prim"]
            differ = got != (near >= 0)
            agree = got == s["want"]
            print("%s %s set %s: %d of %d occluded, %d differ from the closest query, %d from the model" %
                  (name, flavour, which, (got == 1).sum(), got.size, differ.sum(), (~agree).sum()))
            assert got.dtype == np.int32 and np.isin(got, (0, 1)).all()
            assert not differ.any(), (which, np.nonzero(differ)[0][:8])
            assert agree.mean() >= CAP, which
    finally:
        scene.close()


# ---- the window's ends -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three_balls", TREE])
def test_window_ends_are_inclusive(rt, orc, occ, rays, gpu, sets, name):
    b = sets(name, "B")      # (its rays: n = 4096; its window is not used)
    o, d, time, n = b["origin"], b["direction"], b["time"], M.N_B
    scene = open_scene(rt, b)
    try:
        first = closest(rays, scene, o, d, time=time)
        t, hit = first["t"], first["prim"] >= 0      # the device's own closest t: inf on a miss
        assert (hit == (b["closest"]["prim"] >= 0)).mean() >= CAP and 0.3 < hit.mean() < 0.95
        # t_max = t: the far end is inclusive, bit for bit (a miss keeps its infinite window and stays a miss)
        assert np.array_equal(occluded(occ, scene, o, d, t_max=t, time=time), hit.astype(np.int32))
        for factor in (1.0 - 1e-6, 1.0 + 1e-6):
            got = occluded(occ, scene, o, d, t_max=t * factor, time=time)
            want = M.expected(orc, b["bundle"], o, d, t_max=t * factor, time=time)
            print("%s t_max = %r t: %d of %d occluded, %d differ from the model" % (name, factor, (got == 1).sum(), n, (got != want).sum()))
            assert (got == want).mean() >= CAP, factor
            if factor > 1.0:
                assert np.array_equal(got, hit.astype(np.int32))      # the device's own hit lies inside
        # t_min = t: the near end is inclusive (a miss keeps the default: inf is no t_min)
        assert np.array_equal(occluded(occ, scene, o, d, t_min=np.where(hit, t, Q.T_MIN), time=time), hit.astype(np.int32))
        # t_min = t_max = 0 is a valid window that holds no hit
        assert (occluded(occ, scene, o, d, t_min=np.zeros(n), t_max=np.zeros(n), time=time) == 0).all()
    finally:
        scene.close()


# ---- shapes, nothing written past n, what the binding refuses -----------------------------------------------------------------
SENTINEL = -777


@pytest.mark.parametrize("name", ["three_balls", TREE])
def test_shapes_and_refusals(rt, occ, gpu, name):
    import torch
    bundle, cam, spread, closest_hit, in_lds = Q.scene(name)
    o, d, time = Q.random_rays(cam, 1000, spread)
    scene = open_scene(rt, dict(bundle=bundle, closest_hit=closest_hit, in_lds=in_lds))
    dev = torch.device("cuda", scene.device)
    try:
        # the full call: every optional plane given (the window's with the defaults' values)
        full = occluded(occ, scene, o, d, t_min=np.full(1000, Q.T_MIN), t_max=np.full(1000, np.inf), time=time)
        assert 300 < (full == 1).sum() < 950 and np.isin(full, (0, 1)).all()
        to, td, tt = (torch.from_numpy(a).to(dev) for a in (o, d, time))
        for n in (1, 63, 64, 65, 255, 256, 257, 1000):
            out = torch.full((n + 64,), SENTINEL, dtype=torch.int32, device=dev)
            got = occ.occluded_torch(scene, to[:n].contiguous(), td[:n].contiguous(), time=tt[:n].contiguous(), out=out)
            torch.cuda.synchronize(dev)
            assert got is out
            assert np.array_equal(out[:n].cpu().numpy(), full[:n]), n
            assert bool((out[n:] == SENTINEL).all()), n
        # n == 0: RT_OK, nothing launched, nothing written
        out = torch.full((64,), SENTINEL, dtype=torch.int32, device=dev)
        assert occ.occluded_torch(scene, to[:0].contiguous(), td[:0].contiguous(), out=out) is out
        assert occ.occluded_torch(scene, to[:0].contiguous(), td[:0].contiguous()).shape == (0,)
        torch.cuda.synchronize(dev)
        assert bool((out == SENTINEL).all())
        assert occ.occluded(scene, o[:0], d[:0]).shape == (0,)
        # what the binding refuses: another dtype, a view that is not contiguous, host memory — rays and output alike
        with pytest.raises(ValueError):
            occ.occluded_torch(scene, to.float(), td)
        with pytest.raises(ValueError):
            occ.occluded_torch(scene, to[::2], td[::2])
        with pytest.raises(ValueError):
            occ.occluded_torch(scene, to.cpu(), td.cpu())
        with pytest.raises(ValueError):
            occ.occluded_torch(scene, to, td, out=torch.zeros(1000, dtype=torch.int64, device=dev))
        with pytest.raises(ValueError):
            occ.occluded_torch(scene, to, td, out=torch.zeros(2000, dtype=torch.int32, device=dev)[::2])
        with pytest.raises(ValueError):
            occ.occluded_torch(scene, to, td, out=torch.zeros(1000, dtype=torch.int32))
        with pytest.raises(ValueError):
            occ.occluded_torch(scene, to, td, out=torch.zeros(999, dtype=torch.int32, device=dev))
    finally:
        scene.close()


# ---- invalid rays --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three_balls", TREE])
def test_invalid_rays_are_marked_in_their_lane(rt, occ, gpu, name):
    bundle, cam, spread, closest_hit, in_lds = Q.scene(name)
    nan, inf = math.nan, math.inf
    kinds = [("origin", 0, nan), ("origin", 1, inf), ("origin", 2, -inf), ("direction", 0, nan), ("direction", 1, inf),
             ("direction", 2, -inf), ("time", None, nan), ("time", None, inf), ("t_min", None, nan), ("t_min", None, inf),
             ("t_min", None, -1e-3), ("t_max", None, nan), ("t_max", None, 0.5e-3), ("zero", None, 0.0)]
    n = 2 * len(kinds) + 70      # more than one wave; invalid rays at the odd places of the first 2 len(kinds)
    o, d, time = Q.random_rays(cam, n, spread)
    clean = dict(origin=o, direction=d, t_min=np.full(n, Q.T_MIN), t_max=np.full(n, inf), time=time)
    dirty = {k: v.copy() for k, v in clean.items()}
    bad = np.zeros(n, dtype=bool)
    for k, (plane, axis, value) in enumerate(kinds):
        i = 2 * k + 1
        bad[i] = True
        if plane == "zero":
            dirty["direction"][i] = 0.0
        elif axis is None:
            dirty[plane][i] = value
        else:
            dirty[plane][i, axis] = value
    scene = open_scene(rt, dict(bundle=bundle, closest_hit=closest_hit, in_lds=in_lds))
    try:
        want = occluded(occ, scene, clean["origin"], clean["direction"], clean["t_min"], clean["t_max"], clean["time"])
        got = occluded(occ, scene, dirty["origin"], dirty["direction"], dirty["t_min"], dirty["t_max"], dirty["time"])
        host = occ.occluded(scene, dirty["origin"], dirty["direction"], dirty["t_min"], dirty["t_max"], dirty["time"])
    finally:
        scene.close()
    assert np.isin(want, (0, 1)).all() and (want == 1).sum() > n // 4
    assert (got[bad] == occ.RT_RAY_INVALID).all()
    assert np.array_equal(got[~bad], want[~bad])
    assert np.array_equal(host, got)


# ---- the host form -------------------------------------------------------------------------------------------------------------

def test_host_form_equals_device_form_across_a_chunk(rt, occ, gpu):
    bundle, cam, spread, closest_hit, in_lds = Q.scene("three_balls")
    n = occ.RT_RAYS_HOST_CHUNK + 1
    o, d, time = Q.random_rays(cam, n, spread)
    # (the directions end at targets around look_at, where the spheres are: the hits lie around t = 1)
    t_max = np.where(np.arange(n) % 3 == 0, 1.0, np.inf)
    scene = open_scene(rt, dict(bundle=bundle, closest_hit=closest_hit, in_lds=in_lds))
    try:
        dev = occluded(occ, scene, o, d, t_max=t_max, time=time)
        host = occ.occluded(scene, o, d, t_max=t_max, time=time)
        plain_dev = occluded(occ, scene, o, d)
        plain_host = occ.occluded(scene, o, d)      # no optional plane: none staged
    finally:
        scene.close()
    assert 0.3 < (dev == 1).mean() < 0.95 and (plain_dev == 1).sum() > (dev == 1).sum()
    assert host.dtype == np.int32 and np.array_equal(host, dev)
    assert np.array_equal(plain_host, plain_dev)


# ---- a tree that renders re-order for their camera -----------------------------------------------------------------------------

def test_queries_and_renders_of_a_reordered_tree_leave_each_other_alone(rt, occ, gpu, sets):
    s = sets(TREE, "B")
    cam = Q.scene(TREE)[1]
    p = abi.render_params(64, 36, 8)
    camera = S.camera_for(cam, p.width, p.height)
    other = S.camera_for(dict(cam, look_from=tuple(-x for x in cam["look_from"])), p.width, p.height)
    ask = lambda scene: occluded(occ, scene, s["origin"], s["direction"], t_max=s["t_max"], time=s["time"])      # noqa: E731
    scene = open_scene(rt, s)
    try:
        a = ask(scene)
        frame_a = scene.render_frame(camera, p)
        b = ask(scene)      # behind a render: the tree's global copy is in that camera's child order
        frame_b = scene.render_frame(other, p)
        c = ask(scene)      # ... and in the order of a camera on the other side
        frame_c = scene.render_frame(camera, p)
    finally:
        scene.close()
    never = open_scene(rt, s)      # the same renders on a scene that is never queried
    try:
        frames = [never.render_frame(camera, p), never.render_frame(other, p), never.render_frame(camera, p)]
    finally:
        never.close()
    assert 0.2 < (a == 1).mean() < 0.8
    assert np.array_equal(a, b) and np.array_equal(a, c)
    for got, want in zip((frame_a, frame_b, frame_c), frames):
        assert np.array_equal(got, want, equal_nan=True)
    assert not np.array_equal(frame_a, frame_b)


# ---- the helper ----------------------------------------------------------------------------------------------------------------

def test_visible_between_is_occluded_on_the_segments_ray(rt, occ, gpu, sets):
    import torch
    s = sets("three_balls", "B")
    points = s["closest"]["point"][s["closest"]["prim"] >= 0]      # the model's hit points: ON the surfaces
    a, b = points, np.ascontiguousarray(np.roll(points, 1, axis=0))
    eps = 1e-3
    n = len(a)
    scene = open_scene(rt, s)
    dev = torch.device("cuda", scene.device)
    try:
        visible = occ.visible_between(scene, a, b)
        on_device = occ.visible_between_torch(scene, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy()
        direct = occ.occluded(scene, a, b - a, t_min=np.full(n, eps), t_max=np.full(n, 1.0 - eps))
        wide = occ.visible_between(scene, a, b, eps=0.5)      # the window is the segment's midpoint alone
        with pytest.raises(ValueError):
            occ.visible_between(scene, a, b, eps=0.6)
        with pytest.raises(ValueError):
            occ.visible_between_torch(scene, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), eps=0.6)
    finally:
        scene.close()
    print("%d of %d segments between hit points are free" % (visible.sum(), n))
    assert visible.dtype == np.bool_ and visible.shape == (n,)
    assert np.isin(direct, (0, 1)).all() and np.array_equal(visible, direct == 0)
    assert np.array_equal(on_device, visible)
    assert 0.05 < visible.mean() < 0.95
    assert wide.sum() >= visible.sum()


# ---- CLI -----------------------------------------------------------------------------------------------------------------------

def test_cli_visible_prints_yes_and_no(gpu):
    """--visible on three_balls.yml (the centre sphere: radius 0.5 around (0, 0, -1); the ground's top at y = -0.5): a
    segment well above everything is free, one through the centre sphere is not."""
    exe = os.path.join(ROOT, "racer-tracer_amd", "bin", "racer-tracer-amd")
    config, scene_yml = os.path.join(ROOT, "scenes", "config_c1.yml"), os.path.join(ROOT, "scenes", "three_balls.yml")
    base = [exe, "-c", config, "-s", scene_yml, "--image-action", "none", "--seed", "1"]
    free = subprocess.run(base + ["--visible", "0,2,-1,3,2,-1"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert free.returncode == 0, free.stderr
    assert free.stdout.split() == ["visible", "0", "2", "-1", "3", "2", "-1", "yes"], free.stdout
    blocked = subprocess.run(base + ["--visible=0,0,1,0,0,-3"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert blocked.returncode == 0, blocked.stderr
    assert blocked.stdout.split() == ["visible", "0", "0", "1", "0", "0", "-3", "no"], blocked.stdout
    for bad in ("1,2,3,4,5", "1,2,3,4,5,6,7", "1,2,3,4,5,", "a,b,c,d,e,f", "1,2,3,4,5,inf", "1,2,3,nan,5,6", ""):
        r = subprocess.run(base + ["--visible", bad], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode != 0 and r.stdout == "" and "--visible" in r.stderr, (bad, r.stderr)
