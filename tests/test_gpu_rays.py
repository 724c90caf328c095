"""The ray query (include/rt_rays.h) on the GPU against tests/ray_query_model.py: every probe of
tests/ray_probes.py with no ray excused, THE random ray set on every scene form, windows, launch shapes and NULL planes,
invalid rays, any mode, the host form across a chunk boundary, and determinism next to renders."""
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import ray_probes as P
import ray_query_model as Q
import scenes_py as S

pytestmark = pytest.mark.gpu
abi = Q.abi
BOUND = 1e-9       # tests/test_gpu_ray_probes.py: GUIDE, the guides' planes against the oracle's
N = 16384
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rays():
    return importlib.import_module("racer-tracer_amd.rays")


def query(rays, scene, o, d, t_min=None, t_max=None, time=None, **kw):
    """trace_rays_torch on numpy rays -> numpy planes."""
    import torch
    dev = torch.device("cuda", scene.device)
    up = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=torch.float64, device=dev)      # noqa: E731
    got = rays.trace_rays_torch(scene, up(o), up(d), up(t_min), up(t_max), up(time), **kw)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in got.items()}


def within(got, want):
    """|got - want| <= BOUND max(1, |want|); a NaN answers a NaN (a MovingSphere's v is acos of the hit POINT's -y, SURVEY B-19:
    NaN wherever |y| > 1, in the reference as here)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(got - want) <= BOUND * np.maximum(1.0, np.abs(want))) | (np.isnan(got) & np.isnan(want))


def same(a, b):
    """array_equal, a NaN equal to a NaN in the f64 planes."""
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_records(got, want, rows, what):
    """On `rows` (where prim agrees): the record within BOUND max(1, |want|), the integers equal; misses bit for bit."""
    for plane in ("t", "point", "normal", "uv"):
        hit = rows & (want["prim"] >= 0)
        assert within(got[plane][hit], want[plane][hit]).all(), (what, plane)
    for plane in ("obj_id", "front_face"):
        assert np.array_equal(got[plane][rows], want[plane][rows]), (what, plane)
    miss = rows & (want["prim"] < 0)
    for plane in Q.PLANES:
        assert np.array_equal(got[plane][miss], want[plane][miss]), (what, plane, "miss")


# ---- probes: no ray excused ----------------------------------------------------------------------------------------------------
# flavour -> (scene options, the route of tests/ray_probes.py whose open ties apply, the routes that make a probe run here)
FLAVOURS = {
    "fast": (dict(closest_hit=abi.RT_HIT_LINEAR), "guides", ("pool-fast", "v1-fast", "guides")),
    "exact": (dict(closest_hit=abi.RT_HIT_LINEAR, arithmetic=abi.RT_ARITH_REFERENCE), "pool-exact", P.EXACT_ROUTES),
    "tree": (dict(closest_hit=abi.RT_HIT_BVH), "pool-fast-bvh", ("pool-fast-bvh",)),
}
PROBE_CASES = [(name, fl) for name, probe in P.PROBES.items() for fl, (_, _, runs) in FLAVOURS.items()
               if set(runs) & set(probe.routes)]


@pytest.fixture(scope="module")
def probe_model(orc):
    cache = {}

    def get(name, fillers):
        if (name, fillers) not in cache:
            probe = P.PROBES[name]
            o, d, time = Q.probe_rays(probe)
            want = Q.expected(orc, probe.bundle(fillers=fillers), o, d, time=time)
            for a in (o, d, time, *want.values()):
                a.setflags(write=False)
            cache[name, fillers] = (o, d, time, want)
        return cache[name, fillers]
    return get


@pytest.mark.parametrize("name,flavour", PROBE_CASES, ids=lambda x: str(x))
def test_probe_matches_model(rt, rays, gpu, probe_model, name, flavour):
    probe = P.PROBES[name]
    options, tie_route, _ = FLAVOURS[flavour]
    fillers = flavour == "tree"
    o, d, time, want = probe_model(name, fillers)
    scene = rt.Scene(probe.bundle(fillers=fillers), **options)
    try:
        variant = scene.variant()
        got = query(rays, scene, o, d, time=time)
    finally:
        scene.close()
    assert variant["use_bvh"] == int(fillers) and variant["exact"] == int(flavour == "exact")
    open_tie = probe.tie is not None and tie_route in probe.tie[0]
    hit = want["prim"] >= 0
    print("%s %s: %d of %d rays hit, max |delta point| %.3g" % (name, flavour, hit.sum(), hit.size,
                                                                 np.abs(got["point"] - want["point"]).max()))
    if open_tie and len(probe.tie[1]) > 1:      # two primitives at one t: either, and the same one in both planes
        tied = np.isin(want["obj_id"], probe.tie[1])
        assert np.isin(got["obj_id"][tied], probe.tie[1]).all()
        assert same(got["obj_id"][tied], got["prim"][tied] + 1)
        assert same(got["obj_id"][~tied], want["obj_id"][~tied])
        assert same(got["prim"][~tied], want["prim"][~tied])
    else:
        assert same(got["prim"], want["prim"])
        assert same(got["obj_id"], want["obj_id"])
    assert np.abs(got["point"] - want["point"]).max() < BOUND
    if open_tie and probe.tie[2]:      # the side of a box on its edge: the normal of one of the tied sides, against the ray
        sides = [np.array(n) for n in probe.tie[2]]
        for n in got["normal"][hit]:
            assert any(same(n, s) for s in sides), n
        return
    assert np.abs(got["normal"] - want["normal"]).max() < BOUND
    nz = want["normal"] != 0.0
    assert same(np.signbit(got["normal"][nz]), np.signbit(want["normal"][nz]))


# ---- every scene form ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sets(orc):
    """name -> (bundle, options, tree in LDS or None, origin, direction, time, the model's planes); computed once."""
    cache = {}

    def get(name, n=N):
        if (name, n) not in cache:
            bundle, cam, spread, closest_hit, in_lds = Q.scene(name)
            o, d, time = Q.random_rays(cam, n, spread)
            want = Q.expected(orc, bundle, o, d, time=time)
            for a in (o, d, time, *want.values()):
                a.setflags(write=False)
            cache[name, n] = (bundle, closest_hit, in_lds, o, d, time, want)
        return cache[name, n]
    return get


def open_scene(rt, bundle, closest_hit, in_lds):
    scene = rt.Scene(bundle, closest_hit=closest_hit)
    variant = scene.variant()
    assert variant["use_bvh"] == int(in_lds is not None)
    if in_lds is not None:
        assert variant["bvh_nodes_in_lds"] == in_lds
    return scene


@pytest.mark.parametrize("name", Q.SCENES)
def test_random_rays_match_model_on_every_form(rt, rays, gpu, sets, name):
    bundle, closest_hit, in_lds, o, d, time, want = sets(name)
    scene = open_scene(rt, bundle, closest_hit, in_lds)
    try:
        got = query(rays, scene, o, d, time=time)
    finally:
        scene.close()
    agree = got["prim"] == want["prim"]
    print("%s: %d of %d rays differ in prim; max |delta t| on the rest %.3g" %
          (name, (~agree).sum(), N, np.abs(got["t"][agree & (want["prim"] >= 0)] - want["t"][agree & (want["prim"] >= 0)]).max()))
    assert agree.mean() >= 0.9999
    assert_records(got, want, agree, name)


# ---- windows -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three_balls", "form-2-0-0-0"])
def test_windows_follow_the_model(rt, orc, rays, gpu, sets, name):
    n = 4096
    bundle, closest_hit, in_lds, o, d, time, want = sets(name, n)
    hit = want["prim"] >= 0
    scene = open_scene(rt, bundle, closest_hit, in_lds)
    try:
        first = query(rays, scene, o, d, time=time)
        assert (first["prim"] == want["prim"]).mean() >= 0.9999
        kept = first["prim"] == want["prim"]
        for factor in (0.5, 1.0 - 1e-6, 1.0, 1.0 + 1e-6):
            # at 1 exactly the device's own t is fed back: the window's end is inclusive, bit for bit
            t_max = (first["t"] if factor == 1.0 else want["t"]) * factor
            got = query(rays, scene, o, d, t_max=t_max, time=time)
            if factor == 1.0:
                for plane in Q.PLANES:
                    assert same(got[plane], first[plane]), (plane, "t_max = t")
                continue
            model = Q.expected(orc, bundle, o, d, t_max=t_max, time=time)
            agree = got["prim"] == model["prim"]
            print("%s t_max = %r t: %d rays differ, %d hit" % (name, factor, (~agree).sum(), (model["prim"] >= 0).sum()))
            assert agree.mean() >= 0.9999
            assert_records(got, model, agree, (name, "t_max", factor))
        for factor in (1.0, 1.0 + 1e-6):
            base = first["t"] if factor == 1.0 else want["t"]
            t_min = np.where(np.isfinite(base), base * factor, Q.T_MIN)      # (a miss keeps the default: inf is no t_min)
            got = query(rays, scene, o, d, t_min=t_min, time=time)
            if factor == 1.0:
                for plane in Q.PLANES:
                    assert same(got[plane], first[plane]), (plane, "t_min = t")
                continue
            model = Q.expected(orc, bundle, o, d, t_min=t_min, time=time)
            agree = got["prim"] == model["prim"]
            print("%s t_min = %r t: %d rays differ, %d hit" % (name, factor, (~agree).sum(), (model["prim"] >= 0).sum()))
            assert agree.mean() >= 0.9999
            assert_records(got, model, agree, (name, "t_min", factor))
            assert (got["t"][hit & kept & agree] > want["t"][hit & kept & agree]).all()
    finally:
        scene.close()


# ---- shapes, NULL planes, nothing written past n ------------------------------------------------------------------------------
SENTINEL_F, SENTINEL_I = -12345.5, -777


def sentinel_out(rays, scene, n):
    import torch
    dev = torch.device("cuda", scene.device)
    out = {}
    for plane, (width, is_double) in rays.HIT_PLANES.items():
        shape = (n + 64,) if width == 1 else (n + 64, width)
        out[plane] = (torch.full(shape, SENTINEL_F, dtype=torch.float64, device=dev) if is_double
                      else torch.full(shape, SENTINEL_I, dtype=torch.int32, device=dev))
    return out


def untouched(a):
    return bool((a == (SENTINEL_F if a.dtype.is_floating_point else SENTINEL_I)).all())


def test_shapes_and_null_planes(rt, rays, gpu):
    import torch
    bundle, cam, spread, closest_hit, in_lds = Q.scene("three_balls")
    o, d, _ = Q.random_rays(cam, 1000, spread)
    scene = open_scene(rt, bundle, closest_hit, in_lds)
    dev = torch.device("cuda", scene.device)
    try:
        # the full call: every optional plane given, with the defaults' values
        full = query(rays, scene, o, d, t_min=np.full(1000, Q.T_MIN), t_max=np.full(1000, np.inf), time=np.zeros(1000))
        assert 300 < (full["prim"] >= 0).sum() < 950
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        for n in (1, 63, 64, 65, 255, 256, 257, 1000):
            out = sentinel_out(rays, scene, n)
            got = rays.trace_rays_torch(scene, to[:n].contiguous(), td[:n].contiguous(), out=out)
            torch.cuda.synchronize(dev)
            for plane in rays.HIT_PLANES:
                assert got[plane] is out[plane]
                assert same(out[plane][:n].cpu().numpy(), full[plane][:n]), (n, plane)
                assert untouched(out[plane][n:]), (n, plane)
        n = 257
        for left_out in rays.HIT_PLANES:      # each output plane NULL in turn: not written, its neighbours as ever
            out = sentinel_out(rays, scene, n)
            planes = tuple(p for p in rays.HIT_PLANES if p != left_out)
            got = rays.trace_rays_torch(scene, to[:n].contiguous(), td[:n].contiguous(), planes=planes, out=out)
            torch.cuda.synchronize(dev)
            assert sorted(got) == sorted(planes)
            assert untouched(out[left_out]), left_out
            for plane in planes:
                assert same(out[plane][:n].cpu().numpy(), full[plane][:n]), (left_out, plane)
                assert untouched(out[plane][n:]), (left_out, plane)
        # what the binding refuses: another dtype, a view that is not contiguous, host memory
        with pytest.raises(ValueError):
            rays.trace_rays_torch(scene, to.float(), td)
        with pytest.raises(ValueError):
            rays.trace_rays_torch(scene, to[::2], td[::2])
        with pytest.raises(ValueError):
            rays.trace_rays_torch(scene, to.cpu(), td.cpu())
        # n == 0: RT_OK, nothing enqueued
        empty = rays.trace_rays_torch(scene, to[:0].contiguous(), td[:0].contiguous())
        assert all(v.shape[0] == 0 for v in empty.values())
    finally:
        scene.close()


# ---- invalid rays --------------------------------------------------------------------------------------------------------------

def test_invalid_rays_are_marked_in_their_lane(rt, rays, gpu):
    bundle, cam, spread, closest_hit, in_lds = Q.scene("form-2-0-0-0")
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
    scene = open_scene(rt, bundle, closest_hit, in_lds)
    try:
        want = query(rays, scene, clean["origin"], clean["direction"], clean["t_min"], clean["t_max"], clean["time"])
        got = query(rays, scene, dirty["origin"], dirty["direction"], dirty["t_min"], dirty["t_max"], dirty["time"])
        # t_min == 0 and t_max == t_min are valid windows
        edge = query(rays, scene, o, d, t_min=np.zeros(n), t_max=np.zeros(n), time=time)
    finally:
        scene.close()
    assert (want["prim"] >= 0).sum() > n // 4 and (want["prim"] != rays.RT_RAY_INVALID).all()
    none = Q.empty(n)
    for plane in Q.PLANES:
        assert same(got[plane][~bad], want[plane][~bad]), plane
        if plane != "prim":
            assert same(got[plane][bad], none[plane][bad]), plane
    assert (got["prim"][bad] == rays.RT_RAY_INVALID).all()
    assert (edge["prim"] == rays.RT_RAY_MISS).all()


# ---- any mode ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", Q.SCENES)
def test_any_mode_reports_a_hit_of_the_window(rt, orc, rays, gpu, sets, name):
    bundle, closest_hit, in_lds, o, d, time, want = sets(name)
    scene = open_scene(rt, bundle, closest_hit, in_lds)
    try:
        got = query(rays, scene, o, d, time=time, mode=rays.RT_RAYS_ANY)
        only = query(rays, scene, o, d, time=time, mode=rays.RT_RAYS_ANY, planes=("prim",))
    finally:
        scene.close()
    assert same(only["prim"], got["prim"]) and list(only) == ["prim"]
    agree = (got["prim"] >= 0) == (want["prim"] >= 0)
    print("%s any: %d rays differ in hit / miss" % (name, (~agree).sum()))
    assert agree.mean() >= 0.9999
    assert (got["prim"] >= Q.MISS).all() and (got["prim"] < bundle.desc.n_primitives).all()
    hit = got["prim"] >= 0
    assert same(got["obj_id"][hit], got["prim"][hit] + 1)
    worst = 0.0
    for i in np.nonzero(hit & agree)[0]:
        t = Q.primitive_t(orc, bundle.primitives[int(got["prim"][i])], o[i], d[i], time[i], Q.T_MIN, math.inf)
        assert t is not None, (name, i)
        worst = max(worst, abs(t - got["t"][i]) / max(1.0, abs(t)))
    print("%s any: worst |delta t| / max(1, t) %.3g" % (name, worst))
    assert worst <= BOUND
    miss = ~hit
    none = Q.empty(N)
    for plane in Q.PLANES:
        assert same(got[plane][miss], none[plane][miss]), plane


# ---- the host form -------------------------------------------------------------------------------------------------------------

def test_host_form_equals_device_form_across_a_chunk(rt, rays, gpu):
    bundle, cam, spread, closest_hit, in_lds = Q.scene("three_balls")
    n = rays.RT_RAYS_HOST_CHUNK + 1
    o, d, time = Q.random_rays(cam, n, spread)
    t_max = np.where(np.arange(n) % 3 == 0, 11.0, np.inf)
    scene = open_scene(rt, bundle, closest_hit, in_lds)
    try:
        dev = query(rays, scene, o, d, t_max=t_max, time=time)
        host = rays.trace_rays(scene, o, d, t_max=t_max, time=time)
        few = rays.trace_rays(scene, o, d, t_max=t_max, time=time, planes=("t", "prim"))
        any_host = rays.trace_rays(scene, o[:1000], d[:1000], mode=rays.RT_RAYS_ANY)
        any_dev = query(rays, scene, o[:1000], d[:1000], mode=rays.RT_RAYS_ANY)
    finally:
        scene.close()
    assert 0.3 < (dev["prim"] >= 0).mean() < 0.95
    for plane in Q.PLANES:
        assert same(host[plane], dev[plane]), plane
        assert same(any_host[plane], any_dev[plane]), plane
    assert sorted(few) == ["prim", "t"]
    assert same(few["t"], dev["t"]) and same(few["prim"], dev["prim"])


# ---- determinism, next to renders ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["form-2-0-0-1", "cornell_box_boxes"])
def test_queries_and_renders_leave_each_other_alone(rt, rays, gpu, name):
    bundle, cam, spread, closest_hit, in_lds = Q.scene(name)
    o, d, time = Q.random_rays(cam, 4096, spread)
    p = abi.render_params(64, 36, 8)
    camera = S.camera_for(cam, p.width, p.height)
    other = S.camera_for(dict(cam, look_from=tuple(-x for x in cam["look_from"])), p.width, p.height)
    scene = open_scene(rt, bundle, closest_hit, in_lds)
    try:
        a = query(rays, scene, o, d, time=time)
        b = query(rays, scene, o, d, time=time)
        frame_a = scene.render_frame(camera, p)
        c = query(rays, scene, o, d, time=time)       # behind a render (a tree in LDS was re-ordered for its camera)
        scene.render_frame(other, p)
        e = query(rays, scene, o, d, time=time)       # ... and for a camera on the other side
        frame_b = scene.render_frame(camera, p)
    finally:
        scene.close()
    for plane in Q.PLANES:
        assert same(a[plane], b[plane]), plane
        assert same(a[plane], c[plane]), plane
        # another child order: only exact ties may differ, and the set has none (tests/test_rays_cpu.py)
        assert same(a[plane], e[plane]), plane
    assert same(frame_a, frame_b)


# ---- CLI -----------------------------------------------------------------------------------------------------------------------

def test_cli_pick_prints_what_the_guides_see(rt, host, gpu):
    """--pick X,Y on three_balls.yml with config_c1.yml, one hit pixel and one sky pixel: the printed prim and obj_id name
    the object render_guides sees at that pixel, t, point and normal are its footprint, position and normal.  (The CLI forms the pixel's
    ray on the host, the guides form it in the kernel, with the fast flavour's contractions: the numbers are held to the
    bound of every other comparison with the guides, BOUND max(1, |want|), and the guides carry t as the footprint
    t |vertical| / (H - 1).)"""
    exe = os.path.join(ROOT, "racer-tracer_amd", "bin", "racer-tracer-amd")
    config, scene_yml = os.path.join(ROOT, "scenes", "config_c1.yml"), os.path.join(ROOT, "scenes", "three_balls.yml")
    session = host.Session(config, scene=scene_yml)
    scene = rt.Scene(session)
    try:
        guides = scene.render_guides(session.camera, session.params)
    finally:
        scene.close()
    w, h = session.params.width, session.params.height
    ids = guides["obj_id"]
    px, py = w // 2, 3 * h // 4
    assert ids[py, px] > 0
    sky_y, sky_x = (int(v[0]) for v in np.nonzero(ids < 0))
    base = [exe, "-c", config, "-s", scene_yml, "--image-action", "none", "--seed", "1"]
    hit = subprocess.run(base + ["--pick", "%d,%d" % (px, py)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert hit.returncode == 0, hit.stderr
    words = hit.stdout.split()
    assert words[:3] == ["pick", str(px), str(py)] and len(words) == 12, hit.stdout
    prim, obj_id = int(words[3]), int(words[4])
    t, point, normal = float(words[5]), np.array(words[6:9], dtype=float), np.array(words[9:12], dtype=float)
    # the host layer numbers objects with a counter that runs through the whole process (scene.rs:51,60), and the CLI is a
    # process of its own whose counter starts at 1: the ids are compared as offsets from the scene's first object
    first = session.desc.primitives[0].obj_id
    assert session.desc.primitives[prim].obj_id == ids[py, px]
    assert obj_id - 1 == ids[py, px] - first
    want_t = guides["footprint"][py, px] * (h - 1) / math.sqrt(sum(x * x for x in session.camera.vertical[:]))
    assert within(np.array(t), np.array(want_t)).all()
    assert within(point, guides["position"][py, px]).all()
    assert within(normal, guides["normal"][py, px]).all()
    sky = subprocess.run(base + ["--pick=%d,%d" % (sky_x, sky_y)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert sky.returncode == 0, sky.stderr
    assert sky.stdout.split() == ["pick", str(sky_x), str(sky_y), "miss"]
    for bad in ("%d,%d" % (w, 0), "%d,%d" % (0, h), "3", "3,", "a,b", "-1,2"):      # refused like the other flags' bad values
        r = subprocess.run(base + ["--pick", bad], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode != 0 and r.stdout == "" and "--pick" in r.stderr, (bad, r.stderr)
