"""The multi-hit query (include/rt_multihit.h) on the GPU: against tests/multihit_model.py on every scene
form, the stack scenes and both arithmetic flavours; against the device's own closest query; the prefix property between
two k; order and shape; the slot-major layout and what the binding refuses; windows; invalid rays; the host form across a
chunk boundary; queries next to renders of a tree that is re-ordered per camera; the CLI flag.

Tolerance: 1e-9 max(1, |want|), the bound of every comparison with the oracle's records (tests/test_gpu_rays.py: BOUND).
A TIED ray is multihit_model.tied's: on it only count and the sorted t are compared, which do not depend on who wins."""
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import multihit_model as M
import multihit_scenes as MS
import ray_query_model as Q
import scenes_py as S

pytestmark = pytest.mark.gpu
abi = Q.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-9
KS = (1, 2, 3, 4, 5, 8)
TREE = "form-2-0-0-1"      # a tree (staged in LDS by renders) with moving and wrapped primitives
FLAVOURS = {"fast": {}, "exact": dict(arithmetic=abi.RT_ARITH_REFERENCE)}
F64 = ("t", "point", "normal", "uv")
I32 = ("prim", "obj_id", "front_face")


@pytest.fixture(scope="module")
def mh():
    return importlib.import_module("racer-tracer_amd.multihit")


@pytest.fixture(scope="module")
def rays():
    return importlib.import_module("racer-tracer_amd.rays")


@pytest.fixture(scope="module")
def sets(orc):
    """(scene name, set name) -> multihit_scenes.ray_set; computed once, never written to."""
    cache = {}

    def get(name, which):
        if (name, which) not in cache:
            cache[name, which] = MS.ray_set(orc, name, which)
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


def multi(mh, scene, o, d, k, t_min=None, t_max=None, time=None, **kw):
    """trace_rays_multi_torch on numpy rays -> numpy planes."""
    import torch
    got = mh.trace_rays_multi_torch(scene, up(scene, o), up(scene, d), k, up(scene, t_min), up(scene, t_max), up(scene, time), **kw)
    torch.cuda.synchronize(torch.device("cuda", scene.device))
    return {name: v.cpu().numpy() for name, v in got.items()}


def closest(rays, scene, o, d, t_min=None, t_max=None, time=None, planes=("t", "prim")):
    import torch
    got = rays.trace_rays_torch(scene, up(scene, o), up(scene, d), up(scene, t_min), up(scene, t_max), up(scene, time), planes=planes)
    torch.cuda.synchronize(torch.device("cuda", scene.device))
    return {name: v.cpu().numpy() for name, v in got.items()}


def within(got, want):
    """|got - want| <= BOUND max(1, |want|); inf answers inf, a NaN a NaN (a MovingSphere's v, tests/test_gpu_rays.py)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(got - want) <= BOUND * np.maximum(1.0, np.abs(want))) | (got == want) | (np.isnan(got) & np.isnan(want))


def same(a, b):
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def bits_differ(a, b):
    return (a.view(np.int64) != b.view(np.int64)).sum()


def assert_against_model(got, want, tied, what):
    """count and the whole t plane on EVERY ray; the other planes on every ray that is not tied; unfilled slots and misses
    bit for bit."""
    assert same(got["count"], want["count"]), (what, np.nonzero(got["count"] != want["count"])[0][:8])
    assert within(got["t"], want["t"]).all(), (what, "t")
    free = ~tied
    for plane in I32:
        assert same(got[plane][:, free], want[plane][:, free]), (what, plane)
    for plane in ("point", "normal", "uv"):
        assert within(got[plane][:, free], want[plane][:, free]).all(), (what, plane)
    unfilled = want["prim"] < 0      # (k, n): given the count, the same slots in every answer, tied or not
    for plane in F64 + I32:
        assert same(got[plane][unfilled], want[plane][unfilled]), (what, plane, "unfilled")


def assert_order_and_shape(got, k, n, what):
    assert got["count"].shape == (n,) and got["t"].shape == (k, n) and got["point"].shape == (k, n, 3)
    assert (got["count"] <= k).all() and (got["count"] >= 0).all(), what
    assert (got["t"][1:] >= got["t"][:-1]).all(), what      # t does not decrease over the slots (inf behind the filled ones)
    filled = got["prim"] >= 0
    assert same(filled.sum(axis=0).astype(np.int32), got["count"]), what
    assert same(filled, np.arange(k)[:, None] < got["count"][None, :]), what      # the filled slots come first
    for j in range(k):
        for i in range(j + 1, k):
            both = filled[j] & filled[i]
            assert (got["prim"][j][both] != got["prim"][i][both]).all(), (what, "one primitive in two slots")


# ---- the rule: against the model, the closest query, and between two k -----------------------------------------------------------

@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("name", MS.ALL_SCENES)
def test_first_k_hits_match_model_and_closest_query(rt, mh, rays, gpu, sets, name, flavour):
    scene = open_scene(rt, sets(name, MS.sets_of(name)[0]), **FLAVOURS[flavour])
    try:
        for which in MS.sets_of(name):
            check_set(mh, rays, scene, sets(name, which), name, flavour, which)
    finally:
        scene.close()


def check_set(mh, rays, scene, s, name, flavour, which):
    o, d, time, lists = s["origin"], s["direction"], s["time"], s["lists"]
    n = len(o)
    near = closest(rays, scene, o, d, time=time)
    answers = {k: multi(mh, scene, o, d, k, time=time) for k in KS}
    for k in KS:
        got, what = answers[k], (name, flavour, which, k)
        tied = M.tied(lists, k)
        assert_order_and_shape(got, k, n, what)
        assert_against_model(got, M.expected(lists, k), tied, what)
        # slot 0 is the device's own closest answer: the same t — in the reference flavour, which contracts nothing,
        # bit for bit on every ray — and the same primitive where there is no tie
        differ = bits_differ(got["t"][0], near["t"])
        print("%s %s set %s k = %d: %d filled slots, %d tied rays, slot 0 differs from the closest query's t in bits on %d rays"
              % (name, flavour, which, k, (got["prim"] >= 0).sum(), tied.sum(), differ))
        if flavour == "exact":
            assert differ == 0, what
        assert within(got["t"][0], near["t"]).all(), what
        assert same(got["prim"][0][~tied], near["prim"][~tied]), what
    # the prefix property: the answer to k is the head of the answer to k' > k — the walk whose far end has come in
    # against the one whose far end has not (yet).  Two instantiations answer k <= 4 and k > 4: bit for bit in the
    # reference flavour, within the bound in the fast one, whose contractions belong to the instantiation
    for k in KS:
        for k2 in KS:
            if k2 <= k:
                continue
            a, b = answers[k], answers[k2]
            free = ~(M.tied(lists, k) | M.tied(lists, k2))
            assert same(a["count"], np.minimum(b["count"], k)), (name, which, k, k2)
            for plane in I32:
                assert same(a[plane][:, free], b[plane][:k][:, free]), (name, which, k, k2, plane)
            for plane in F64:
                if flavour == "exact":
                    assert same(a[plane][:, free], b[plane][:k][:, free]), (name, which, k, k2, plane)
                assert within(a[plane][:, free], b[plane][:k][:, free]).all(), (name, which, k, k2, plane)


# ---- layout ----------------------------------------------------------------------------------------------------------------------
SENTINEL = -777


@pytest.mark.parametrize("name", ["three_balls", TREE])
def test_slot_major_layout_null_planes_and_refusals(rt, mh, gpu, name):
    import torch
    bundle, cam, spread, closest_hit, in_lds = Q.scene(name)
    o, d, time = Q.random_rays(cam, 1000, spread)
    scene = open_scene(rt, dict(bundle=bundle, closest_hit=closest_hit, in_lds=in_lds))
    dev = torch.device("cuda", scene.device)
    widths = {p: mh.HIT_PLANES[p][0] for p in mh.HIT_PLANES}
    try:
        to, td, tt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (o, d, time))
        for k in (3, 8):
            full = multi(mh, scene, o, d, k, time=time)      # n = 1000: the reference of every shorter batch
            assert (full["count"] > 0).sum() > 300 and (full["count"] > 1).sum() > 20
            for n in (1, 63, 65, 257, 1000):
                out = {p: torch.full((k * n * w + 64 * w,), SENTINEL, dtype=torch.float64 if mh.HIT_PLANES[p][1] else torch.int32,
                                     device=dev) for p, w in widths.items()}
                out["count"] = torch.full((n + 64,), SENTINEL, dtype=torch.int32, device=dev)
                got = mh.trace_rays_multi_torch(scene, to[:n].contiguous(), td[:n].contiguous(), k, time=tt[:n].contiguous(), out=out)
                torch.cuda.synchronize(dev)
                for p, w in widths.items():
                    assert got[p] is out[p]
                    flat = out[p].cpu().numpy()
                    for j in range(k):      # plane j starts at entry j * n
                        assert same(flat[w * j * n:w * (j + 1) * n], full[p][j, :n].reshape(-1)), (p, k, n, j)
                    assert (flat[w * k * n:] == SENTINEL).all() and flat[w * k * n:].size == 64 * w, (p, k, n)
                count = out["count"].cpu().numpy()
                assert same(count[:n], full["count"][:n]) and (count[n:] == SENTINEL).all()
            # NULL planes and a NULL count: what is asked for is what the full call gives
            for planes in (("t",), ("prim", "uv"), ()):
                for want_count in (True, False):
                    part = multi(mh, scene, o, d, k, time=time, planes=planes, count=want_count)
                    assert sorted(part) == sorted(planes + (("count",) if want_count else ()))
                    for p in part:
                        assert same(part[p], full[p]), (p, planes)
        # n == 0: RT_OK, nothing launched
        none = mh.trace_rays_multi_torch(scene, to[:0].contiguous(), td[:0].contiguous(), 4)
        assert none["t"].shape == (4, 0) and none["point"].shape == (4, 0, 3) and none["count"].shape == (0,)
        host_none = mh.trace_rays_multi(scene, o[:0], d[:0], 4)
        assert host_none["t"].shape == (4, 0) and host_none["count"].shape == (0,)
        # what the binding refuses: another dtype, a view that is not contiguous, host memory, too small an output, a bad k
        with pytest.raises(ValueError):
            mh.trace_rays_multi_torch(scene, to.float(), td, 4)
        with pytest.raises(ValueError):
            mh.trace_rays_multi_torch(scene, to[::2], td[::2], 4)
        with pytest.raises(ValueError):
            mh.trace_rays_multi_torch(scene, to.cpu(), td.cpu(), 4)
        with pytest.raises(ValueError):
            mh.trace_rays_multi_torch(scene, to, td, 4, time=tt[:999])
        with pytest.raises(ValueError):
            mh.trace_rays_multi_torch(scene, to, td, 4, out={"t": torch.zeros(4 * 1000 - 1, dtype=torch.float64, device=dev)})
        with pytest.raises(ValueError):
            mh.trace_rays_multi_torch(scene, to, td, 4, out={"prim": torch.zeros(4 * 1000, dtype=torch.int64, device=dev)})
        with pytest.raises(ValueError):
            mh.trace_rays_multi_torch(scene, to, td, 4, out={"count": torch.zeros(1000, dtype=torch.int32)})
        with pytest.raises(ValueError):
            mh.trace_rays_multi(scene, o, d[:999], 4)
        for bad in (0, 9, -1):
            with pytest.raises(rt.RtError) as e:
                mh.trace_rays_multi_torch(scene, to, td, bad)
            assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
            with pytest.raises(rt.RtError):
                mh.trace_rays_multi(scene, o, d, bad)
    finally:
        scene.close()


# ---- windows ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three_balls", TREE, "stack", "stack-wrapped"])
def test_windows(rt, orc, mh, gpu, sets, name):
    s = sets(name, MS.sets_of(name)[-1])      # the pair set, or the stack's
    o, d, time = s["origin"], s["direction"], s["time"]
    n, k = len(o), 4
    scene = open_scene(rt, s)
    try:
        base = multi(mh, scene, o, d, k, time=time)
        two = base["count"] >= 2
        assert two.mean() > 0.3
        # the device's own slot-1 t as the far end: inclusive, so at least two hits, and slots 0 and 1 as they were
        t1 = np.where(two, base["t"][1], np.inf)
        at = multi(mh, scene, o, d, k, t_max=t1, time=time)
        assert (at["count"][two] >= 2).all() and same(at["count"][~two], base["count"][~two])
        for plane in F64 + I32:
            assert same(at[plane][:2], base[plane][:2]), plane
        # ... and just below it: what the model finds inside the shorter window
        below = t1 * (1.0 - 1e-6)
        got = multi(mh, scene, o, d, k, t_max=below, time=time)
        lists = M.hit_lists(orc, s["bundle"], o, d, t_max=below, time=time)
        want = M.expected(lists, k)
        print("%s: t_max just below slot 1: counts %s, were %s" % (name, np.bincount(got["count"], minlength=k + 1).tolist(),
                                                                     np.bincount(base["count"], minlength=k + 1).tolist()))
        assert_against_model(got, want, M.tied(lists, k), (name, "below"))
        assert (got["count"][two] < base["count"][two]).all()
        # the near end is inclusive too: t_min = the device's own slot-0 t changes nothing (a sphere in front of it whose
        # near root it cut off would have been slot 0 itself)
        t0 = np.where(base["count"] >= 1, base["t"][0], Q.T_MIN)
        near = multi(mh, scene, o, d, k, t_min=t0, time=time)
        for plane in base:
            assert same(near[plane], base[plane]), plane
        # t_min = t_max = 0 is a valid window that holds no hit
        zero = multi(mh, scene, o, d, k, t_min=np.zeros(n), t_max=np.zeros(n), time=time)
        assert (zero["count"] == 0).all() and (zero["prim"] == Q.MISS).all() and np.isinf(zero["t"]).all()
    finally:
        scene.close()


# ---- invalid rays ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["three_balls", TREE])
def test_invalid_rays_are_marked_in_their_lane(rt, mh, gpu, name):
    bundle, cam, spread, closest_hit, in_lds = Q.scene(name)
    nan, inf = math.nan, math.inf
    kinds = [("origin", 0, nan), ("origin", 1, inf), ("origin", 2, -inf), ("direction", 0, nan), ("direction", 1, inf),
             ("direction", 2, -inf), ("time", None, nan), ("time", None, inf), ("t_min", None, nan), ("t_min", None, inf),
             ("t_min", None, -1e-3), ("t_max", None, nan), ("t_max", None, 0.5e-3), ("zero", None, 0.0)]
    n, k = 2 * len(kinds) + 70, 3      # more than one wave; invalid rays at the odd places of the first 2 len(kinds)
    o, d, time = Q.random_rays(cam, n, spread)
    clean = dict(origin=o, direction=d, t_min=np.full(n, Q.T_MIN), t_max=np.full(n, inf), time=time)
    dirty = {key: v.copy() for key, v in clean.items()}
    bad = np.zeros(n, dtype=bool)
    for q, (plane, axis, value) in enumerate(kinds):
        i = 2 * q + 1
        bad[i] = True
        if plane == "zero":
            dirty["direction"][i] = 0.0
        elif axis is None:
            dirty[plane][i] = value
        else:
            dirty[plane][i, axis] = value
    scene = open_scene(rt, dict(bundle=bundle, closest_hit=closest_hit, in_lds=in_lds))
    try:
        want = multi(mh, scene, clean["origin"], clean["direction"], k, clean["t_min"], clean["t_max"], clean["time"])
        got = multi(mh, scene, dirty["origin"], dirty["direction"], k, dirty["t_min"], dirty["t_max"], dirty["time"])
        host = mh.trace_rays_multi(scene, dirty["origin"], dirty["direction"], k, dirty["t_min"], dirty["t_max"], dirty["time"])
    finally:
        scene.close()
    assert (want["count"] >= 0).all() and (want["count"] > 0).sum() > n // 4
    assert (got["count"][bad] == mh.RT_RAY_INVALID).all() and (got["prim"][:, bad] == mh.RT_RAY_INVALID).all()
    model = M.expected([None] * int(bad.sum()), k)      # a miss's values elsewhere
    for plane in F64 + I32:
        assert same(got[plane][:, bad], model[plane]), plane
        assert same(got[plane][:, ~bad], want[plane][:, ~bad]), plane
        assert same(host[plane], got[plane]), plane
    assert same(got["count"][~bad], want["count"][~bad]) and same(host["count"], got["count"])


# ---- the host form ---------------------------------------------------------------------------------------------------------------

def test_host_form_equals_device_form_across_a_chunk(rt, mh, gpu):
    """k = 8 on the deep scene, one ray more than a staging chunk holds: every slot of every plane lands at j * n + r."""
    bundle, closest_hit, in_lds = MS.stack_scene("stack")
    n, k = mh.RT_MULTIHIT_HOST_CHUNK + 1, 8
    o, d, time = MS.stack_rays(n)
    scene = open_scene(rt, dict(bundle=bundle, closest_hit=closest_hit, in_lds=in_lds))
    try:
        dev = multi(mh, scene, o, d, k, time=time)
        host = mh.trace_rays_multi(scene, o, d, k, time=time)
        part_dev = multi(mh, scene, o, d, 3, planes=("t", "obj_id"))
        part_host = mh.trace_rays_multi(scene, o, d, 3, planes=("t", "obj_id"))      # no optional plane: none staged
    finally:
        scene.close()
    assert (dev["count"] == 8).mean() > 0.5 and (dev["count"] < 4).mean() > 0.05
    assert (dev["count"][-1] > 0) and sorted(host) == sorted(dev)
    for plane in dev:
        assert host[plane].dtype == dev[plane].dtype and same(host[plane], dev[plane]), plane
    for plane in part_dev:
        assert same(part_host[plane], part_dev[plane]), plane


# ---- a tree that renders re-order for their camera -------------------------------------------------------------------------------

def test_queries_and_renders_of_a_reordered_tree_leave_each_other_alone(rt, mh, gpu, sets):
    s = sets(TREE, "pair")
    assert not M.tied(s["lists"], 4).any()      # (no tie: the answer is the same in every child order)
    cam = Q.scene(TREE)[1]
    p = abi.render_params(64, 36, 8)
    camera = S.camera_for(cam, p.width, p.height)
    other = S.camera_for(dict(cam, look_from=tuple(-x for x in cam["look_from"])), p.width, p.height)
    ask = lambda scene: multi(mh, scene, s["origin"], s["direction"], 4, time=s["time"])      # noqa: E731
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
    assert (a["count"] > 2).mean() > 0.3
    for plane in a:
        assert same(a[plane], b[plane]) and same(a[plane], c[plane]), plane
    for got, want in zip((frame_a, frame_b, frame_c), frames):
        assert np.array_equal(got, want, equal_nan=True)
    assert not np.array_equal(frame_a, frame_b)


# ---- CLI -------------------------------------------------------------------------------------------------------------------------

def test_cli_pick_through_prints_one_line_per_slot(rt, host, gpu):
    """--pick-through X,Y[,K] on three_balls.yml next to --pick X,Y of the same pixel: slot 0 is the picked primitive (t,
    point and normal within the bound: two kernels in the fast flavour), the slots are numbered and ascend in t, K
    defaults to 4, and a sky pixel prints `miss`."""
    exe = os.path.join(ROOT, "racer-tracer_amd", "bin", "racer-tracer-amd")
    config, scene_yml = os.path.join(ROOT, "scenes", "config_c1.yml"), os.path.join(ROOT, "scenes", "three_balls.yml")
    session = host.Session(config, scene=scene_yml)
    scene = rt.Scene(session)
    try:
        ids = scene.render_guides(session.camera, session.params)["obj_id"]
    finally:
        scene.close()
    w, h = session.params.width, session.params.height
    px, py = w // 2, 3 * h // 4
    assert ids[py, px] > 0
    sky_y, sky_x = (int(v[0]) for v in np.nonzero(ids < 0))
    base = [exe, "-c", config, "-s", scene_yml, "--image-action", "none", "--seed", "1"]
    run = subprocess.run(base + ["--pick", "%d,%d" % (px, py), "--pick-through", "%d,%d" % (px, py)], capture_output=True, text=True,
                         cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stderr
    lines = [line.split() for line in run.stdout.splitlines()]
    pick, through = lines[0], lines[1:]
    assert pick[:3] == ["pick", str(px), str(py)] and len(pick) == 12, run.stdout
    assert 1 <= len(through) <= 4
    ts, prims, objs = [], [], []
    for j, words in enumerate(through):
        assert len(words) == 13 and words[:4] == ["pick-through", str(px), str(py), str(j)], run.stdout
        prims.append(int(words[4]))
        ts.append(float(words[6]))
        objs.append(int(words[5]))
        normal = np.array(words[10:13], dtype=float)
        assert abs(np.linalg.norm(normal) - 1.0) < 1e-9
    assert through[0][4:6] == pick[3:5]
    assert within(np.array(through[0][6:], dtype=float), np.array(pick[5:], dtype=float)).all()
    assert ts == sorted(ts) and len(set(prims)) == len(prims) and len(set(objs)) == len(objs)
    assert all(0 <= q < session.desc.n_primitives for q in prims)
    one = subprocess.run(base + ["--pick-through=%d,%d,1" % (px, py)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert one.returncode == 0 and one.stdout.splitlines() == [" ".join(through[0])], one.stdout
    sky = subprocess.run(base + ["--pick-through", "%d,%d,8" % (sky_x, sky_y)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert sky.returncode == 0, sky.stderr
    assert sky.stdout.split() == ["pick-through", str(sky_x), str(sky_y), "miss"]
    for bad in ("%d,%d" % (w, 0), "%d,%d" % (0, h), "3", "3,", "a,b", "-1,2", "1,2,0", "1,2,9", "1,2,3,4", "1,2,", ""):
        r = subprocess.run(base + ["--pick-through", bad], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode != 0 and r.stdout == "" and "--pick-through" in r.stderr, (bad, r.stderr)
