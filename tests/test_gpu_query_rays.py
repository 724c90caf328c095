"""The three ray queries (include/rt_rays.h, rt_occlusion.h, rt_multihit.h) on the GPU, on the rays a
caller sends and a camera never makes (tests/query_ray_sets.py): directions of any scale, exactly zero components, origins
outside the scene's box with windows that end before it or begin behind it.  Every scene form — the linear loop, the tree
staged in LDS by renders, the tree in global memory — both arithmetic flavours, RT_RAYS_CLOSEST with all planes, occlusion,
and multi-hit at k = 1, 4, 8; one scene object per case.

The rule against the models (tests/ray_query_model.py, tests/multihit_model.py) is the one of tests/test_gpu_rays.py and
tests/test_gpu_multihit.py: prim and count equal on every ray that is not TIED (multihit_model.tied), records within
1e-9 max(1, |want|), misses and unfilled slots bit for bit.  No ray is excused beyond the ties, with one thing the
reference itself does (tests/query_ray_sets.py, held on the CPU by tests/test_query_rays_cpu.py): a ray EXACTLY in a
rect's plane makes the reference's plane test 0 / 0, its answer NaN and the primitive it names a matter of visiting order.
Such a DEGENERATE ray occurs among the Z family's in-plane rays only (none in S or O: asserted); it is sent through
every query and must come back well-formed, no more.

One bound is widened, as the issue provides for far origins.  At f = 256 (the four sphere forms) the fast flavour missed
1e-9 max(1, |want|) in the point by a factor of 3.3, in the normal by 5.5 and in uv by 1.3, while prim, count and t (worst
1.4e-12) agreed; the reference's own t moves by S = 2.1e-10 between the base ray and the pulled-back one there
(query_ray_sets.far_origin_movement).  A t off by dt moves the point o + t d by dt |d|, a sphere's normal by that over its
radius, and its u, v by that over pi sin(theta): on those scenes the fast flavour's point, normal and uv of ray i of
"pulled" and "between" are held to the bound plus these figures at dt = 8 S (query_ray_sets.far_origin_slack).  t, the
reference flavour, and every scene with f = 1 keep the plain bound, as does the whole Z family, whose rays tangent to the
ground sphere (where the reference moves by 5.4e-9) were taken out of the set instead.

S, reference flavour: every plane of every query at every scale equals the same device's answer at e = 0, t 2^e bit for
bit — IEEE operations commute with a power of two, and tests/test_query_rays_cpu.py holds the oracle to the same.
S, fast flavour: against the rescaled model; and, since every direction outside the band of rt_query_ray.h is walked in
its unit form, all scales |e| >= 63 give one answer, bit for bit.
"""
import importlib
import math

import numpy as np
import pytest

import multihit_model as M
import query_ray_sets as R
import ray_query_model as Q

pytestmark = pytest.mark.gpu
abi = Q.abi
BOUND = 1e-9       # tests/test_gpu_rays.py: BOUND
KS = (1, 4, 8)
FLAVOURS = {"fast": {}, "exact": dict(arithmetic=abi.RT_ARITH_REFERENCE)}
F64 = ("t", "point", "normal", "uv")
I32 = ("prim", "obj_id", "front_face")
OUT_OF_BAND = tuple(e for e in R.SCALES if abs(e) >= 63)


@pytest.fixture(scope="module")
def mods():
    return {m: importlib.import_module("racer-tracer_amd." + m) for m in ("rays", "occlusion", "multihit")}


@pytest.fixture(scope="module")
def models(orc):
    """(scene, family) -> the ray sets with the models' answers; computed once, shared by the flavours, never written to."""
    cache = {}

    def with_models(bundle, rays):
        lists = R.hit_lists(orc, bundle, rays)
        n = len(lists)
        want = R.closest_model(orc, bundle, rays)
        return dict(rays=rays, want=want, lists=lists, multi={k: M.expected(lists, k) for k in KS},
                    tied={k: M.tied(lists, k) for k in KS}, degenerate=R.degenerate(lists, bundle, rays) | R.models_disagree(want, lists),
                    slack=None, slack_multi=None)

    def get(name, family):
        if (name, family) not in cache:
            bundle = R.scene(name)[0]
            if family == "S":
                cache[name, family] = with_models(bundle, R.s_base(name))
            elif family == "Z":
                cache[name, family] = with_models(bundle, R.z_family(orc, name))
            else:
                o = R.o_family(orc, name)
                cache[name, family] = dict(o, **{which: with_models(bundle, o[which]) for which in ("pulled", "between")})
                if o["f"] > 1:      # far origins: what dt = 8 S does to the fast flavour's record (the module's docstring)
                    moved = R.far_origin_movement(orc, name, o)
                    for which in ("pulled", "between"):
                        m = cache[name, family][which]
                        m["slack"] = R.far_origin_slack(bundle, m["rays"], m["want"], moved)
                        m["slack_multi"] = {k: R.far_origin_slack(bundle, m["rays"], m["multi"][k], moved) for k in KS}
            if family != "Z":       # the S claim "no ray is excused" holds against the model too
                for m in ([cache[name, family]] if family == "S" else [cache[name, family][w] for w in ("pulled", "between")]):
                    assert not m["degenerate"].any(), (name, family)
        return cache[name, family]
    return get


def open_scene(rt, name, flavour):
    bundle, _cam, _spread, closest_hit, in_lds = R.scene(name)
    scene = rt.Scene(bundle, closest_hit=closest_hit, **FLAVOURS[flavour])
    variant = scene.variant()
    assert variant["use_bvh"] == int(in_lds is not None)
    if in_lds is not None:
        assert variant["bvh_nodes_in_lds"] == in_lds
    assert variant["exact"] == int(flavour == "exact")
    return scene


def ask(mods, scene, rays):
    """All three queries on one ray set -> dict(closest planes, "occluded", "multi": {k: planes + count})."""
    import torch
    dev = torch.device("cuda", scene.device)
    o, d, lo, hi, time = (torch.tensor(rays[p], dtype=torch.float64, device=dev) for p in ("origin", "direction", "t_min", "t_max", "time"))
    out = dict(mods["rays"].trace_rays_torch(scene, o, d, lo, hi, time))
    out["occluded"] = mods["occlusion"].occluded_torch(scene, o, d, lo, hi, time)
    multi = {k: mods["multihit"].trace_rays_multi_torch(scene, o, d, k, lo, hi, time) for k in KS}
    torch.cuda.synchronize(dev)
    out = {p: v.cpu().numpy() for p, v in out.items()}
    out["multi"] = {k: {p: v.cpu().numpy() for p, v in planes.items()} for k, planes in multi.items()}
    return out


def within(got, want, slack=0.0):
    """|got - want| <= BOUND max(1, |want|) + slack; inf answers inf, a NaN a NaN (a MovingSphere's v, tests/test_gpu_rays.py)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(got - want) <= BOUND * np.maximum(1.0, np.abs(want)) + slack) | (got == want) | (np.isnan(got) & np.isnan(want))


def slack_on(slack, plane, rows, ray_axis=0):
    """The additive slack of `plane` (query_ray_sets.far_origin_slack's arrays, or None: nothing) on the rays `rows`."""
    if slack is None or plane not in slack:
        return 0.0
    return np.compress(rows, slack[plane], axis=ray_axis)


def same(a, b):
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64)) if a.dtype.kind == "f" else np.array_equal(a, b)


def worst(got, want):
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    return float(np.nanmax(np.where(np.isfinite(e), e, 0.0))) if e.size else 0.0


def rescaled(ans, e):
    """The answer at scale e with every t times 2^e: what e = 0 reports."""
    up = math.ldexp(1.0, e)
    out = dict(ans, t=ans["t"] * up)
    out["multi"] = {k: dict(planes, t=planes["t"] * up) for k, planes in ans["multi"].items()}
    return out


def assert_identities(ans, m, what):
    """occluded == the closest query reports a hit, on every ray; slot 0 of every k is the closest query's answer.  (Not on
    a degenerate ray: a NaN t is ordered by nobody.)"""
    fine = ~m["degenerate"]
    assert ans["occluded"].dtype == np.int32 and same(ans["occluded"][fine], (ans["prim"][fine] >= 0).astype(np.int32)), what
    for k in KS:
        got = ans["multi"][k]
        assert within(got["t"][0][fine], ans["t"][fine]).all(), (what, k)
        free = fine & ~m["tied"][k]
        assert same(got["prim"][0][free], ans["prim"][free]), (what, k)
        assert same(got["count"][fine] > 0, ans["prim"][fine] >= 0), (what, k)


def assert_well_formed(ans, rows, n_prims, what):
    """What holds of every answer, a degenerate ray's included."""
    assert ((ans["prim"][rows] >= Q.MISS) & (ans["prim"][rows] < n_prims)).all(), what
    assert np.isin(ans["occluded"][rows], (0, 1)).all(), what
    for k in KS:
        got = ans["multi"][k]
        assert ((got["count"][rows] >= 0) & (got["count"][rows] <= k)).all(), (what, k)
        assert ((got["prim"][:, rows] >= Q.MISS) & (got["prim"][:, rows] < n_prims)).all(), (what, k)


def assert_against_models(ans, m, what, n_prims, widened=False):
    want, n = m["want"], len(m["want"]["prim"])
    fine = ~m["degenerate"]
    slack, slack_multi = (m["slack"], m["slack_multi"]) if widened else (None, None)
    assert_well_formed(ans, np.ones(n, dtype=bool), n_prims, what)
    free = fine & ~m["tied"][1]
    hit = free & (want["prim"] >= 0)
    print("%s: %d rays, %d hit, %d tied, %d degenerate, largest slack %s; closest: %d differ in prim, worst %s" %
          (what, n, (want["prim"] >= 0).sum(), m["tied"][8].sum(), m["degenerate"].sum(),
           None if slack is None else {p: "%.2g" % v[hit].max() for p, v in slack.items()}, (ans["prim"][free] != want["prim"][free]).sum(),
           {p: "%.3g" % worst(ans[p][hit], want[p][hit]) for p in F64}))
    assert same(ans["prim"][free], want["prim"][free]), (what, np.nonzero(free & (ans["prim"] != want["prim"]))[0][:8])
    assert same(ans["occluded"][free], (want["prim"][free] >= 0).astype(np.int32)), what
    for plane in F64:
        ok = within(ans[plane][hit], want[plane][hit], slack_on(slack, plane, hit))
        assert ok.all(), (what, plane, worst(ans[plane][hit], want[plane][hit]))
    for plane in ("obj_id", "front_face"):
        assert same(ans[plane][free], want[plane][free]), (what, plane)
    miss = free & (want["prim"] < 0)
    for plane in Q.PLANES:
        assert same_bits(ans[plane][miss], want[plane][miss]), (what, plane, "miss")
    assert within(ans["t"][fine], want["t"][fine]).all(), (what, "t on tied rays")
    for k in KS:      # tests/test_gpu_multihit.py: assert_against_model
        got, model, loose = ans["multi"][k], m["multi"][k], fine & ~m["tied"][k]
        assert got["t"].shape == (k, n) and got["count"].shape == (n,)
        assert same(got["count"][fine], model["count"][fine]), (what, k, np.nonzero(fine & (got["count"] != model["count"]))[0][:8])
        ok = within(got["t"][:, fine], model["t"][:, fine])
        assert ok.all(), (what, k, "t", worst(got["t"][:, fine], model["t"][:, fine]))
        for plane in I32:
            assert same(got[plane][:, loose], model[plane][:, loose]), (what, k, plane)
        for plane in ("point", "normal", "uv"):
            ok = within(got[plane][:, loose], model[plane][:, loose], slack_on(slack_multi and slack_multi[k], plane, loose, 1))
            assert ok.all(), (what, k, plane, worst(got[plane][:, loose], model[plane][:, loose]))
        unfilled = (model["prim"] < 0) & fine[None, :]
        for plane in F64 + I32:
            assert same_bits(got[plane][unfilled], model[plane][unfilled]), (what, k, plane, "unfilled")
    assert_identities(ans, m, what)


def assert_all_miss(ans, n, what):
    """Every query reports a miss on every ray: the planes of a miss bit for bit, count 0, occluded 0."""
    none = Q.empty(n)
    for plane in Q.PLANES:
        assert same_bits(ans[plane], none[plane]), (what, plane, np.nonzero(ans["prim"] != Q.MISS)[0][:8])
    assert ans["occluded"].shape == (n,) and (ans["occluded"] == 0).all(), what
    for k in KS:
        got, none_k = ans["multi"][k], M.empty(k, n)
        for plane in none_k:
            assert same_bits(got[plane], none_k[plane]), (what, k, plane)


def assert_same_answer(a, b, what):
    """Two answers of one device, bit for bit in every plane of every query."""
    for plane in Q.PLANES + ("occluded",):
        assert same_bits(a[plane], b[plane]), (what, plane, int((a["prim"] != b["prim"]).sum()),
                                               np.nonzero(a["prim"] != b["prim"])[0][:8])
    for k in KS:
        for plane in a["multi"][k]:
            assert same_bits(a["multi"][k][plane], b["multi"][k][plane]), (what, k, plane)


# ---- S: scaled directions ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("name", R.SCENES)
def test_scaled_directions(rt, mods, gpu, models, name, flavour):
    m = models(name, "S")
    scene = open_scene(rt, name, flavour)
    n_prims = R.scene(name)[0].desc.n_primitives
    try:
        answers = {e: rescaled(ask(mods, scene, R.scaled(m["rays"], e)), e) for e in R.scales_for(name)}
    finally:
        scene.close()
    unit = answers[0]
    assert 0.2 <= (unit["prim"] >= 0).mean() <= 0.98
    differ = {e: int((answers[e]["prim"] != unit["prim"]).sum()) for e in answers}
    print("%s %s: rays whose closest prim differs from e = 0, per e: %s" % (name, flavour, differ))
    for e, ans in answers.items():
        what = (name, flavour, "S", e)
        if flavour == "exact":
            assert_same_answer(ans, unit, what)
        assert_identities(ans, m, what)
    if flavour == "fast":
        for e, ans in answers.items():
            assert_against_models(ans, m, "%s %s S e = %d" % (name, flavour, e), n_prims)
        for e in OUT_OF_BAND[1:]:      # walked in the unit form, whatever the scale: one answer by construction
            assert_same_answer(answers[e], answers[OUT_OF_BAND[0]], (name, flavour, "S out of band", e))
    else:
        assert_against_models(unit, m, "%s %s S e = 0" % (name, flavour), n_prims)


# ---- Z: zero components ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("name", R.SCENES)
def test_zero_components(rt, mods, gpu, models, name, flavour):
    m = models(name, "Z")
    scene = open_scene(rt, name, flavour)
    n_prims = R.scene(name)[0].desc.n_primitives
    try:
        ans = ask(mods, scene, m["rays"])
    finally:
        scene.close()
    assert_against_models(ans, m, "%s %s Z" % (name, flavour), n_prims)
    kind = m["rays"]["kind"]
    assert (ans["prim"][kind < 2] >= 0).mean() >= 0.9      # aimed at a surface point (tests/test_query_rays_cpu.py)


# ---- O: origins outside the box ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("name", R.SCENES)
def test_origins_outside_the_box(rt, mods, gpu, models, name, flavour):
    o = models(name, "O")
    scene = open_scene(rt, name, flavour)
    n_prims = R.scene(name)[0].desc.n_primitives
    try:
        answers = {which: ask(mods, scene, o[which]["rays"] if which in ("pulled", "between") else o[which])
                   for which in ("pulled", "between", "before", "behind", "beside")}
    finally:
        scene.close()
    for which in ("before", "behind", "beside"):      # no ray excused
        assert_all_miss(answers[which], len(o[which]["origin"]), (name, flavour, which))
    for which in ("pulled", "between"):
        widened = flavour == "fast" and o["f"] > 1
        assert_against_models(answers[which], o[which], "%s %s O %s (f = %d)" % (name, flavour, which, o["f"]), n_prims, widened)
