"""Ray sets of the kinds a caller sends and a camera never makes, for the three ray queries (include/rt_rays.h,
rt_occlusion.h, rt_multihit.h).  A helper, not a test file: tests/test_query_rays_cpu.py checks the
conditions stated here with the oracle alone, tests/test_gpu_query_rays.py compares the device with the models
(tests/ray_query_model.py, tests/multihit_model.py) on the same rays.

The BASE of every family is THE random set (ray_query_model.random_rays, seed 2026) at n = 256, 64 on large_bvh, on the
scenes of ray_query_model.SCENES and on the three stack forms of tests/multihit_scenes.py (seen from STACK_CAM).

  S  scale.  Direction d 2^e, t_min = 0.001 2^-e, a finite t_max times 2^-e, for e in SCALES.  The answer is the one of
     e = 0 with t 2^-e: IEEE add, multiply, divide and sqrt commute with a power of two while nothing under- or
     overflows, and the oracle is held to that bit for bit.  Every fourth base ray carries t_max = S_T_MAX, so that a
     finite far end is scaled too.
  Z  zero components.  Targets: the base set's model hit points.  Axis rays reach each target along +-x, +-y, +-z from
     L away (L the scene's spread; the two other components are +-0, cycling through the four sign pairs); plane rays
     have exactly one zero component; and, on the forms that hold plain rects, 16 rays lie IN a rect's plane
     (o[axis] = k, d[axis] = +-0) and cross its extent.  An axis or plane ray that runs along its target's own flat
     surface (d . normal == 0: in a rect's or a box side's plane) counts as an in-plane ray: it is not aimed AT a
     surface, and the hit share is not asked of it.
     A ray that would meet its target's CURVED surface at 0 < |d . normal| <= GRAZE |d| is NOT IN THE SET: tangent to
     the ground sphere of radius 1000 (|d . n| <= 1.3e-4 |d|: every horizontal axis ray over it) the reference's
     discriminant cancels and its own t moves by up to 5.4e-9 when the same ray is merely started one d earlier, more
     than the comparisons' bound.  On every ray kept, the reference moves by less than an eighth of the bound
     (tests/test_query_rays_cpu.py), and the bound is 1e-9 max(1, |want|) with nothing added.
     What the reference does EXACTLY in a rect's plane (o[axis] == k, d[axis] == +-0): its plane test forms 0 / 0, the
     NaN passes every comparison, the rect reports a hit with t = NaN, and from then on every later candidate is
     accepted — which primitive is named depends on the order the primitives are visited in, and the device visits
     them in its own order.  Such a ray is DEGENERATE (degenerate() below): it is sent, and its answer must be
     well-formed, but there is no expected value to compare with.
  O  outside.  The base ray pulled back to o - f d, f = PULL_BACK[scene], the smallest power of 4 that puts at least 0.9
     of the origins outside the scene's box, with four windows: [0.001 + f, inf) (the base ray's own answer, t + f),
     the default window, a window that ends before the box (t_max = 0.5 t_enter) and one that begins behind it
     (t_min = 2 t_exit).  And 32 rays whose line passes beside the box.
     At f = 256 (the sphere forms, whose ground sphere has radius 1000) the reference's own t differs by up to S = 2.1e-10
     between the base ray and the pulled-back one (far_origin_movement()).  A t that is off by dt moves the point
     o + t d by dp = dt |d|, a sphere's normal (p - c) / r by dp / r, and its u = phi / 2 pi and v = theta / pi by at most
     dn / (pi sin theta): where f > 1, the fast flavour's record on ray i of "pulled" and "between" is held to the bound
     plus those three figures at dt = 8 S (far_origin_slack()).  Nothing else is widened: not t, not the reference
     flavour, not a scene with f = 1, not a primitive that is no plain sphere.
"""
import ctypes as C
import math

import numpy as np

import multihit_model as M
import multihit_scenes as MS
import ray_query_model as Q

abi = Q.abi
SCENES = MS.ALL_SCENES
SCALES = (-300, -130, -80, -65, -63, -24, -1, 0, 1, 24, 63, 65, 80, 130, 300)
DROPPED_SCALES = {}      # scene -> scales the oracle itself does not commute with there (none)
S_T_MAX = 1.25           # the targets lie at t = 1
STACK_CAM = dict(look_from=(0.0, 0.0, 5.0), look_at=MS.CENTRE)
STACK_SPREAD = 12.0
SIGN_PAIRS = ((0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0))
SEED_Z, SEED_O = 2031, 2032
N_IN_PLANE, N_BESIDE = 16, 32
GRAZE = 0.02             # 0 < |d . normal| / |d| <= GRAZE: tangent to a curved target, left out of the Z family
TIE = 1e-9
TIE_CAP = {"cornell_box_boxes": 0.05}      # 0.01 elsewhere
# scene -> f of the O family; tests/test_query_rays_cpu.py holds each to "the smallest power of 4 that ..."
PULL_BACK = {
    "form-0-0-0-0": 1, "form-0-0-1-0": 1, "form-0-1-0-0": 1, "form-0-1-1-0": 1,
    "form-1-0-0-0": 256, "form-1-0-1-0": 256, "form-1-1-0-0": 256, "form-1-1-1-0": 256,
    "form-2-0-0-0": 1, "form-2-0-1-0": 1, "form-2-1-0-0": 1, "form-2-1-1-0": 1,
    "form-2-0-0-1": 1, "form-2-0-1-1": 1, "form-2-1-0-1": 1, "form-2-1-1-1": 1,
    "large_bvh": 1, "three_balls": 1, "cornell_box_boxes": 1, "stack": 1, "stack-tree": 1, "stack-wrapped": 1,
}


def scene(name):
    """-> (numbered bundle, camera dict, spread, closest_hit option, tree in LDS or None: no tree)."""
    if name in MS.STACKS:
        bundle, closest_hit, in_lds = MS.stack_scene(name)
        return bundle, STACK_CAM, STACK_SPREAD, closest_hit, in_lds
    return Q.scene(name)


def scales_for(name):
    return tuple(e for e in SCALES if e not in DROPPED_SCALES.get(name, ()))


def frozen(rays):
    for a in rays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return rays


def ray_dict(o, d, time, t_min=None, t_max=None, **more):
    n = len(o)
    return frozen(dict(origin=np.ascontiguousarray(o, dtype=np.float64), direction=np.ascontiguousarray(d, dtype=np.float64),
                       time=np.ascontiguousarray(time, dtype=np.float64),
                       t_min=np.full(n, Q.T_MIN) if t_min is None else np.ascontiguousarray(t_min, dtype=np.float64),
                       t_max=np.full(n, np.inf) if t_max is None else np.ascontiguousarray(t_max, dtype=np.float64), **more))


def base(name):
    """THE random set on the scene, the default window."""
    _bundle, cam, spread, _c, _l = scene(name)
    o, d, time = Q.random_rays(cam, MS.n_for(name), spread)
    return ray_dict(o, d, time)


# ---- S ---------------------------------------------------------------------------------------------------------------------------

def s_base(name):
    """The base set with t_max = S_T_MAX on every fourth ray."""
    b = base(name)
    t_max = np.where(np.arange(len(b["origin"])) % 4 == 3, S_T_MAX, np.inf)
    return ray_dict(b["origin"], b["direction"], b["time"], t_max=t_max)


def scaled(rays, e):
    """The same rays with the direction in units 2^e times as long.  Every product is exact."""
    up, down = math.ldexp(1.0, e), math.ldexp(1.0, -e)
    return ray_dict(rays["origin"], rays["direction"] * up, rays["time"], rays["t_min"] * down, rays["t_max"] * down)


# ---- the scene's box ---------------------------------------------------------------------------------------------------------------

def scene_box(orc, bundle):
    """The union of the description's primitive boxes (the oracle's own, orc_primitive_aabb) -> (mn [3], mx [3])."""
    lib = orc.lib()
    mn, mx = np.full(3, np.inf), np.full(3, -np.inf)
    a, b = abi.D3(), abi.D3()
    for i in range(bundle.desc.n_primitives):
        lib.orc_primitive_aabb(C.byref(bundle.primitives[i]), a, b)
        mn, mx = np.minimum(mn, a[:]), np.maximum(mx, b[:])
    return mn, mx


def slab_interval(mn, mx, o, d):
    """The parameter interval of the LINE o + t d inside the box, in f64 -> (t_enter [n], t_exit [n]); t_enter > t_exit: the line
    passes beside the box.  (A zero component: +-inf or, ON a slab's plane, NaN, which fmax / fmin drop.)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = (mn - o) / d, (mx - o) / d
    return np.fmax.reduce(np.fmin(a, b), axis=1), np.fmin.reduce(np.fmax(a, b), axis=1)


def outside(mn, mx, p):
    return ((p < mn) | (p > mx)).any(axis=1)


# ---- Z ---------------------------------------------------------------------------------------------------------------------------

def plain_rects(bundle):
    """[(axis, a-axis, b-axis, a0, a1, b0, b1, k)] of the description's rects that stand in no wrapper."""
    out = []
    for i in range(bundle.desc.n_primitives):
        p = bundle.primitives[i]
        if p.flags == 0 and p.kind in (abi.RT_PRIM_XY_RECT, abi.RT_PRIM_XZ_RECT, abi.RT_PRIM_YZ_RECT):
            axis = {abi.RT_PRIM_XY_RECT: 2, abi.RT_PRIM_XZ_RECT: 1, abi.RT_PRIM_YZ_RECT: 0}[p.kind]
            ia, ib = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
            out.append((axis, ia, ib, p.p[0], p.p[1], p.p[2], p.p[3], p.p[4]))
    return out


def z_family(orc, name):
    """-> rays with `kind` [n]: 0 axis, 1 plane, 2 in-plane — the 16 laid into a rect's plane, and every axis or plane ray
    whose direction is exactly perpendicular to the model's normal at its target (it runs ALONG a rect or a box side, which
    it then cannot hit); rays tangent to a curved target within GRAZE are left out; `axis_dir` [n]: 0..5 = +x -x +y -y +z -z on a ray along an axis, else -1; `pair` [n]: its index into
    SIGN_PAIRS, else -1."""
    bundle, _cam, spread, _c, _l = scene(name)
    b = base(name)
    want = Q.expected(orc, bundle, b["origin"], b["direction"], time=b["time"])
    hit = want["prim"] >= 0
    targets, times, normals = want["point"][hit], b["time"][hit], want["normal"][hit]
    rng = np.random.default_rng(SEED_Z)
    L = float(spread)
    o, d, time, kind, axis_dir, pair = [], [], [], [], [], []
    for j, (p, tm, nrm) in enumerate(zip(targets, times, normals)):
        for a in range(6):
            axis, sign = a // 2, (1.0 if a % 2 == 0 else -1.0)
            q = (j + a) % 4
            dv = np.zeros(3)
            dv[[x for x in range(3) if x != axis]] = SIGN_PAIRS[q]
            dv[axis] = sign * L
            ov = p.copy()
            ov[axis] = p[axis] - sign * L
            if 0.0 < abs(nrm[axis]) <= GRAZE:      # tangent to a curved target: the reference itself is not steady there
                continue
            # (along its target's own flat surface the ray is no longer aimed AT the surface: an in-plane ray)
            o.append(ov), d.append(dv), time.append(tm), kind.append(2 if nrm[axis] == 0.0 else 0), axis_dir.append(a), pair.append(q)
        # one zero component: the direction lies in a coordinate plane
        zero = j % 3
        phi = rng.uniform(0.0, 2.0 * math.pi)
        dv = np.zeros(3)
        dv[[x for x in range(3) if x != zero]] = (L * math.cos(phi), L * math.sin(phi))
        dv[zero] = 0.0 if j % 2 == 0 else -0.0
        along = abs(float(np.dot(dv, nrm)))
        if 0.0 < along <= GRAZE * L:
            continue
        o.append(p - dv), d.append(dv), time.append(tm), kind.append(2 if along == 0.0 else 1), axis_dir.append(-1), pair.append(-1)
    rects = plain_rects(bundle)
    if rects:
        for j in range(N_IN_PLANE):
            axis, ia, ib, a0, a1, b0, b1, k = rects[j % len(rects)]
            ov, dv = np.zeros(3), np.zeros(3)
            ov[axis], dv[axis] = k, (0.0 if j % 2 == 0 else -0.0)
            ov[ia], dv[ia] = a0 - 0.5 * (a1 - a0), 2.0 * (a1 - a0)      # from before the extent to behind it
            ov[ib], dv[ib] = b0 + rng.uniform(0.2, 0.8) * (b1 - b0), rng.uniform(-0.1, 0.1) * (b1 - b0)
            if j % 4 >= 2:
                ov[ia], dv[ia] = a1 + 0.5 * (a1 - a0), -2.0 * (a1 - a0)
            o.append(ov), d.append(dv), time.append(rng.uniform(0, 1)), kind.append(2), axis_dir.append(-1), pair.append(-1)
    return ray_dict(np.array(o), np.array(d), np.array(time), kind=np.array(kind), axis_dir=np.array(axis_dir), pair=np.array(pair))


# ---- O ---------------------------------------------------------------------------------------------------------------------------

def pull_back_factor(mn, mx, b):
    """The smallest power of 4 that puts at least 0.9 of the base origins, pulled back by it along d, outside the box."""
    f = 1
    while outside(mn, mx, b["origin"] - f * b["direction"]).mean() < 0.9:
        f *= 4
        assert f <= 4 ** 12
    return f


def o_family(orc, name):
    """-> dict of ray sets: "pulled" (window [0.001 + f, inf)), "between" (the default window), "before" and "behind" (the
    rays of "pulled" whose line crosses the box in front of an origin outside it; misses), "beside" (misses), plus
    "f" and "crossing" (bool [n]: the rays "before" and "behind" hold)."""
    bundle, _cam, _spread, _c, _l = scene(name)
    mn, mx = scene_box(orc, bundle)
    b = base(name)
    f = float(PULL_BACK[name])
    n = len(b["origin"])
    o = b["origin"] - f * b["direction"]
    d, time = b["direction"], b["time"]
    t_enter, t_exit = slab_interval(mn, mx, o, d)
    crossing = outside(mn, mx, o) & (t_enter > 2.0 * Q.T_MIN) & (t_enter <= t_exit) & np.isfinite(t_exit)
    c = np.nonzero(crossing)[0]
    rng = np.random.default_rng(SEED_O)
    ext = mx - mn
    bo, bd = [], []
    while len(bo) < N_BESIDE:      # drawn around the box, kept when the whole LINE misses it (the slab test in f64)
        ov = mn + rng.uniform(-1.0, 2.0, 3) * ext
        dv = rng.uniform(-1.0, 1.0, 3) * ext
        lo, hi = slab_interval(mn, mx, ov[None, :], dv[None, :])
        if lo[0] > hi[0] and outside(mn, mx, ov[None, :])[0]:
            bo.append(ov), bd.append(dv)
    return {
        "f": f, "crossing": crossing, "box": (mn, mx),
        "pulled": ray_dict(o, d, time, t_min=np.full(n, Q.T_MIN + f)),
        "between": ray_dict(o, d, time),
        "before": ray_dict(o[c], d[c], time[c], t_max=0.5 * t_enter[c]),
        "behind": ray_dict(o[c], d[c], time[c], t_min=2.0 * t_exit[c]),
        "beside": ray_dict(np.array(bo), np.array(bd), rng.uniform(0, 1, N_BESIDE)),
    }


# ---- the models on a set ---------------------------------------------------------------------------------------------------------

def closest_model(orc, bundle, rays):
    return Q.expected(orc, bundle, rays["origin"], rays["direction"], rays["t_min"], rays["t_max"], rays["time"])


def hit_lists(orc, bundle, rays):
    return M.hit_lists(orc, bundle, rays["origin"], rays["direction"], rays["t_min"], rays["t_max"], rays["time"])


def tied_closest(orc, bundle, rays, want):
    """bool [n]: ray_query_model.tie_margins (the default window's, as that helper has it) below TIE max(1, t)."""
    margins = Q.tie_margins(orc, bundle, rays["origin"], rays["direction"], rays["time"], want)
    return margins < TIE * np.maximum(1.0, np.where(np.isfinite(want["t"]), np.abs(want["t"]), 1.0))


# ---- the reference's own conditioning ------------------------------------------------------------------------------------------------

def degenerate(lists, bundle=None, rays=None):
    """bool [n]: the model's hit list holds a NaN t (the reference's 0 / 0 on a ray exactly in a rect's plane) — or, given
    the scene and the rays, the ray lies exactly in the plane of a rect or of a box's side (a box is six rects to the
    reference, and a side's NaN is forgotten behind a later side's finite t, with the wrong side named).  Inside a RotateY
    the ray's x and z are products: a vertical ray within TIE max(1, |k|) of a turned box's side runs along that side as far
    as anyone can tell (cornell_box_boxes: three rays, which the fast flavour's slab test sees beside the box and the
    reference's six rects on it)."""
    out = np.array([bool(found) and any(math.isnan(h[0]) for h in found) for found in lists])
    if bundle is None:
        return out
    o, d = rays["origin"], rays["direction"]
    for i in range(bundle.desc.n_primitives):
        p = bundle.primitives[i]
        shift = np.array(p.translate[:]) if p.flags & abi.RT_PRIM_HAS_TRANSLATE else np.zeros(3)
        turned = bool(p.flags & abi.RT_PRIM_HAS_ROTATE_Y)
        if p.kind == abi.RT_PRIM_BOX:
            planes = [(axis, p.p[axis + 3 * side]) for axis in range(3) for side in range(2)]
        elif p.kind in (abi.RT_PRIM_XY_RECT, abi.RT_PRIM_XZ_RECT, abi.RT_PRIM_YZ_RECT):
            planes = [({abi.RT_PRIM_XY_RECT: 2, abi.RT_PRIM_XZ_RECT: 1, abi.RT_PRIM_YZ_RECT: 0}[p.kind], p.p[4])]
        else:
            continue
        oo, dd = o - shift, d
        if turned:      # rotate_y.rs:39-48, the oracle's own products; these coordinates carry a rounding: within TIE of the plane
            sn, cs = p.rot_sin, p.rot_cos
            oo = np.stack([cs * oo[:, 0] - sn * oo[:, 2], oo[:, 1], sn * oo[:, 0] + cs * oo[:, 2]], axis=1)
            dd = np.stack([cs * d[:, 0] - sn * d[:, 2], d[:, 1], sn * d[:, 0] + cs * d[:, 2]], axis=1)
        for axis, k in planes:
            reach = TIE * max(1.0, abs(k)) if turned and axis != 1 else 0.0
            out |= (dd[:, axis] == 0.0) & (np.abs(oo[:, axis] - k) <= reach)
    return out


def models_disagree(want, lists):
    """bool [n]: the reference's scan (closest_model) and its per-primitive tests (the head of the hit list) name different
    primitives on a ray that is not tied: the scan's shrinking window met a NaN the full window does not.  There is no one
    expected answer on such a ray; tests/test_query_rays_cpu.py caps their number."""
    head = M.expected(lists, 1)
    return ~M.tied(lists, 1) & (head["prim"][0] != want["prim"])


def conditioning(near, far, shift, rows):
    """How far the reference's own answer moves when a ray is started `shift` d earlier with its window moved along:
    `near` and `far` are closest_model()'s planes of the two, -> {plane: max |far - near| over `rows` where both name the
    same primitive} for t (less the shift), point, normal and uv; 0 where there is no such ray."""
    both = rows & (near["prim"] >= 0) & (near["prim"] == far["prim"])
    out = {}
    for plane in ("t", "point", "normal", "uv"):
        delta = np.abs(far[plane][both] - (shift if plane == "t" else 0.0) - near[plane][both])
        delta = delta[np.isfinite(delta)]
        out[plane] = float(delta.max()) if delta.size else 0.0
    return out


def z_conditioning(orc, name, z, want, lists):
    """conditioning() of every Z ray that is not degenerate, against the same ray started one d earlier."""
    bundle = scene(name)[0]
    earlier = ray_dict(z["origin"] - z["direction"], z["direction"], z["time"], t_min=z["t_min"] + 1.0)
    return conditioning(want, closest_model(orc, bundle, earlier), 1.0, ~degenerate(lists, bundle, z))


def far_origin_movement(orc, name, o):
    """S of the O family: max |t_model(o - f d) - f - t_model(o)| over the base set, the reference's own movement in t."""
    bundle = scene(name)[0]
    b = base(name)
    near = closest_model(orc, bundle, b)
    return conditioning(near, closest_model(orc, bundle, o["pulled"]), o["f"], np.ones(len(b["origin"]), dtype=bool))["t"]


def far_origin_slack(bundle, rays, planes, moved):
    """What a t that is off by 8 `moved` does to the record, per entry of the model's `planes` (shape [n] or [k, n] in prim):
    -> {"point", "normal", "uv"}: arrays that broadcast against those planes.  Zero where the entry is no plain sphere.
    (|radius|: the inner surface of a glass shell is a sphere of negative radius.)"""
    radius = np.array([abs(bundle.primitives[j].p[3]) if bundle.primitives[j].kind == abi.RT_PRIM_SPHERE and bundle.primitives[j].flags == 0
                       else np.inf for j in range(bundle.desc.n_primitives)] + [np.inf])      # (the last: a miss, prim < 0)
    point = 8.0 * moved * np.linalg.norm(rays["direction"], axis=1)      # [n]
    prim = planes["prim"]
    point = np.broadcast_to(point, prim.shape)
    normal = point / radius[np.where(prim >= 0, prim, len(radius) - 1)]
    sin_theta = np.sqrt(np.maximum(1.0 - planes["normal"][..., 1] ** 2, 1e-300))
    uv = normal / (math.pi * sin_theta)
    return {"point": point[..., None], "normal": normal[..., None], "uv": uv[..., None]}
