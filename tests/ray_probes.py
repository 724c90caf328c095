"""Probe rays that take the hit and scatter code to its edges, one known ray (or one fan of rays) at a time.

A jittered camera never lands a ray on a rect's bound, on a tangent, on t == t_min; these probes do.  The camera of a probe
is built by hand: origin = o, upper_left_corner = o + d, horizontal = vertical = 0 (camera.rs:326-337: the jitter then
multiplies zero, every sample of every pixel is the ray (o, d)), or exactly one of the two non-zero along one axis: a fan
of rays with one component of the direction EXACTLY zero.  lens_radius = 0, and time_a = time_b where a MovingSphere is
probed at a fixed time.  The library and the oracle both accept such a camera (tests/test_random_scene_bvh.py:
test_gpu_bvh_with_axis_parallel_rays), so this is a per-ray known-answer harness through the public C ABI.

Two readouts:
  max_depth = 1 over a black background, one solid colour per primitive: the pixel names the primitive that was hit
                (renderer.rs:48-55: albedo x white at depth 0)
  max_depth = 2 or 3 over the Sky: the scattered or refracted direction, and so the normal, shows in the sky's colour or in the
                second hit

PROBES is the table: name -> Probe.  A probe's spec function returns, for alt = False, the scene and the ray ON the edge,
and for alt = True the same with the decisive coordinate one ulp on the other side (spec["ulp"] names the pair of
neighbouring doubles) or, where the probe pins a configuration and not a boundary (a back face, the exit side of a box),
with the other configuration.  tests/test_ray_probes_cpu.py holds every probe to an exact rational model (the q_* functions
below, fractions.Fraction over the doubles' exact values: an independent restatement of the reference's rules, not the
oracle's code) and checks that the oracle's frame moves between the two; tests/test_gpu_ray_probes.py renders every probe
through every route that has hit or scatter code of its own.

Rays that the reference answers with a non-finite t are out of scope (LABNOTES.md): its comparisons are all false on NaN,
so it ACCEPTS (k - o) / d = 0 / 0 and x * inf hits, the box slab form and the tree are documented as open there, and no
probe forms one (test_ray_probes_cpu.py checks every primitive of every probe against every ray).
"""
import math
from collections import namedtuple
from fractions import Fraction as Fr

import numpy as np

import scenes_py as S
import texture_probes as T
import variant_scenes as V

abi = S.abi
L, M, D, E = abi.RT_MAT_LAMBERTIAN, abi.RT_MAT_METAL, abi.RT_MAT_DIELECTRIC, abi.RT_MAT_DIFFUSE_LIGHT
T_MIN = 0.001
INF = math.inf
UP, DOWN = INF, -INF

# ---- routes: the texture probes' (tests/texture_probes.py), every kernel path with hit or scatter code of its own ------------
ROUTES = T.ROUTES
ALL_ROUTES = T.ALL_ROUTES
EXACT_ROUTES = T.EXACT_ROUTES
# where box_slab_t chooses the side of a box (rt_trace_common.h: "ties and such grazing rays are open, SURVEY B-15")
SLAB_ROUTES = ("pool-fast", "pool-fast-bvh", "v1-fast", "guides")
# where the tree's visiting order decides between two hits of the same t (closest_hit_bvh: "only exact ties can differ")
TREE_ROUTES = ("pool-fast-bvh",)
RECTS, SPHERES, ANY = 0, 1, 2

SINGLE, FAN = (8, 8, 4), (64, 8, 4)      # one work item; the widest fan
PALETTE = [(0.9, 0.1, 0.1), (0.1, 0.8, 0.2), (0.15, 0.25, 0.9), (0.8, 0.7, 0.1), (0.6, 0.1, 0.7), (0.1, 0.7, 0.7),
           (0.5, 0.5, 0.5), (0.3, 0.6, 0.1)]
OFF = (0.5, -0.25, 0.75)                  # the Translate of every wrapped probe: dyadic, so that o - offset is exact
WRAPS = {"bare": None, "tr": (None, OFF), "rot90": ((1.0, 0.0), OFF), "rot0": ((0.0, 1.0), OFF)}     # (sin, cos), offset


def nxt(x, toward):
    return float(np.nextafter(x, toward))


def _pz(v):
    """-0.0 -> +0.0: a camera cannot form a negative zero (x - x = +0)."""
    return tuple(float(x) + 0.0 for x in v)


def rot_back(a, sc):     # rotate_y.rs:55-59
    s, c = sc
    return _pz((c * a[0] + s * a[2], a[1], -s * a[0] + c * a[2]))


def world_point(p, wrap):
    """The world point that the wrapper `wrap` takes to the object-space point p."""
    w = WRAPS[wrap]
    if w is None:
        return _pz(p)
    q = rot_back(p, w[0]) if w[0] else _pz(p)
    return tuple(q[i] + w[1][i] for i in range(3))


def world_dir(d, wrap):
    w = WRAPS[wrap]
    return rot_back(d, w[0]) if (w and w[0]) else _pz(d)


def wrapped(prim, wrap):
    w = WRAPS[wrap]
    if w is not None:
        prim.flags = abi.RT_PRIM_HAS_TRANSLATE | (abi.RT_PRIM_HAS_ROTATE_Y if w[0] else 0)
        if w[0]:
            prim.rot_sin, prim.rot_cos = w[0]      # exactly (1, 0) or (0, 1): math.cos(pi / 2) is 6e-17, not 0
        prim.translate = abi.D3(*w[1])
    return prim


def lam(n):
    """n Lambertians, one solid colour each: material i names primitive i."""
    return [(L, PALETTE[i % len(PALETTE)], 0.0, 0.0) for i in range(n)]


# ---- the exact rational model ------------------------------------------------------------------------------------------------
# Every quantity is a Fraction over the exact values of the doubles: no rounding anywhere.  `steps` collects what the
# f64 evaluation forms on the way, in the reference's order of operations, so that a probe can ask whether each was
# representable (then f64, with or without FMA contraction, with a division or a reciprocal that is exact for these
# operands, computes the same number).

def representable(x):
    try:
        return Fr(float(x)) == x
    except OverflowError:
        return False


def fv(v):
    return tuple(Fr(float(x)) for x in v)


def _dot(a, b, steps):
    p = [a[i] * b[i] for i in range(3)]
    s1 = p[0] + p[1]
    s2 = s1 + p[2]
    steps += p + [s1, s2]
    return s2


def _sqrt(x):
    """The exact square root of a non-negative Fraction, or None."""
    n, d = x.numerator, x.denominator
    rn, rd = math.isqrt(n), math.isqrt(d)
    return Fr(rn, rd) if rn * rn == n and rd * rd == d else None


RectQ = namedtuple("RectQ", "t a b hit")
SphereQ = namedtuple("SphereQ", "a half_b c disc sqrtd near far t")
BoxQ = namedtuple("BoxQ", "t side planes")


def q_frame(prim, o, d, steps):
    """translate.rs:31 and rotate_y.rs:39-48: the ray in the primitive's own frame."""
    o, d = fv(o), fv(d)
    if prim.flags & abi.RT_PRIM_HAS_TRANSLATE:
        off = fv(prim.translate[:])
        o = tuple(o[i] - off[i] for i in range(3))
        steps += list(o)
    if prim.flags & abi.RT_PRIM_HAS_ROTATE_Y:
        s, c = Fr(prim.rot_sin), Fr(prim.rot_cos)

        def fwd(a):
            p = [c * a[0], s * a[2], s * a[0], c * a[2]]
            r = (p[0] - p[1], a[1], p[2] + p[3])
            steps.extend(p + list(r))
            return r
        o, d = fwd(o), fwd(d)
    return o, d


def q_rect(axis, p, o, d, t_min, t_max, steps):
    """xy_rect.rs:29-40 and its siblings: t in [t_min, t_max] and the in-plane point in [a0, a1] x [b0, b1], all bounds
    inclusive.  A ray parallel to the plane misses (the reference's t = +-inf or NaN is excluded from the table)."""
    ia, ib = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    a0, a1, b0, b1, k = (Fr(float(x)) for x in p[:5])
    if d[axis] == 0:
        return RectQ(None, None, None, False)
    ko = k - o[axis]
    t = ko / d[axis]
    steps += [ko, t]
    # a = o + t d.  Where d is zero the product is an exact zero whatever t is: t need not be representable for that
    pa, pb = t * d[ia], t * d[ib]
    a, b = o[ia] + pa, o[ib] + pb
    hit = not (t < t_min or t > t_max) and not (a < a0 or a > a1 or b < b0 or b > b1)
    return RectQ(t, a, b, hit)


def q_sphere(center, radius, o, d, t_min, t_max, steps):
    """sphere.rs:39-59: the nearer root of the half-b quadratic if it lies in [t_min, t_max], else the farther one.
    The comparisons are made without a square root (sqrt(disc) >= r <=> r <= 0 or disc >= r^2); a root's VALUE is exact
    where the discriminant is a rational square, and the nearest double's otherwise (then it only orders the hits of a
    scene, never decides a probe's edge)."""
    oc = tuple(o[i] - center[i] for i in range(3))
    steps += list(oc)
    a = _dot(d, d, steps)
    half_b = _dot(oc, d, steps)
    r2 = radius * radius
    c = _dot(oc, oc, steps) - r2
    ac = a * c
    disc = half_b * half_b - ac
    steps += [r2, c, half_b * half_b, ac, disc]
    if disc < 0:
        return SphereQ(a, half_b, c, disc, None, None, None, None)
    sq = _sqrt(disc)
    if sq is not None:
        near, far = (-half_b - sq) / a, (-half_b + sq) / a
        steps += [sq, -half_b - sq, near]
    else:
        f = Fr(math.sqrt(float(disc)))
        near, far = (-half_b - f) / a, (-half_b + f) / a

    def at_least(sign, bound):      # root >= bound, root = (-half_b + sign sqrt(disc)) / a, a > 0
        r = a * bound + half_b
        return (r <= 0 or disc >= r * r) if sign > 0 else (r <= 0 and disc <= r * r)

    def at_most(sign, bound):
        if bound == INF:
            return True
        r = a * bound + half_b
        return (r >= 0 and disc <= r * r) if sign > 0 else (r >= 0 or disc >= r * r)
    t = None
    if at_least(-1, t_min) and at_most(-1, t_max):
        t = near
    elif at_least(+1, t_min) and at_most(+1, t_max):
        t = far
    return SphereQ(a, half_b, c, disc, sq, near, far, t)


def box_sides(p):
    """box.rs:22-71: the six sides in the reference's order, as (axis, (a0, a1, b0, b1, k))."""
    mnx, mny, mnz, mxx, mxy, mxz = (float(x) for x in p[:6])
    return [(2, (mnx, mxx, mny, mxy, mxz)), (2, (mnx, mxx, mny, mxy, mnz)), (1, (mnx, mxx, mnz, mxz, mxy)),
            (1, (mnx, mxx, mnz, mxz, mny)), (0, (mny, mxy, mnz, mxz, mxx)), (0, (mny, mxy, mnz, mxz, mnx))]


def q_box(p, o, d, t_min, t_max, steps):
    """box.rs:82-101: six rect tests, each against the closest so far; a later side of the same t wins."""
    closest, side, planes = t_max, None, []
    for s, (axis, rect) in enumerate(box_sides(p)):
        r = q_rect(axis, rect, o, d, t_min, closest, steps)
        planes.append(r)
        if r.hit:
            closest, side = r.t, s
    return BoxQ(closest if side is not None else None, side, planes)


def q_prim(prim, o, d, time=0.0, t_min=Fr(T_MIN), t_max=INF):
    """-> (t or None, detail, steps) of one primitive with its wrappers."""
    steps = []
    oo, dd = q_frame(prim, o, d, steps)
    kind = prim.kind
    if kind in (abi.RT_PRIM_SPHERE, abi.RT_PRIM_MOVING_SPHERE):
        center = fv(prim.p[:3])
        if kind == abi.RT_PRIM_MOVING_SPHERE:      # moving_sphere.rs:37-39
            cb = fv(prim.center_b[:])
            f = (Fr(float(time)) - Fr(prim.time_a)) / (Fr(prim.time_b) - Fr(prim.time_a))
            center = tuple(center[i] + (cb[i] - center[i]) * f for i in range(3))
            steps += [f] + list(center)
        q = q_sphere(center, Fr(prim.p[3]), oo, dd, t_min, t_max, steps)
        return q.t, q, steps
    if kind == abi.RT_PRIM_BOX:
        q = q_box(prim.p, oo, dd, t_min, t_max, steps)
        return q.t, q, steps
    axis = {abi.RT_PRIM_XY_RECT: 2, abi.RT_PRIM_XZ_RECT: 1, abi.RT_PRIM_YZ_RECT: 0}[kind]
    q = q_rect(axis, prim.p, oo, dd, t_min, t_max, steps)
    return (q.t if q.hit else None), q, steps


def q_scene(prims, o, d, time=0.0):
    """The closest-so-far loop (box.rs:82-101, scene.rs:188-195): every primitive against the closest so far, t == closest accepted: the later one wins a tie.
    -> (index or None, t)"""
    best, closest = None, INF
    for i, prim in enumerate(prims):
        t, _, _ = q_prim(prim, o, d, time, Fr(T_MIN), closest)
        if t is not None:
            best, closest = i, t
    return best, (closest if best is not None else None)


Edge = namedtuple("Edge", "on exact")     # the edge is reached; the quantities that decide it (each must be representable)


# ---- the probe ---------------------------------------------------------------------------------------------------------------

class Probe:
    """name; cls: the edge class of the issue's list; form: the prims_class the scene must select; fn(alt) -> spec;
    routes; depth: max_depth; tie: None, or (routes on which the choice is open, the obj_ids tied, their normals)."""

    def __init__(self, name, cls, form, fn, routes=ALL_ROUTES, depth=1, tie=None, rounding=False):
        self.name, self.cls, self.form, self.fn, self.routes, self.depth, self.tie = name, cls, form, fn, tuple(routes), depth, tie
        self.rounding = rounding      # the decisive quantity is NOT free of rounding in f64: exact routes only
        self.__doc__ = fn.__doc__
        assert not rounding or set(routes) <= set(EXACT_ROUTES)

    def spec(self, alt=False):
        s = dict(fan=None, time=0.0, ulp=None, own_tree=False, mats=None)
        s.update(self.fn(alt))
        if s["mats"] is None:
            s["mats"] = lam(len(s["prims"]))
        return s

    @property
    def shape(self):
        return FAN if self.spec()["fan"] else SINGLE

    def guide_shape(self):
        w, h, _ = self.shape
        return (w, h, 1)

    def params(self, shape=None):
        w, h, spp = shape or self.shape
        return abi.render_params(w, h, spp, max_depth=self.depth)

    def bundle(self, alt=False, fillers=False):
        """`fillers`: six small spheres far outside every ray's reach, so that RT_HIT_BVH walks a tree with inner nodes
        (texture_probes._bundle); a probe of the "bvh" classes brings a tree of its own."""
        s = self.spec(alt)
        prims = list(s["prims"])
        mats = list(s["mats"])
        if fillers and not s["own_tree"]:
            mats.append((L, (0.5, 0.5, 0.5), 0.0, 0.0))
            for i in range(6):
                prims.append(abi.sphere((1.0e4 + 40.0 * i, 1.0e4, 1.0e4 + 25.0 * i), 1.0, len(mats) - 1))
        textures = [abi.solid(m[1]) for m in mats]
        materials = [abi.material(m[0], -1 if m[0] == D else i, m[2], m[3]) for i, m in enumerate(mats)]
        for i, p in enumerate(prims):
            p.obj_id = i + 1
        bg = abi.solid_background((0.0, 0.0, 0.0)) if self.depth == 1 else abi.sky()
        return abi.SceneBundle(prims, materials, textures, bg)

    def camera(self, alt=False):
        s = self.spec(alt)
        return camera(s["o"], s["d"], s["fan"], s["time"])


def camera(o, d, fan=None, time=0.0):
    cam = abi.RtCamera()
    ulc = tuple(float(o[i]) + float(d[i]) for i in range(3))
    assert tuple(ulc[i] - float(o[i]) for i in range(3)) == tuple(float(x) for x in d), (o, d)    # d bit for bit
    cam.origin, cam.upper_left_corner = abi.D3(*o), abi.D3(*ulc)
    cam.horizontal = abi.D3(*(fan[1] if fan and fan[0] == "h" else (0.0, 0.0, 0.0)))
    cam.vertical = abi.D3(*(fan[1] if fan and fan[0] == "v" else (0.0, 0.0, 0.0)))
    cam.right, cam.up, cam.forward = abi.D3(1, 0, 0), abi.D3(0, 1, 0), abi.D3(0, 0, 1)
    cam.lens_radius, cam.focus_distance, cam.time_a, cam.time_b = 0.0, 10.0, time, time
    return cam


def oracle_frame(orc, probe, alt=False, fillers=False):
    """-> (frame, segments) of the oracle's LINEAR scan, for every probe: the closest-so-far loop (box.rs:82-101) is where the reference's rule for
    two hits of the same t (the later one wins) is written down, and a tree's visiting order would replace it."""
    bundle = probe.bundle(alt, fillers)
    return orc.render(bundle.desc, probe.camera(alt), probe.params(), use_bvh=0)


PROBES = {}


def add(name, cls, form, fn, **kw):
    assert name not in PROBES, name
    PROBES[name] = Probe(name, cls, form, fn, **kw)


# ---- rects -------------------------------------------------------------------------------------------------------------------
AXES = {"xy": (abi.RT_PRIM_XY_RECT, 2, 0, 1), "xz": (abi.RT_PRIM_XZ_RECT, 1, 0, 2), "yz": (abi.RT_PRIM_YZ_RECT, 0, 1, 2)}
A0, A1, B0, B1, K = -1.0, 1.0, -1.0, 2.0, -4.0
TAU = Fr(T_MIN)


def v3(ax, ia, ib, k, a, b):
    out = [0.0, 0.0, 0.0]
    out[ax], out[ia], out[ib] = k, a, b
    return tuple(out)


RECT_DOCS = {
    "plane_a0": "A fan of rays lying exactly in the plane a == a0 (o.a == a0, d.a == 0): a = o.a + t * 0 is a0 itself, and "
                "`a < a0` is false: the bound is inclusive (xy_rect.rs:37 and its siblings).  Across the fan b runs over both of "
                "its bounds.  alt: o.a one ulp outside, every ray misses.",
    "plane_a1": "The same fan in the plane a == a1: `a > a1` is false (xy_rect.rs:37).  alt: one ulp outside.",
    "corner": "One ray through the corner (a0, b1): both inclusive bounds at once (xy_rect.rs:37; test_oracle_kats.py: "
              "'exactly on the corner').  alt: o.b one ulp beyond b1.",
    "outside_ulp": "The neighbour of the bound: o.a one ulp beyond a1 misses (xy_rect.rs:37).  alt: o.a == a1 hits.",
    "tmin": "t == t_min = 0.001 exactly: d[axis] = +-1 and k - o[axis] = -+0.001's double, so that the quotient (or the product "
            "with the ray's reciprocal, 1 / +-1) is 0.001 itself; `t < t_min` is false (xy_rect.rs:32).  alt: k one ulp nearer.",
    "tmin_below": "t one ulp below t_min: rejected (xy_rect.rs:32), the backdrop shows.  alt: t == t_min.",
    "back_face": "dir[axis] > 0: the back face, normal -e_axis (xy_rect.rs:43-45, geometry.rs:49-56; the device takes it from "
                 "the sign bit of dir[axis], set_face_normal_axis).  A Lambertian at max_depth 2 over the sky: normal + "
                 "unit(sample) (lambertian.rs:26-38) decides the colour.  alt: the same rect from the front.",
    "front_face": "dir[axis] < 0: the front face, normal +e_axis, under a Lambertian at max_depth 2 (lambertian.rs:26-38).  "
                  "alt: from behind.",
    "coplanar": "Two overlapping rects in one plane: the same t, and `t > t_max` is false, so the LATER one wins "
                "(xy_rect.rs:32 inside the closest-so-far loop, box.rs:82-101; the linear loops keep the description's order within a group).  Through the tree the visiting "
                "order decides (closest_hit_bvh: 'only exact ties can differ'): either colour.  alt: the two swapped.",
}


def rect_probe(edge, axname, wrap):
    kind, ax, ia, ib = AXES[axname]
    sgn = 1.0 if axname == "xz" else -1.0      # the ray travels along -axis (xy, yz) or +axis (xz): both signs of d[axis]

    def fn(alt):
        a0, a1, b0, b1, k = A0, A1, B0, B1, sgn * 4.0
        o_ax, d_ax, a, b, d_b, fan, ulp = 0.0, sgn, 0.25, 0.5, 0.0, None, None
        rects = None
        if edge in ("plane_a0", "plane_a1"):
            bound, out = (A0, DOWN) if edge == "plane_a0" else (A1, UP)
            ulp = (bound, nxt(bound, out))
            a, d_b = ulp[int(alt)], -0.5
            fan = ("h", world_dir(v3(ax, ia, ib, 0.0, 0.0, 1.0), wrap))      # b = 0.5 + 4 (-0.5 + u): -1.5 .. 2.5
        elif edge == "corner":
            ulp = (B1, nxt(B1, UP))
            a, b = A0, ulp[int(alt)]
        elif edge == "outside_ulp":
            ulp = (nxt(A1, UP), A1)
            a = ulp[int(alt)]
        elif edge in ("tmin", "tmin_below"):
            ulp = (sgn * T_MIN, nxt(sgn * T_MIN, 0.0))
            if edge == "tmin_below":
                ulp = ulp[::-1]
            k = ulp[int(alt)]
        elif edge in ("back_face", "front_face"):
            d_ax = 1.0 if (edge == "back_face") != alt else -1.0      # dir[axis] > 0 meets the back face
            o_ax = k - 4.0 * d_ax
        elif edge == "coplanar":
            rects = [(a0, a1, b0, b1), (0.0, 2.0, b0, b1)]
            if alt:
                rects.reverse()
            a = 0.5
        if rects is None:
            rects = [(a0, a1, b0, b1)]
        prims = [wrapped(abi.rect(kind, r[0], r[1], r[2], r[3], k, i), wrap) for i, r in enumerate(rects)]
        if alt and edge == "coplanar":      # the colours stay with the rects, not with the positions
            prims[0].material, prims[1].material = 1, 0
        # a backdrop in the same frame: a ray that misses the probed rect shows another colour, not the background's
        prims.append(wrapped(abi.rect(kind, -50.0, 50.0, -50.0, 50.0, o_ax + 20.0 * d_ax, len(prims)), wrap))
        o = world_point(v3(ax, ia, ib, o_ax, a, b), wrap)
        d = world_dir(v3(ax, ia, ib, d_ax, 0.0, d_b), wrap)

        def check():
            t, q, steps = q_prim(prims[0], o, d)
            frame = steps[:-2]      # the wrappers' own steps (q_rect appends k - o and t)
            if edge in ("plane_a0", "plane_a1"):
                return Edge(q.a == Fr(ulp[0]) and q.t >= TAU, frame + [q.a])      # (b runs over the fan)
            if edge == "corner":
                return Edge(q.a == Fr(A0) and q.b == Fr(B1) and q.hit, frame + [q.t, q.a, q.b])
            if edge == "outside_ulp":
                return Edge(q.a == Fr(ulp[0]) and q.a > Fr(A1) and not q.hit, frame + [q.a])
            if edge == "tmin":
                return Edge(q.t == TAU and q.hit, steps)
            if edge == "tmin_below":
                return Edge(q.t < TAU and Fr(nxt(float(q.t), UP)) == TAU and not q.hit, steps)
            if edge in ("back_face", "front_face"):
                oo, dd = q_frame(prims[0], o, d, [])
                return Edge(q.hit and (dd[ax] > 0) == (edge == "back_face"), steps + [q.a, q.b])
            t1, q1, _ = q_prim(prims[1], o, d)
            return Edge(q.hit and q1.hit and t == t1, steps + [q.a, q.b])
        return dict(prims=prims, o=o, d=d, fan=fan, ulp=ulp, check=check)
    fn.__doc__ = RECT_DOCS[edge]
    return fn


_RECT_EDGES = ["plane_a0", "plane_a1", "corner", "outside_ulp", "tmin", "tmin_below", "back_face", "front_face", "coplanar"]
for _i, _edge in enumerate(_RECT_EDGES):
    _depth = 2 if _edge in ("back_face", "front_face") else 1
    _tie = (TREE_ROUTES, (1, 2), None) if _edge == "coplanar" else None
    for _ax in ("xy", "xz", "yz"):
        add("rect_%s[%s]" % (_edge, _ax), "rect_" + _edge, RECTS, rect_probe(_edge, _ax, "bare"), depth=_depth, tie=_tie)
    # the wrapped forms (translate.rs:24-41, rotate_y.rs:31-64), the axes taken in turn
    _axes = ("xy", "xz", "yz")
    add("rect_%s[%s,tr]" % (_edge, _axes[_i % 3]), "rect_" + _edge + "_wrapped", ANY, rect_probe(_edge, _axes[_i % 3], "tr"),
        depth=_depth, tie=_tie)
    add("rect_%s[%s,rot90]" % (_edge, _axes[(_i + 1) % 3]), "rect_" + _edge + "_wrapped", ANY,
        rect_probe(_edge, _axes[(_i + 1) % 3], "rot90"), depth=_depth, tie=_tie)


# ---- spheres -----------------------------------------------------------------------------------------------------------------

def _aside(material):
    """A small rect behind every probe's camera: it makes a scene of spheres an any-primitive one without standing between
    a scattered ray and the sky (a backdrop would be what every second segment hits)."""
    return abi.rect(abi.RT_PRIM_XY_RECT, 29.0, 31.0, -1.0, 1.0, 60.0, material)


SPHERE_DOCS = {
    "tangent": "A tangent ray with dyadic inputs: centre (1, 0, -1), r = 1, o = 0, d = (0, 0, -1): discriminant 1 - 1 = 0 exactly, "
               "`discriminant < 0` is false and both roots are 1 (sphere.rs:46-49).  The numbers are small on purpose: with the centre "
               "one ulp farther (alt) c = 1 + 2^-51 is still representable and the f64 discriminant is -2^-51, a miss; beside a "
               "|oc|^2 of 26 that ulp would be rounded away.",
    "tangent_d2": "The same tangent with an unnormalised d, |d|^2 = 4: half_b = -2, a c = 4, root 2 / 4 (sphere.rs:39-52; the "
                  "device multiplies by 1 / |d|^2 = 0.25).",
    "tangent_d3": "The tangent of sphere.rs:46-49 with |d|^2 = 9, no power of two: the discriminant 9 - 9 is still exact; the root 3 / 9 is not, "
                  "and does not decide anything at max_depth 1.",
    "root_tmin": "The near root EQUAL to t_min: r = 2^-8, centre (0, 0, -(0.001 + r)) (representable: 0.001's double is a multiple "
                 "of 2^-60), so that the root is 0.001's double in exact arithmetic, and in f64 too; `root < t_min` is false, the "
                 "front face is hit (sphere.rs:53).  A Lambertian at max_depth 2: the near root scatters into the sky, the far one "
                 "into the sphere.  The squares of these 51-bit numbers are NOT representable: a rounding decides in f64, so the probe "
                 "runs on the RT_ARITH_REFERENCE routes only, which round as the reference does.  alt: the centre one ulp nearer.",
    "root_below": "The near root one ulp below t_min: the far root is taken (sphere.rs:53-58).  RT_ARITH_REFERENCE routes only, as "
                  "root_tmin.  alt: root == t_min.",
    "inside": "The origin inside the sphere: the near root is negative, the far one is taken, a back face (sphere.rs:53-58, "
              "geometry.rs:49-56).  Lambertian, max_depth 2.  alt: the origin outside.",
    "surface": "The origin ON the surface: centre 0, r = 1, o = (0, 0, 1), d = (0, 0, -1): c = 0, the near root is exactly 0 < t_min and "
               "is rejected, the far root 2 is taken: the self-intersection guard (sphere.rs:53-58, renderer.rs: t_min = 0.001).  "
               "alt: the origin outside, at z = 1.5.",
    "neg_radius": "A negative radius: outward = (p - c) / r points INWARD, so the hit from outside is a back face and the normal is "
                  "flipped once more (sphere.rs:61-66): the same normal as with r = +1, but front_face is false, and front_face selects a "
                  "Dielectric's ratio (dialectric.rs:27-31).  An oblique ray, max_depth 3.  alt: r = +1.",
}


def sphere_probe(edge, form):
    """form: "spheres" (the spheres-only kernel), "group" (a plain sphere in the any-primitive table: its sphere group, and the
    compact leaf record of the tree), "flagged" (a Translate around it: prim_t<PRIMS_ANY> in both)."""
    wrap = "tr" if form == "flagged" else "bare"

    def fn(alt):
        c, r, o, d, ulp = (1.0, 0.0, -1.0), 1.0, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), None
        if edge.startswith("tangent"):
            ulp = (1.0, nxt(1.0, UP))
            c = (ulp[int(alt)], 0.0, -1.0)
            d = (0.0, 0.0, -float({"tangent": 1, "tangent_d2": 2, "tangent_d3": 3}[edge]))
        elif edge in ("root_tmin", "root_below"):
            r = 2.0 ** -8
            ulp = (-(T_MIN + r), nxt(-(T_MIN + r), 0.0))
            if edge == "root_below":
                ulp = ulp[::-1]
            c = (0.0, 0.0, ulp[int(alt)])
        elif edge == "inside":
            c, r, o = (0.0, 0.0, 0.0), 2.0, (0.0, 0.0, 4.0 if alt else 0.5)
        elif edge == "surface":
            c, r, o = (0.0, 0.0, 0.0), 1.0, (0.0, 0.0, 1.5 if alt else 1.0)
        elif edge == "neg_radius":
            c, r, o = (0.0, 0.0, -5.0), (1.0 if alt else -1.0), (0.25, 0.5, 0.0)
        prims = [wrapped(abi.sphere(c, r, 0), wrap)]
        if form == "spheres":
            prims.append(abi.sphere((0.0, 0.0, -200.0), 100.0, 1) if edge.startswith("tangent") else abi.sphere((30.0, 0.0, 60.0), 1.0, 1))
        else:
            prims.append(abi.rect(abi.RT_PRIM_XY_RECT, -50.0, 50.0, -50.0, 50.0, -100.0, 1) if edge.startswith("tangent") else _aside(1))
        ow, dw = world_point(o, wrap), world_dir(d, wrap)

        def check():
            t, q, steps = q_prim(prims[0], ow, dw)
            if edge.startswith("tangent"):
                return Edge(q.disc == 0 and t == q.near == q.far, steps[:-1] if edge == "tangent_d3" else steps)
            if edge == "root_tmin":
                return Edge(q.near == TAU and t == q.near, steps)
            if edge == "root_below":
                return Edge(q.near < TAU and t == q.far, steps)
            if edge == "inside":
                return Edge(q.c < 0 and q.near < 0 and t == q.far, steps)
            if edge == "surface":
                return Edge(q.c == 0 and q.near == 0 and t == q.far == 2, steps)
            return Edge(Fr(prims[0].p[3]) < 0 and t == q.near, steps)
        mats = [(D, (1, 1, 1), 0.0, 1.5), (L, PALETTE[1], 0.0, 0.0)] if edge == "neg_radius" else None
        return dict(prims=prims, o=ow, d=dw, ulp=ulp, check=check, mats=mats)
    fn.__doc__ = SPHERE_DOCS[edge]
    return fn


_FORMS = {"spheres": SPHERES, "group": ANY, "flagged": ANY}
for _i, _edge in enumerate(["tangent", "tangent_d2", "tangent_d3", "root_tmin", "root_below", "inside", "surface", "neg_radius"]):
    _kw = dict(depth=1 if _edge.startswith("tangent") else (3 if _edge == "neg_radius" else 2))
    if _edge in ("root_tmin", "root_below"):
        _kw.update(routes=EXACT_ROUTES, rounding=True)
    # every edge in the spheres-only form; in the any-primitive table the group and the flagged sphere take turns, the plain
    # tangent runs in both
    # (neg_radius in the group: inside a Translate front_face is always true, translate.rs:36, and r's sign shows in nothing)
    _forms = ["spheres", "group" if (_i % 2 == 0 or _edge == "neg_radius") else "flagged"] + (["flagged"] if _edge == "tangent" else [])
    for _form in _forms:
        add("sphere_%s[%s]" % (_edge, _form), "sphere_" + _edge, _FORMS[_form], sphere_probe(_edge, _form), **_kw)


def moving_probe(other_interval):
    def fn(alt):
        x = nxt(1.0, UP) if alt else 1.0
        prims = []
        if other_interval:      # the first MovingSphere sets the tree's scene-wide interval (rt_plan.cpp: leaf_geometry)
            prims.append(abi.moving_sphere((40.0, 40.0, 0.0), (40.0, 44.0, 0.0), 1.0, 2, 0, 0.0, 1.0))
        # the centre is (x, -2, -1) at 0.25 and (x, 2, -1) at 0.75
        prims.append(abi.moving_sphere((x, -2.0, -1.0), (x, 2.0, -1.0), 1.0, 0, 0, 0.25, 0.75))
        prims.append(abi.rect(abi.RT_PRIM_XY_RECT, -50.0, 50.0, -50.0, 50.0, -100.0, 1))
        time = 0.5 if other_interval else 0.25
        o, d = (0.0, 0.0 if other_interval else -2.0, 0.0), (0.0, 0.0, -1.0)
        probed = prims[-2]

        def check():
            t, q, steps = q_prim(probed, o, d, time)
            return Edge(q.disc == 0 and t == q.near == 1, steps)
        return dict(prims=prims, o=o, d=d, time=time, ulp=(1.0, nxt(1.0, UP)), check=check,
                    mats=lam(3) if other_interval else None)
    fn.__doc__ = ("A MovingSphere tangent to the ray at the ray's time: the camera's shutter is the single instant %s, where the "
                  "centre (moving_sphere.rs:37-39) is exactly (1, %s, -1) and the discriminant exactly 0 (moving_sphere.rs:49-69).  %s"
                  "alt: both end points one ulp farther in x." %
                  (("0.5, the middle of the sphere's interval [0.25, 0.75]", "0",
                    "Another MovingSphere, listed first, has the interval [0, 1]: in the tree this one keeps the general record.  ")
                   if other_interval else ("0.25 == time_a", "-2", "")))
    return fn


add("moving_time_a", "moving_sphere", ANY, moving_probe(False))
add("moving_other_interval", "moving_sphere", ANY, moving_probe(True))


# ---- boxes -------------------------------------------------------------------------------------------------------------------
BOX = ((-1.0, -1.0, -6.0), (1.0, 1.0, -4.0))
BOX_DOCS = {
    "entry": "Entry through the %s pair of sides: the side with the smallest t in range whose in-plane point lies inside wins "
             "(box.rs:82-101; box_slab_t: the axis whose nearer distance t_enter equals).  Lambertian at max_depth 2: the side's normal "
             "shows.  alt: entry from the opposite side.",
    "inside": "The origin inside the box: the exit side is returned, a back face (box.rs:82-101; box_slab_t: entry is false).  "
              "alt: the origin outside.",
    "near_tmin": "The origin 2^-11 in front of a side: t_enter = 0.00049 < t_min, the entry side is rejected and the EXIT side at "
                 "t = 2.00049 is the hit (xy_rect.rs:32 in each of box.rs:82-101's six tests).  alt: 2^-9 in front, t_enter = 0.00195 is "
                 "accepted.",
    "edge": "A ray through the edge x = 1, z = -4 with t_enter = 2 on both axes: the reference's six rect tests return the later "
            "side, yz at max.x (box.rs:22-71's order); box_slab_t asks z first (its comment: ties are open, SURVEY B-15).  At "
            "max_depth 1 the colour is the box's either way.  alt: the ray moved past the box (a depth-1 frame can only tell a hit "
            "from a miss; box_edge_side shows the side).",
    "vertex": "A ray through the vertex (1, 1, -4): t_enter = 2 on all three axes; the reference returns yz at max.x, the last of the "
              "three (box.rs:22-71).  As box_edge.",
    "edge_side": "box_edge at max_depth 2 on the routes that run the reference's six rect tests in the reference's order (box.rs:22-71, :82-101): the side "
                 "is yz at max.x, normal +x, and the Lambertian's scatter shows it.  alt: o.x one ulp smaller: t_x < t_z = 2, where "
                 "the x side's in-plane z is still above -4: the ray enters through the z side alone, normal +z.",
}


def box_probe(edge, wrap="bare", axis=2):
    def fn(alt):
        mn, mx = BOX
        ulp = None
        d = [0.0, 0.0, 0.0]
        if edge == "entry":
            o = [0.25, 0.5, -5.0]      # (the box's centre is (0, 0, -5))
            far = {0: 3.0, 1: 3.0, 2: -2.0}[axis]
            o[axis] = far if not alt else 2.0 * (0.0 if axis < 2 else -5.0) - far
            if axis < 2:
                o[2] = -4.5
            d[axis] = -1.0 if not alt else 1.0
        elif edge == "inside":
            o, d = [0.25, 0.5, -2.0 if alt else -5.0], [0.0, 0.0, -1.0]
        elif edge == "near_tmin":
            o, d = [0.25, 0.5, -4.0 + (2.0 ** -9 if alt else 2.0 ** -11)], [0.0, 0.0, -1.0]
        elif edge == "edge":
            o, d = [7.0 if alt else 3.0, 0.5, -2.0], [-1.0, 0.0, -1.0]
        elif edge == "edge_side":
            ulp = (3.0, nxt(3.0, DOWN))
            o, d = [ulp[int(alt)], 0.5, -2.0], [-1.0, 0.0, -1.0]
        else:
            o, d = [7.0 if alt else 3.0, 3.0, -2.0], [-1.0, -1.0, -1.0]
        prims = [wrapped(abi.box(mn, mx, 0), wrap),
                 wrapped(abi.rect(abi.RT_PRIM_XY_RECT, -50.0, 50.0, -50.0, 50.0, -100.0, 1), wrap)]
        ow, dw = world_point(o, wrap), world_dir(d, wrap)

        def check():
            t, q, steps = q_prim(prims[0], ow, dw)
            ts = [p.t for p in q.planes]      # plane distances in box.rs's order: z max, z min, y max, y min, x max, x min
            if edge == "entry":
                return Edge(q.side == {2: 0, 1: 2, 0: 4}[axis] and t == 2, steps)
            if edge == "inside":
                return Edge(q.side == 1 and t == 1 and ts[0] < 0, steps)
            if edge == "near_tmin":
                return Edge(q.side == 1 and 0 < ts[0] < TAU, steps)
            if edge in ("edge", "edge_side"):
                return Edge(ts[0] == ts[4] == 2 and q.side == 4 and q.planes[0].hit, steps)
            return Edge(ts[0] == ts[2] == ts[4] == 2 and q.side == 4 and q.planes[0].hit and q.planes[2].hit, steps)
        return dict(prims=prims, o=ow, d=dw, ulp=ulp, check=check)
    fn.__doc__ = BOX_DOCS[edge] % ("xyz"[axis],) if edge == "entry" else BOX_DOCS[edge]
    return fn


for _axis in (0, 1, 2):
    add("box_entry[%s]" % "xyz"[_axis], "box_entry", ANY, box_probe("entry", "bare", _axis), depth=2)
# rotate_y.rs:31-64 with sin = 1, cos = 0 and with sin = 0, cos = 1 exactly, inside a Translate
add("box_entry[z,rot90]", "box_rotated", ANY, box_probe("entry", "rot90", 2), depth=2)
add("box_entry[x,rot0]", "box_rotated", ANY, box_probe("entry", "rot0", 0), depth=2)
add("box_inside", "box_inside", ANY, box_probe("inside"), depth=2)
add("box_inside[rot90]", "box_rotated", ANY, box_probe("inside", "rot90"), depth=2)
add("box_near_tmin", "box_near_tmin", ANY, box_probe("near_tmin"), depth=2)
_X, _Y, _Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
add("box_edge", "box_tie", ANY, box_probe("edge"), tie=(SLAB_ROUTES, (1,), (_X, _Z)))
add("box_vertex", "box_tie", ANY, box_probe("vertex"), tie=(SLAB_ROUTES, (1,), (_X, _Y, _Z)))
add("box_edge_side", "box_tie_side", ANY, box_probe("edge_side"), routes=EXACT_ROUTES, depth=2)


# ---- the tree ----------------------------------------------------------------------------------------------------------------

def _near_fillers(material):
    """Six small spheres around the probe, off every ray: a tree with inner nodes whose extent is the probe's own, so that
    the padding of the f32 boxes (2^-20 of the extent, rt_bvh.cpp) is as small as the scene allows."""
    return [abi.sphere((3.0 * sx, 2.5 * sy, -3.0 + sz), 0.25, material)
            for sx, sy, sz in ((-1, -1, 0), (1, -1, 1), (-1, 1, 2), (1, 1, -1), (-1, 0.5, -2), (1, -0.5, 3))]


def bvh_f32_probe(alt):
    """A rect whose bounds are not f32-representable (k = -0.1, a in [0.1, 0.7]) in a small tree, hit by a fan in the plane
    a == a0 = 0.1 (xy_rect.rs:37, inclusive): the ray only touches the rect's extreme coordinate.  The nearest f32 of 0.1 lies ABOVE it: a culling box
    rounded to nearest instead of outward would cull a true hit (rt_bvh_slab.h, rt_bvh.cpp: the boxes are rounded outward and
    padded).  alt: o.a one ulp outside."""
    ulp = (0.1, nxt(0.1, DOWN))
    prims = [abi.rect(abi.RT_PRIM_XY_RECT, 0.1, 0.7, -1.0, 2.0, -0.1, 0),
             abi.rect(abi.RT_PRIM_XY_RECT, -50.0, 50.0, -50.0, 50.0, -20.0, 1)] + _near_fillers(2)
    o, d = (ulp[int(alt)], 0.5, 4.0), (0.0, -0.5, -1.0)      # t = 4.1: b runs from -1.55 to 2.55 across the fan

    def check():
        t, q, steps = q_prim(prims[0], o, d)
        return Edge(q.a == Fr(0.1) and q.t >= TAU and float(np.float32(0.1)) > 0.1, [q.a])      # (b runs over the fan)
    return dict(prims=prims, o=o, d=d, fan=("h", (0.0, 1.0, 0.0)), ulp=ulp, check=check, own_tree=True, mats=lam(3))


def bvh_flat_probe(alt):
    """A flat XZ rect in a small tree: its f32 box has zero thickness before padding, and the ray (0, -1, 0) meets it head-on,
    in the corner (a0, b1) (xz_rect.rs:37).  alt: one ulp beyond b1."""
    ulp = (2.0, nxt(2.0, UP))
    prims = [abi.rect(abi.RT_PRIM_XZ_RECT, -1.0, 1.0, -1.0, 2.0, -4.0, 0),
             abi.rect(abi.RT_PRIM_XZ_RECT, -50.0, 50.0, -50.0, 50.0, -20.0, 1)] + _near_fillers(2)
    o, d = (-1.0, 0.0, ulp[int(alt)]), (0.0, -1.0, 0.0)

    def check():
        t, q, steps = q_prim(prims[0], o, d)
        return Edge(q.a == -1 and q.b == 2 and q.hit, steps + [q.a, q.b])
    return dict(prims=prims, o=o, d=d, ulp=ulp, check=check, own_tree=True, mats=lam(3))


_LARGE = {}


def bvh_global_probe(alt):
    """The tangent sphere of sphere_tangent beside variant_scenes.large_bvh_scene's 3000 spheres: the node array does not fit
    LDS (bvh_nodes_in_lds == 0), the walk reads the direction-ordered copies from global memory and tests the compact leaf
    record (closest_hit_bvh; sphere.rs:46-49).  RT_HIT_BVH only: the other routes have no path of their own for it."""
    if "prims" not in _LARGE:
        bundle, _ = V.large_bvh_scene()
        _LARGE["prims"] = [abi.sphere(tuple(bundle.primitives[i].p[:3]), bundle.primitives[i].p[3], 2)
                           for i in range(bundle.desc.n_primitives)]
    ulp = (101.0, nxt(101.0, UP))
    prims = [abi.sphere((ulp[int(alt)], 0.0, -1.0), 1.0, 0), abi.sphere((100.0, 0.0, -300.0), 100.0, 1)] + _LARGE["prims"]
    o, d = (100.0, 0.0, 0.0), (0.0, 0.0, -1.0)

    def check():
        t, q, steps = q_prim(prims[0], o, d)
        return Edge(q.disc == 0 and t == 1, steps)
    return dict(prims=prims, o=o, d=d, ulp=ulp, check=check, own_tree=True, mats=lam(3))


add("bvh_f32_extreme", "bvh_f32_box", ANY, bvh_f32_probe, routes=TREE_ROUTES)
add("bvh_flat_rect", "bvh_flat_box", ANY, bvh_flat_probe, routes=TREE_ROUTES)
add("bvh_global_nodes", "bvh_global", SPHERES, bvh_global_probe, routes=TREE_ROUTES)


# ---- materials, max_depth >= 2 over the sky ----------------------------------------------------------------------------------

def _ball(mat, o, d, wrap="bare", c=(0.0, 0.0, -5.0), r=1.0):
    prims = [wrapped(abi.sphere(c, r, 0), wrap)]
    if wrap != "bare":      # (a plain sphere keeps the scene in the spheres-only form)
        prims.append(_aside(1))
    return dict(prims=prims, o=world_point(o, wrap), d=world_dir(d, wrap), mats=[mat, (L, PALETTE[1], 0.0, 0.0)][:len(prims)])


def diel_head_on(alt):
    """A Dielectric sphere met head-on: unit(d) = (0, 0, -1) = -normal exactly, cos_theta = min(1, 1): the clamp's edge, sin_theta
    = sqrt(1 - 1) = 0, Schlick's reflectance is r0 itself (dialectric.rs:17-22, :33-36; refract: vec3.rs:416-422, sqrt(|1 - 0|)).
    max_depth 3: in, out, sky.  d = (0, 0, -2) is unnormalised; 2 / 2 is exact.  alt: an oblique hit, o.x = 0.5."""
    s = _ball((D, (1, 1, 1), 0.0, 1.5), (0.5 if alt else 0.0, 0.25 if alt else 0.0, 0.0), (0.0, 0.0, -2.0))
    prim, o, d = s["prims"][0], s["o"], s["d"]

    def check():
        t, q, steps = q_prim(prim, o, d)
        hit = tuple(Fr(o[i]) + t * Fr(d[i]) for i in range(3))
        n = tuple(hit[i] - Fr(prim.p[i]) for i in range(3))
        return Edge(n == (0, 0, 1) and t == q.near, steps)      # unit(d) . n = -1: cos_theta = 1 exactly
    return dict(s, check=check)


def diel_critical(above):
    def fn(alt):
        side = above != alt
        # Pythagorean directions: sin_theta = 20 / 29 = 0.690 (1.5 x: 1.034) and 48 / 73 = 0.658 (1.5 x: 0.986)
        dy, dz = (20.0, 21.0) if side else (48.0, 55.0)
        prims = [abi.rect(abi.RT_PRIM_XY_RECT, -500.0, 500.0, -500.0, 500.0, -4.0, 0)]
        o, d = (0.0, 0.0, -80.0), (0.0, dy, dz)

        def check():
            t, q, steps = q_prim(prims[0], o, d)
            sin2 = Fr(int(dy * dy), int(dy * dy + dz * dz))
            return Edge(q.hit and d[2] > 0 and (Fr(9, 4) * sin2 > 1) == side, [])      # (no ulp decides here: the docstring)
        return dict(prims=prims, o=o, d=d, mats=[(D, (1, 1, 1), 0.0, 1.5)], check=check)
    fn.__doc__ = ("A Dielectric pane (ior 1.5) hit from INSIDE, on its back face (front_face false selects ratio = ior, "
                  "dialectric.rs:27-31), just %s the critical angle: ratio^2 (1 - cos^2) = 2.25 x %s = %s 1, `ratio * sin_theta > 1.0` "
                  "(dialectric.rs:35-36) is %s.  The margin (1.4 %% / 3.4 %%) is far above any rounding of unit(d) or of the device's "
                  "1 / ior; what is pinned is the side of the threshold and the choice of ratio.  max_depth 2: the reflected "
                  "ray goes down, the refracted one on, and the sky tells them apart.  alt: the other side of the angle."
                  % (("above", "400 / 841", ">", "true: every sample reflects") if above else
                     ("below", "2304 / 5329", "<", "false: refraction, or Schlick's reflection by the draw")))
    return fn


def diel_ior(ior):
    def fn(alt):
        s = _ball((D, (1, 1, 1), 0.0, ior), (0.125, 0.25, 0.0) if alt else (0.75, 0.5, 0.0), (0.0, 0.0, -1.0))
        prim, o, d = s["prims"][0], s["o"], s["d"]

        def check():
            t, q, steps = q_prim(prim, o, d)
            sin2 = Fr(o[0]) ** 2 + Fr(o[1]) ** 2      # the ray runs along -z at the distance sqrt(x^2 + y^2) from the axis of a unit sphere
            ratio2 = 1 / Fr(ior) ** 2
            return Edge(t == q.near and sin2 == Fr(13, 16) and (ratio2 * sin2 > 1) == (ior < 1.0), [q.disc])
        return dict(s, check=check)
    fn.__doc__ = ("A Dielectric sphere with ior = %s hit obliquely from outside, sin^2 = 0.8125: %s (dialectric.rs:17-22, :27-36; the "
                  "device keeps 1 / ior and r0 from the upload).  max_depth 3.  alt: sin^2 = 5 / 64%s." %
                  (("1", "ratio = 1 on both faces, r0 = 0, the ray goes straight through up to Schlick's (1 - cos)^5", "")
                   if ior == 1.0 else
                   ("0.5", "ratio = 1 / ior = 2 on the FRONT face, 4 x 0.8125 > 1, total reflection from outside",
                    ", 4 x 5 / 64 < 1: refraction")))
    return fn


def diel_translate_back(alt):
    """A Dielectric sphere inside a Translate, passed through: leaving through the back face the reference runs set_face_normal a
    second time with the already flipped normal (translate.rs:36, SURVEY B-12), which turns front_face back to TRUE, and
    front_face selects ratio = 1 / ior (dialectric.rs:27-31): the ray leaves as if it entered.  max_depth 3.  alt: the same
    sphere at the same place without the wrapper, where front_face is false on the way out."""
    c = (0.0, 0.0, -5.0)
    if alt:
        s = _ball((D, (1, 1, 1), 0.0, 1.5), (0.25, 0.5, 0.0), (0.0, 0.0, -1.0), c=world_point(c, "tr"))
        s["o"] = world_point((0.25, 0.5, 0.0), "tr")
        s["prims"].append(_aside(1))
        s["mats"] = [s["mats"][0], (L, PALETTE[1], 0.0, 0.0)]
    else:
        s = _ball((D, (1, 1, 1), 0.0, 1.5), (0.25, 0.5, 0.0), (0.0, 0.0, -1.0), wrap="tr")
    prim, o, d = s["prims"][0], s["o"], s["d"]

    def check():
        t, q, steps = q_prim(prim, o, d)
        return Edge(t == q.near and bool(prim.flags & abi.RT_PRIM_HAS_TRANSLATE) != alt, [q.disc])
    return dict(s, check=check)


def metal_probe(kind):
    def fn(alt):
        if kind == "normal":
            s = _ball((M, (0.8, 0.8, 0.8), 0.0, 0.0), (0.0, 0.5 if alt else 0.0, 0.0), (0.0, 0.0, -2.0))
        elif kind == "fuzz1":
            s = _ball((M, (0.8, 0.8, 0.8), 0.0 if alt else 1.0, 0.0), (0.25, 0.5, 0.0), (0.0, 0.0, -1.0))
        else:       # the back face of an XY rect, d.z > 0, going up (alt: going down)
            s = dict(prims=[abi.rect(abi.RT_PRIM_XY_RECT, -500.0, 500.0, -500.0, 500.0, -4.0, 0)], o=(0.0, 0.0, -80.0),
                     d=(0.0, -20.0 if alt else 20.0, 21.0), mats=[(M, (0.8, 0.8, 0.8), 0.0, 0.0)])
        prim, o, d = s["prims"][0], s["o"], s["d"]

        def check():
            t, q, steps = q_prim(prim, o, d)
            if kind == "normal":
                return Edge(t == q.near == 2 and o[:2] == (0.0, 0.0), steps)
            if kind == "fuzz1":
                return Edge(t == q.near and s["mats"][0][2] == 1.0, [q.disc])
            return Edge(q.hit and d[2] > 0, [])      # (a configuration, not a boundary)
        return dict(s, check=check)
    fn.__doc__ = {
        "normal": "Metal with fuzz = 0 at normal incidence: reflect(unit(d), n) = -unit(d) exactly, d . n = 1 > 0 (metal.rs:26-43, "
                  "vec3.rs:412-414); the sky at unit.y = 0.  max_depth 2.  alt: an oblique hit.",
        "fuzz1": "Metal with fuzz = 1: reflected + 1 x random_in_unit_sphere; the samples whose direction ends below the surface "
                 "are ABSORBED and black, not re-drawn (metal.rs:38-42).  max_depth 2.  alt: fuzz = 0.",
        "back_face": "Metal on a rect's BACK face (dir.z > 0): the normal is -e_z, the ray is reflected back down -z and keeps its "
                     "d.y; with the normal not flipped, `dot(dir, normal) < 0` would absorb it (metal.rs:30-42, xy_rect.rs:43-45).  "
                     "max_depth 2.  alt: d.y negated (the reflected ray's sky colour follows).",
    }[kind]
    return fn


add("diel_head_on", "diel_head_on", SPHERES, diel_head_on, depth=3)
add("diel_below_critical", "diel_critical", RECTS, diel_critical(False), depth=2)
add("diel_above_critical", "diel_critical", RECTS, diel_critical(True), depth=2)
add("diel_ior_1", "diel_ior_1", SPHERES, diel_ior(1.0), depth=3)
add("diel_ior_below_1", "diel_ior_below_1", SPHERES, diel_ior(0.5), depth=3)
add("diel_translate_back_face", "diel_translate", ANY, diel_translate_back, depth=3)
add("metal_normal_incidence", "metal_normal", SPHERES, metal_probe("normal"), depth=2)
add("metal_back_face", "metal_back_face", RECTS, metal_probe("back_face"), depth=2)
add("metal_fuzz_1", "metal_fuzz_1", SPHERES, metal_probe("fuzz1"), depth=2)
# (Lambertian on each rect face: rect_front_face[*] and rect_back_face[*] above)

CASES = [(name, route) for name, probe in PROBES.items() for route in probe.routes]


# ---- guides ------------------------------------------------------------------------------------------------------------------

def oracle_guides(orc, probe, alt=False):
    """tests/denoise_model.py: oracle_guides' normal, position and obj_id planes (one ray per pixel through its centre, at the
    middle of the shutter interval, the first hit over [0.001, inf)), with the oracle's LINEAR scan for every probe, like
    oracle_frame above; held to denoise_model.oracle_guides itself in tests/test_ray_probes_cpu.py."""
    import ctypes as C
    bundle, cam = probe.bundle(alt), probe.camera(alt)
    w, h, _ = probe.guide_shape()
    lib = orc.lib()
    scene = lib.orc_scene_build(C.byref(bundle.desc), 0, 1)
    g = {"normal": np.zeros((h, w, 3)), "position": np.zeros((h, w, 3)), "obj_id": np.full((h, w), -1, dtype=np.int32)}
    o = np.array(cam.origin[:])
    ulc, hor, ver = np.array(cam.upper_left_corner[:]), np.array(cam.horizontal[:]), np.array(cam.vertical[:])
    time = (cam.time_a + cam.time_b) * 0.5
    hit = orc.OrcHit()
    try:
        for py in range(h):
            for px in range(w):
                d = ulc + (px + 0.5) / (w - 1) * hor - (py + 0.5) / (h - 1) * ver - o
                if lib.orc_scene_hit_time(scene, orc.d3(o), orc.d3(d), time, T_MIN, INF, C.byref(hit)):
                    g["normal"][py, px], g["position"][py, px], g["obj_id"][py, px] = hit.normal[:], hit.point[:], hit.obj_id
    finally:
        lib.orc_scene_free(scene)
    return g
