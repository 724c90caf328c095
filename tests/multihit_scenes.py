"""Scenes and ray sets of the multi-hit query's tests (include/rt_multihit.h).  A helper, not a test file.

The scenes the suite already has are shallow: THE random set of tests/ray_query_model.py reaches 3 to 4 hits per ray at
most, so k = 8 would never truncate on them.  Two additions:

  the STACK scene: six nested spheres of radius 1..6 at C = (0, 0, -10); two MovingSpheres of radius 6.5 and 7 around them
  whose centres move by 0.2 and 0.1 over the shutter; four XY rects over +-8 at z = -2.5, -2, -17.5 and -18; a box of
  +-0.3 around C and a box over +-8 from z = -20 to -19; 16 filler spheres of radius 0.4 around (40, 0, -10), which give
  the tree some depth.  Forms: "stack" (linear), "stack-tree" (the same primitives behind a tree) and "stack-wrapped" (a
  tree; the sphere of radius 3 stands inside a Translate and the small box inside a RotateY and a Translate, as
  variant_scenes.wrap builds them).
  Its ray set (stack_rays): of every four rays, two go from around (0, 0, 5) to targets within 2 of C — they pass 11 to 14
  primitives — one goes to a target within 16 of C, so that short and empty lists occur, and one starts inside the
  nest, within 0.9 of C, so that spheres answer with their far root.

  the PAIR set on the scenes of ray_query_model.SCENES: rays through two hit points P of THE random set that lie on two
  different primitives, o = P[a] - 2 (P[b] - P[a]), d = P[b] - P[a]: a ray that is known to pass two primitives, at t = 2
  and t = 3, and usually more.  (With a and b drawn freely, both points lie on the ground sphere of the sphere-only forms
  too often: fewer than 0.05 of the rays then passed more than two primitives.)
"""
import math

import numpy as np

import multihit_model as M
import ray_query_model as Q
import variant_scenes as V

abi = Q.abi
SEED_PAIR, SEED_STACK = 2028, 2029
CENTRE = (0.0, 0.0, -10.0)
STACKS = ["stack", "stack-tree", "stack-wrapped"]
N = 256      # what the tests use; 64 on large_bvh (3000 primitives)


def n_for(name):
    return 64 if name == "large_bvh" else N


def stack_scene(name):
    """-> (numbered bundle, closest_hit option, tree in LDS or None: no tree)."""
    T = V._Tables()
    grey = T.mat(V.L, T.tex(abi.solid((0.6, 0.6, 0.55))))
    glass = T.mat(V.D, -1, ior=1.5)
    wrapped = name == "stack-wrapped"
    prims = []
    for r in range(1, 7):
        if wrapped and r == 3:
            s = abi.sphere((0.0, 0.0, 0.0), 3.0, glass)
            s.flags = abi.RT_PRIM_HAS_TRANSLATE
            s.translate = abi.D3(*CENTRE)
            prims.append(s)
        else:
            prims.append(abi.sphere(CENTRE, float(r), glass if r % 2 else grey))
    prims.append(abi.moving_sphere(CENTRE, (0.0, 0.2, -10.0), 6.5, glass, 0, 0.0, 1.0))
    prims.append(abi.moving_sphere(CENTRE, (0.1, 0.0, -10.0), 7.0, grey, 0, 0.0, 1.0))
    for z in (-2.5, -2.0, -17.5, -18.0):
        prims.append(abi.rect(abi.RT_PRIM_XY_RECT, -8, 8, -8, 8, z, grey))
    if wrapped:
        prims.append(V.wrap(abi.box((-0.3, -0.3, -0.3), (0.3, 0.3, 0.3), grey), 25.0, CENTRE))
    else:
        prims.append(abi.box((-0.3, -0.3, -10.3), (0.3, 0.3, -9.7), grey))
    prims.append(abi.box((-8.0, -8.0, -20.0), (8.0, 8.0, -19.0), grey))
    for i in range(16):
        a = 2.0 * math.pi * i / 16
        prims.append(abi.sphere((40.0 + 3.0 * math.cos(a), 3.0 * math.sin(a), -10.0), 0.4, grey))
    bundle = Q.number(abi.SceneBundle(prims, T.materials, T.textures, abi.sky()))
    tree = name != "stack"
    return bundle, (abi.RT_HIT_BVH if tree else abi.RT_HIT_AUTO), (1 if tree else None)


def stack_rays(n=N):
    """-> origin [n, 3], direction [n, 3], time [n]; ray i is of kind i % 4: 0, 1 base, 2 wide, 3 from inside the nest."""
    rng = np.random.default_rng(SEED_STACK)
    c = np.array(CENTRE)
    kind = np.arange(n) % 4
    origin = np.array([0.0, 0.0, 5.0]) + rng.uniform(-1, 1, (n, 3))
    spread = np.where(kind == 2, 16.0, 2.0)[:, None]
    target = c + rng.uniform(-1, 1, (n, 3)) * spread
    inside = c + rng.uniform(-1, 1, (n, 3)) * 0.5      # within 0.87 of C: inside every sphere of the nest
    away = rng.uniform(-1, 1, (n, 3)) + np.array([0.0, 0.0, -2.0])      # mostly towards -z, where the far rects and the slab are
    origin = np.where((kind == 3)[:, None], inside, origin)
    direction = np.where((kind == 3)[:, None], away, target - origin)
    time = rng.uniform(0, 1, n)
    return np.ascontiguousarray(origin), np.ascontiguousarray(direction), time


def pair_rays(points, prims, n):
    """The pair set through `points` [m, 3], hit points on the primitives `prims` [m] (at least two different ones): ray i
    goes through point a_i and a point b_i of ANOTHER primitive.  -> origin, direction [n, 3], time [n]."""
    rng = np.random.default_rng(SEED_PAIR)
    m = len(points)
    a = rng.integers(0, m, n)
    pick = rng.uniform(0, 1, n)
    time = rng.uniform(0, 1, n)
    b = np.zeros(n, dtype=np.int64)
    for i in range(n):
        others = np.nonzero(prims != prims[a[i]])[0]
        b[i] = others[int(pick[i] * len(others))]
    direction = points[b] - points[a]
    origin = points[a] - 2.0 * direction
    return np.ascontiguousarray(origin), np.ascontiguousarray(direction), time


def scene(name):
    """-> (numbered bundle, closest_hit, in_lds) of a stack form or a scene of ray_query_model.SCENES."""
    if name in STACKS:
        return stack_scene(name)
    bundle, _cam, _spread, closest_hit, in_lds = Q.scene(name)
    return bundle, closest_hit, in_lds


def ray_set(orc, name, which):
    """-> dict(bundle, closest_hit, in_lds, origin, direction, time, lists): the set `which` — "A" THE random set, "pair", or
    "stack" — on the scene, with multihit_model.hit_lists over the default window.  Arrays are read-only."""
    bundle, closest_hit, in_lds = scene(name)
    n = n_for(name)
    if which == "stack":
        o, d, time = stack_rays(n)
    else:
        _b, cam, spread, _c, _l = Q.scene(name)
        o, d, time = Q.random_rays(cam, n, spread)
        if which == "pair":
            first = Q.expected(orc, bundle, o, d, time=time)
            hit = first["prim"] >= 0
            o, d, time = pair_rays(first["point"][hit], first["prim"][hit], n)
    lists = M.hit_lists(orc, bundle, o, d, time=time)
    for a in (o, d, time):
        a.setflags(write=False)
    return dict(bundle=bundle, closest_hit=closest_hit, in_lds=in_lds, origin=o, direction=d, time=time, lists=lists)


def sets_of(name):
    return ("stack",) if name in STACKS else ("A", "pair")


ALL_SCENES = Q.SCENES + STACKS
