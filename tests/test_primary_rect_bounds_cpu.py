"""The pixel rectangle of every rect record (racer-tracer_amd/csrc/rt_primary_bounds.h: primary_rect_bounds,
primary_rects), on the CPU: tests/primary_rect_bounds_driver.cpp is compiled with the host compiler and answers a list
of cases.  The camera batches of the rects-only plain trace kernel step over a record in the items none of whose pixels
lies inside the record's rectangle, so a rectangle must be CONSERVATIVE — and whatever the host cannot tell must switch
the whole thing off.

1. Conservative: for every pixel outside a rect's rectangle no ray through the pixel's four jitter corners or 16 seeded
   jitters passes the reference's rect test (xy_rect.rs:28-48, numpy, f64): 240 seeded cameras (outside, near, inside,
   looking away) x scenes of one to five random rects, frames 33x21 and 64x40.
2. Every doubt gives the whole frame: a corner on or behind the camera plane, an aperture, a non-finite input, reversed
   bounds, a scene rectangle that is the whole frame, more records than RT_PRIMARY_RECTS.
3. Not vacuous: with C3's camera at 1920x1080 the 16 900 unculled tiles see 1 (13 222), 2 (3 670) or 3 (8) of cornell's
   six rects.
4. primary_bounds itself is held by tests/test_primary_bounds_cpu.py, unchanged."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import primary_bounds_model as M
import scenes_py as S
from test_primary_bounds_cpu import _cam, _random_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RECTS = 16   # rt_primary_bounds.h: RT_PRIMARY_RECTS
T_MIN = 0.001  # renderer.rs:56
AXIS_OF_KIND = {S.abi.RT_PRIM_XY_RECT: 2, S.abi.RT_PRIM_XZ_RECT: 1, S.abi.RT_PRIM_YZ_RECT: 0}


def _fmt(x):
    x = float(x)
    return "nan" if math.isnan(x) else ("inf" if x > 0 else "-inf") if math.isinf(x) else x.hex()


def _box_of(rects):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for axis, a0, a1, b0, b1, k in rects:
        ia, ib = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
        p0, p1 = np.zeros(3), np.zeros(3)
        p0[axis] = p1[axis] = k
        p0[ia], p1[ia], p0[ib], p1[ib] = a0, a1, b0, b1
        lo, hi = np.minimum(lo, np.minimum(p0, p1)), np.maximum(hi, np.maximum(p0, p1))
    return tuple(lo), tuple(hi)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("primary_rect_bounds") / "primary_rect_bounds_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "racer-tracer_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "primary_rect_bounds_driver.cpp")], check=True)

    def run(cases):
        """cases: list of dict(cam, w, h, rects[, box, lens_radius, force]) -> list of (n, scene rect, [N_RECTS rectangles])"""
        lines = []
        for c in cases:
            mn, mx = c.get("box") or _box_of(c["rects"])
            head = M.case_line(c["cam"], c["w"], c["h"], mn, mx, c.get("lens_radius"))
            tail = " ".join(" ".join(_fmt(v) for v in r) for r in c["rects"])
            lines.append("%s %d %d %s" % (head, 1 if c.get("force") else 0, len(c["rects"]), tail))
        out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(cases)
        answers = []
        for line in out:
            v = [int(x) for x in line.split()]
            assert len(v) == 5 + 4 * N_RECTS
            answers.append((v[0], tuple(v[1:5]), [tuple(v[5 + 4 * i:9 + 4 * i]) for i in range(N_RECTS)]))
        return answers
    return run


def _jitters():
    """(ju, jv) of a pixel: its four corners (the largest double below 1 stands for the open end) and 16 seeded draws."""
    top = 1.0 - 2.0 ** -53
    rng = np.random.default_rng(20261019)
    return np.concatenate([np.array([(0.0, 0.0), (top, 0.0), (0.0, top), (top, top)]), rng.random((16, 2))])


JITTERS = _jitters()


def _pixels_hit(cam, w, h, rect):
    """bool [h][w]: some sampled ray of the pixel passes the reference's rect test (xy_rect.rs:28-48) of `rect`."""
    axis, a0, a1, b0, b1, k = rect
    ia, ib = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    px, py = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    hit = np.zeros((h, w), dtype=bool)
    o = cam["origin"]
    for ju, jv in JITTERS:
        u = (px + ju) / float(w - 1)                                # cpu.rs:35-36
        v = (py + jv) / float(h - 1)                                # cpu.rs:39-40
        d = (cam["ulc"][None, None, :] + u[None, :, None] * cam["horizontal"][None, None, :]
             - v[:, None, None] * cam["vertical"][None, None, :] - o[None, None, :])   # camera.rs:331
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (k - o[axis]) / d[..., axis]
            a = o[ia] + t * d[..., ia]
            b = o[ib] + t * d[..., ib]
            miss = (t < T_MIN) | (t > np.inf) | (a < a0) | (a > a1) | (b < b0) | (b > b1)   # (a NaN passes, as in the reference)
        hit |= ~miss
    return hit


def _inside(rectangle, w, h):
    px0, px1, py0, py1 = rectangle
    m = np.zeros((h, w), dtype=bool)
    if px0 <= px1 and py0 <= py1:
        m[py0:py1 + 1, px0:px1 + 1] = True
    return m


def _random_rects(rng):
    rects = []
    for _ in range(int(rng.integers(1, 6))):
        axis = int(rng.integers(0, 3))
        a0, b0 = rng.uniform(-300.0, 300.0, 2)
        rects.append((axis, a0, a0 + rng.uniform(1.0, 400.0), b0, b0 + rng.uniform(1.0, 400.0), rng.uniform(-300.0, 300.0)))
    return rects


def test_rectangles_are_conservative(driver):
    rng = np.random.default_rng(20261020)
    cases, kinds = [], []
    for i in range(240):
        kind = ("outside", "near", "inside", "away")[i % 4]
        rects = _random_rects(rng)
        mn, mx = (np.array(v) for v in _box_of(rects))   # (one rect: a flat box; the camera is placed by its diagonal all the same)
        spec = _random_camera(rng, kind, mn, mx)
        for w, h in ((33, 21), (64, 40)):
            cases.append(dict(cam=_cam(spec, w, h), w=w, h=h, rects=rects))
            kinds.append(kind)
    proper = 0
    for case, kind, (n, scene, rectangles) in zip(cases, kinds, driver(cases)):
        w, h = case["w"], case["h"]
        whole = (0, w - 1, 0, h - 1)
        assert n in (0, len(case["rects"]))
        if scene == whole:
            assert n == 0
        if n == 0:
            assert all(r == whole for r in rectangles)
        assert all(r == whole for r in rectangles[len(case["rects"]):])
        for rect, rectangle in zip(case["rects"], rectangles):
            assert 0 <= rectangle[0] <= w and -1 <= rectangle[1] <= w - 1 and 0 <= rectangle[2] <= h and -1 <= rectangle[3] <= h - 1
            seen_outside = _pixels_hit(case["cam"], w, h, rect) & ~_inside(rectangle, w, h)
            assert not seen_outside.any(), (kind, w, h, rect, rectangle, np.argwhere(seen_outside)[:4])
            # inside the scene's own rectangle, up to the shared rounding
            if n:
                assert rectangle[0] >= scene[0] and rectangle[1] <= scene[1] and rectangle[2] >= scene[2] and rectangle[3] <= scene[3]
        if kind == "inside":
            assert n == 0
        if kind == "outside" and (w, h) == (64, 40):
            # the scene spans under 19 of at least 40 degrees (tests/test_primary_bounds_cpu.py): no rect's rectangle is the frame
            assert n == len(case["rects"]) and all(r != whole for r in rectangles[:n])
            proper += 1
    assert proper == 60


def test_every_doubt_gives_the_whole_frame(driver):
    ahead = dict(look_from=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, 10.0), vfov=40.0, aperture=0.0, focus_distance=10.0)
    good = (2, -2.0, 2.0, -2.0, 2.0, 20.0)   # an XY rect 20 in front of `ahead`
    c3_rects = [(AXIS_OF_KIND[p.kind], p.p[0], p.p[1], p.p[2], p.p[3], p.p[4]) for p in list(S.cornell_box()[0].primitives)[:6]]
    for w, h in ((64, 40), (1920, 1080)):
        whole = (0, w - 1, 0, h - 1)
        cam, c3 = _cam(ahead, w, h), _cam(M.C3_CAMERA, w, h)
        # ---- the rect's own doubts, beside a good rect that keeps its rectangle (the scene's rectangle is forced proper)
        for name, bad in (("a corner on the camera plane", (1, -2.0, 2.0, 0.0, 20.0, -1.0)),
                          ("a corner behind the camera plane", (1, -2.0, 2.0, -5.0, 20.0, -1.0)),
                          ("a rect behind the camera", (2, -2.0, 2.0, -2.0, 2.0, -20.0)),
                          ("a NaN bound", (2, math.nan, 2.0, -2.0, 2.0, 20.0)),
                          ("an infinite bound", (2, -2.0, math.inf, -2.0, 2.0, 20.0)),
                          ("an infinite plane", (2, -2.0, 2.0, -2.0, 2.0, math.inf)),
                          ("reversed bounds", (2, 2.0, -2.0, -2.0, 2.0, 20.0)),
                          ("no such axis", (3, -2.0, 2.0, -2.0, 2.0, 20.0))):
            (n, scene, rectangles), = driver([dict(cam=cam, w=w, h=h, rects=[good, bad], box=((-2.0, -2.0, 20.0), (2.0, 2.0, 20.0)), force=True)])
            assert n == 2 and rectangles[0] != whole and rectangles[1] == whole, name
        # ---- the render's doubts: the scene's rectangle is the whole frame, so every rectangle is, and n says "off"
        for name, case in (("an aperture", dict(cam=c3, w=w, h=h, rects=c3_rects, lens_radius=15.0)),
                           ("a camera inside the box", dict(cam=_cam(dict(M.C3_CAMERA, look_from=(278.0, 278.0, 100.0), look_at=(278.0, 278.0, 555.0)), w, h),
                                                            w=w, h=h, rects=c3_rects)),
                           ("a decoy behind the camera", dict(cam=c3, w=w, h=h, rects=c3_rects + [(2, 0.0, 1e-6, 0.0, 1e-6, -1e7)])),
                           ("a non-finite camera", dict(cam=dict(c3, ulc=np.array([math.nan, 0.0, 0.0])), w=w, h=h, rects=c3_rects)),
                           ("a non-finite scene box", dict(cam=c3, w=w, h=h, rects=c3_rects, box=((0.0, 0.0, 0.0), (555.0, math.inf, 555.0)))),
                           ("more records than rectangles", dict(cam=c3, w=w, h=h, rects=c3_rects + [c3_rects[0]] * (N_RECTS + 1 - len(c3_rects)))),
                           ("no rect at all", dict(cam=c3, w=w, h=h, rects=[], box=M.CORNELL_BOX))):
            (n, scene, rectangles), = driver([case])
            assert n == 0 and all(r == whole for r in rectangles), name
            if name not in ("more records than rectangles", "no rect at all"):
                assert scene == whole, name
        # ---- and the plain scene, as many records as there are rectangles: on
        (n, scene, rectangles), = driver([dict(cam=c3, w=w, h=h, rects=c3_rects + [c3_rects[0]] * (N_RECTS - len(c3_rects)))])
        assert n == N_RECTS and scene != whole and all(r != whole for r in rectangles)
    # a frame narrower than two pixels
    (n, scene, rectangles), = driver([dict(cam=_cam(M.C3_CAMERA, 1, 40), w=1, h=40, rects=c3_rects)])
    assert n == 0 and all(r == (0, 0, 0, 39) for r in rectangles)


def tile_histogram(scene, rectangles, w, h):
    """{rects seen: tiles} over the 8x8 tiles that have a pixel inside the scene's rectangle (whole tiles rows: a tile's
    pixels are its box)."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    x0, y0 = np.arange(tx) * 8, np.arange(ty) * 8
    x1, y1 = np.minimum(x0 + 7, w - 1), np.minimum(y0 + 7, h - 1)

    def overlaps(r):
        return ((x1 >= r[0]) & (x0 <= r[1]))[None, :] & ((y1 >= r[2]) & (y0 <= r[3]))[:, None]
    count = sum(overlaps(r).astype(int) for r in rectangles)
    values, tiles = np.unique(count[overlaps(scene)], return_counts=True)
    return dict(zip(values.tolist(), tiles.tolist()))


def test_c3_tiles_see_one_rect_mostly(driver):
    w, h = 1920, 1080
    rects = [(AXIS_OF_KIND[p.kind], p.p[0], p.p[1], p.p[2], p.p[3], p.p[4]) for p in list(S.cornell_box()[0].primitives)[:6]]
    (n, scene, rectangles), = driver([dict(cam=_cam(M.C3_CAMERA, w, h), w=w, h=h, rects=rects)])
    assert n == 6
    hist = tile_histogram(scene, rectangles[:n], w, h)
    print(scene, rectangles[:n], hist)
    assert hist == {1: 13222, 2: 3670, 3: 8}
    assert sum(k * v for k, v in hist.items()) / sum(hist.values()) < 1.23


@pytest.mark.parametrize("w,h", [(128, 24), (64, 40), (61, 21)])
def test_the_gpu_tests_shapes_have_tiles_with_a_proper_mask(driver, w, h):
    """What tests/test_gpu_primary_masks.py relies on: tiles that see some but not all of the six rects."""
    rects = [(AXIS_OF_KIND[p.kind], p.p[0], p.p[1], p.p[2], p.p[3], p.p[4]) for p in list(S.cornell_box()[0].primitives)[:6]]
    (n, scene, rectangles), = driver([dict(cam=_cam(M.C3_CAMERA, w, h), w=w, h=h, rects=rects)])
    hist = tile_histogram(scene, rectangles[:n], w, h)
    print(w, h, hist)
    assert n == 6 and sum(v for k, v in hist.items() if 0 < k < 6) > 0
