"""What keeps tests/test_gpu_texture_edges.py honest, without a GPU: conditions on the probes' inputs, checked on the oracle
alone.  A probe is only worth rendering if its lookups reach the edge it is named after, and if the oracle's frame moves when
the thing it guards is broken.  The counts measured when the probes were written (seed 1) stand beside each floor; if a
count falls short after a shape changes, enlarge the frame, do not lower the floor."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_texture_edges as G
import texture_probes as P

abi = P.abi
# rt_trace_common.h: RT_UV_EPS_U, RT_UV_EPS_V and the pole threshold of prim_hit_record
UV_EPS_U, UV_EPS_V, POLE_CAP = 5e-7, 2e-6, 2.0 ** -10


@pytest.fixture(scope="module")
def hits(orc):
    cache = {}

    def get(name):
        if name not in cache:
            probe = P.PROBES[name]
            bundle = probe.build()
            cache[name] = (bundle, P.first_hits(orc, bundle, P.camera(orc, probe), P.params(probe)))
        return cache[name]
    return get


def _frame(orc, name, **override):
    probe = P.PROBES[name]
    frame, segments = P.oracle_frame(orc, probe, probe.build(**override))
    w, h, spp = probe.shape
    assert segments == w * h * spp      # one segment per sample at max_depth = 1
    return frame


# ---- the table ---------------------------------------------------------------------------------------------------------------

def test_every_probe_runs_on_every_route_of_its_row():
    assert G.CASES == P.CASES and len(set(P.CASES)) == len(P.CASES)
    for name, probe in P.PROBES.items():
        want = P.EXACT_ROUTES if name == "checker_zero_plane" else P.ALL_ROUTES
        assert probe.routes == want, name
    assert set(P.ALL_ROUTES) == {"pool-fast", "pool-fast-bvh", "pool-exact", "v1-fast", "v1-exact", "guides"}
    for name in ["image_equator", "image_seam", "image_pole_up", "image_pole_down", "image_shell", "image_inside", "image_wrapped", "image_moving",
                 "images_two_sizes", "noise_two_tables", "noise_two_tables_shuffled", "noise_room", "noise_big_argument",
                 "noise_wave", "checker_room", "checker_room_negative", "checker_zero_plane"] + \
                ["noise_depth[%d]" % d for d in (0, 1, 8, 9, 10, 16, 24)]:
        assert name in P.PROBES, name
    assert P.ROUTES["pool-exact"].exact and P.ROUTES["v1-exact"].exact


def test_every_probe_selects_the_kernel_class_it_is_described_with(rt):
    want = {"image_wrapped": 2, "image_moving": 2}
    for name, probe in P.PROBES.items():
        got = rt.classify(probe.build())
        assert got["textured"] == 1 and got["specular"] == 0, name
        assert got["prims_class"] == want.get(name, 1 if name.startswith("image_") else 0), name
        assert rt.classify(probe.build(fillers=True))["textured"] == 1


# ---- first_hits against the oracle's own camera ------------------------------------------------------------------------------

def test_primary_rays_are_the_oracles(orc):
    probe = P.PROBES["image_moving"]
    cam, prm = P.camera(orc, probe), P.params(probe)
    px, py, sample, dirs, time = P.primary_rays(cam, prm)
    w, h, spp = probe.shape
    assert len(px) == w * h * spp
    lib = orc.lib()
    ulc, hor, ver, org = (np.array(x[:]) for x in (cam.upper_left_corner, cam.horizontal, cam.vertical, cam.origin))
    for i in list(range(0, len(px), 997)) + [len(px) - 1]:
        x, y, s = int(px[i]), int(py[i]), int(sample[i])
        assert (y * w + x) * spp + s == i
        u = lib.orc_pixel_u(C.byref(prm), x, y)
        v = (y + lib.orc_rng_double(prm.seed, y * w + x, s, 0, P.RT_RNG_CAMERA, 0, 0)) / (h - 1)
        assert np.array_equal(dirs[i], ((ulc + hor * u) - ver * v) - org)
        assert time[i] == cam.time_a + (cam.time_b - cam.time_a) * lib.orc_rng_double(prm.seed, y * w + x, s, 0, P.RT_RNG_CAMERA, 0, 1)


@pytest.mark.parametrize("name", ["image_moving", "images_two_sizes", "noise_wave"])
def test_a_probe_pixel_is_the_root_of_the_mean_first_hit_texture(orc, hits, name):
    """The fact every probe rests on, and first_hits as a whole (time included: the MovingSphere) against orc_render."""
    bundle, fh = hits(name)
    probe = P.PROBES[name]
    frame = P.frame_from_samples(P.texture_values(orc, bundle, fh), P.params(probe))
    assert np.array_equal(frame, _frame(orc, name))


# ---- the image probes reach their edges --------------------------------------------------------------------------------------

def _boundary_distance(fh):
    """Distance of u W and v H from the nearest cell boundary, in cells, for every first hit."""
    u, v = fh.rec["u"][fh.hit], fh.rec["v"][fh.hit]
    fu, fv = (u * P.IMAGE_W) % 1.0, (v * P.IMAGE_H) % 1.0
    return np.minimum(fu, 1.0 - fu), np.minimum(fv, 1.0 - fv)


def test_image_equator_reaches_both_arms_of_the_certification(hits):
    _, fh = hits("image_equator")
    du, dv = _boundary_distance(fh)
    band = (du < UV_EPS_U * P.IMAGE_W) | (dv < UV_EPS_V * P.IMAGE_H)
    near = (du < 1e-7 * P.IMAGE_W) | (dv < 1e-7 * P.IMAGE_H)
    print("image_equator: %d first hits, %d in the band, %d within 1e-7, %d outside" % (fh.hit.sum(), band.sum(), near.sum(), (~band).sum()))
    assert band.sum() >= 100        # measured 161 of 25 860
    assert near.sum() >= 10         # measured 17
    assert (~band).sum() >= 20000   # measured 25 699


def test_image_seam_reaches_both_ends_of_u(hits):
    _, fh = hits("image_seam")
    u = fh.rec["u"][fh.hit]
    print("image_seam: %d lookups at the seam, u in [%g, %g]" % (((u < 1e-3) | (u > 1 - 1e-3)).sum(), u.min(), u.max()))
    assert ((u < 1e-3) | (u > 1.0 - 1e-3)).sum() >= 100     # measured 180
    assert (u < 1e-3).sum() >= 20 and (u > 1.0 - 1e-3).sum() >= 20


@pytest.mark.parametrize("name", ["image_pole_up", "image_pole_down"])
def test_image_poles_reach_both_sides_of_the_f64_switch(hits, name):
    _, fh = hits(name)
    ny = fh.rec["point"][fh.hit][:, 1]      # the unit sphere at the origin: the outward normal is the point
    cap = 1.0 - ny * ny < POLE_CAP
    print("%s: %d inside the cap, %d outside" % (name, cap.sum(), (~cap).sum()))
    assert cap.sum() >= 1000 and (~cap).sum() >= 10000      # measured 1 448 and 64 088
    v = fh.rec["v"][fh.hit]
    assert (v.max() > 0.999) if name == "image_pole_up" else (v.min() < 0.001)


def test_image_shell_wrapped_and_moving_are_what_they_say(hits):
    bundle, fh = hits("image_shell")
    # radius -1 seen from inside: front faces, and the outward normal points at the centre
    assert fh.hit.all() and fh.rec["front_face"].all() and np.allclose(fh.rec["normal"], -fh.rec["point"], atol=1e-12)
    bundle, fh = hits("image_inside")
    # radius 1 seen from inside: back faces, the normal is flipped (and the kernel's exact-uv lambda un-flips it)
    assert fh.hit.all() and not fh.rec["front_face"].any() and np.allclose(fh.rec["normal"], -fh.rec["point"], atol=1e-12)
    bundle, fh = hits("image_wrapped")
    assert bundle.primitives[0].flags == abi.RT_PRIM_HAS_ROTATE_Y | abi.RT_PRIM_HAS_TRANSLATE and fh.hit.sum() >= 20000
    bundle, fh = hits("image_moving")
    assert bundle.primitives[0].kind == abi.RT_PRIM_MOVING_SPHERE and fh.hit.sum() >= 10000
    assert fh.time.min() < 0.01 and fh.time.max() > 0.99


def test_images_two_sizes_shows_every_image(orc, hits):
    bundle, fh = hits("images_two_sizes")
    assert [(bundle.images[i].width, bundle.images[i].height) for i in range(3)] == [(1, 1), (7, 1), (5, 3)]
    ids = fh.rec["obj_id"][fh.hit]
    assert all((ids == k).sum() >= 1000 for k in (1, 2, 3))
    values = P.texture_values(orc, bundle, fh)
    for k, texels in ((1, 1), (2, 7), (3, 15 + 1)):     # every texel of every image is looked up (+ the Checkered's solid side)
        seen = {tuple(x) for x in values[fh.hit & (fh.rec["obj_id"] == k)]}
        assert len(seen) == texels, (k, len(seen))


# ---- the noise probes ----------------------------------------------------------------------------------------------------------

def _changed(a, b):
    d = np.abs(a - b).max(axis=-1)
    return float((d > 1e-3).mean()), float(d.max())


SENSITIVE = [
    ("noise_depth[9]", dict(depth=8)),          # the second pass of the octave loop dropped: measured 23 %, max 0.005
    ("noise_depth[1]", dict(depth=0)),          # 97 %
    ("noise_two_tables", dict(table1=0)),       # the table-1 texture served from table 0: 48 % (its half of the frame)
    ("noise_two_tables_shuffled", dict(table1=0)),
    ("image_equator", dict(roll=1)),            # the image rolled by one texel: 40 % (the sphere's share of the frame)
    ("checker_room", dict(swap=True)),          # the two colours swapped: 33 %
    ("checker_room_negative", dict(swap=True)),
]


@pytest.mark.parametrize("name,override", SENSITIVE, ids=lambda x: str(x).replace(" ", ""))
def test_the_oracle_sees_what_a_probe_guards(orc, name, override):
    share, worst = _changed(_frame(orc, name), _frame(orc, name, **override))
    print("%s -> %s: %.1f %% of pixels beyond 1e-3, max %g" % (name, override, 100 * share, worst))
    assert share >= 0.10


@pytest.mark.parametrize("name,depth", [("noise_depth[16]", 15), ("noise_depth[24]", 23), ("noise_room", 23)])
def test_the_deep_octaves_are_below_tol(orc, name, depth):
    """Octaves 16 and 24 move the frame by less than TOL (measured 4.3e-5 and 1.6e-7) but by far more than TIGHT: the GPU
    module's RT_ARITH_REFERENCE routes, which hold every pixel to TIGHT, are what decides these probes."""
    share, worst = _changed(_frame(orc, name), _frame(orc, name, depth=depth))
    assert share == 0.0 and worst < G.TOL
    if name == "noise_depth[16]":
        assert worst > 1e3 * G.TIGHT


def test_noise_room_takes_lattice_coordinates_past_the_int_range(orc, hits):
    bundle, fh = hits("noise_room")
    depth = bundle.textures[0].depth
    pts = np.abs(fh.rec["point"][fh.hit])
    assert fh.hit.sum() >= 4000
    # octave o looks up 2^o p: the last one's lattice coordinate saturates `as i32`, and index + 1 wraps
    assert (pts.max(axis=1) * 2.0 ** (depth - 1) > 2.0 ** 31).sum() >= 4000
    frame = _frame(orc, "noise_room")
    assert np.isfinite(frame).all() and frame.std() > 0.1


def test_noise_big_argument_stays_inside_the_documented_range(hits):
    bundle, fh = hits("noise_big_argument")
    arg = bundle.textures[0].scale * fh.rec["point"][fh.hit][:, 2]     # + 10 turb, at most ~20
    assert 8e5 < arg.min() and arg.max() < 1e6


def test_noise_wave_asks_for_more_than_eight_lookups_in_a_wave(hits):
    _, fh = hits("noise_wave")
    count = np.zeros((16, 16), dtype=int)
    np.add.at(count, (fh.py[fh.hit], fh.px[fh.hit]), 1)
    tiles = [int(count[y:y + 8, x:x + 8].sum()) for y in (0, 8) for x in (0, 8)]
    assert max(tiles) > 8 and min(tiles) > 8, tiles     # measured 98 .. 128 Noise first hits per 8x8 tile


# ---- the checker probes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,sign", [("checker_room", 1.0), ("checker_room_negative", -1.0)])
def test_checker_room_reaches_large_arguments_of_both_signs(hits, name, sign):
    _, fh = hits(name)
    pts = fh.rec["point"][fh.hit] * sign
    assert fh.hit.sum() >= 4000 and set(np.unique(fh.rec["obj_id"][fh.hit])) == {1, 2, 3}      # all three orientations
    assert pts.min() > -1e-9 and pts.max() > 554.0 and (10.0 * pts.max(axis=1) > 5000.0).sum() >= 4000


def test_checker_zero_plane_hits_zero_and_its_neighbours(hits):
    _, fh = hits("checker_zero_plane")
    y = fh.rec["point"][fh.hit][:, 1]
    zero, tiny = int((y == 0.0).sum()), int(((y != 0.0) & (np.abs(y) < 1e-15)).sum())
    print("checker_zero_plane: %d first hits with y == 0, %d with 0 < |y| < 1e-15" % (zero, tiny))
    assert zero >= 1000 and tiny >= 100     # measured 5 736 and 924 of 6 660


# ---- the guides route ----------------------------------------------------------------------------------------------------------

def test_guide_hits_are_oracle_guides(orc):
    import denoise_model
    probe = P.PROBES["image_moving"]
    w, h, _ = P.guide_shape(probe)
    bundle, cam = probe.build(), P.camera(orc, probe, (w, h, 1))
    gh = P.guide_hits(orc, bundle, cam, w, h)
    ref = denoise_model.oracle_guides(orc, bundle, cam, w, h)
    assert np.array_equal(np.where(gh.hit, gh.rec["obj_id"], -1).reshape(h, w), ref["obj_id"])
    assert np.array_equal(gh.rec["point"][gh.hit], ref["position"][ref["obj_id"] > 0])


SPHERE_IMAGE_PROBES = [n for n, p in P.PROBES.items() if p.kind == "image" and n != "images_two_sizes"]


@pytest.mark.parametrize("name", SPHERE_IMAGE_PROBES)
def test_guide_lookups_of_the_image_probes_stay_off_the_cell_boundaries(orc, name):
    """texture_probes.guide_shape: with a probe's own square, even frame, lines of pixel centres sit exactly on cell
    boundaries, where the sign of a zero picks the texel; with the guide frame no lookup comes within 1e-9 of a cell of
    one (rounding moves a lookup by ~1e-12 of a cell), and the probe's edge is still in the frame."""
    probe = P.PROBES[name]
    w, h, _ = probe.shape
    if name in ("image_equator", "image_pole_up"):
        even = P.guide_hits(orc, probe.build(), P.camera(orc, probe), w, h)
        du, dv = _boundary_distance(even)
        assert (np.minimum(du, dv) < 1e-9).sum() >= 64      # what the guide frame is there to avoid
    gw, gh_, _ = P.guide_shape(probe)
    assert (gw, gh_) == (w - 1, h - 3)
    fh = P.guide_hits(orc, probe.build(), P.camera(orc, probe, (gw, gh_, 1)), gw, gh_)
    du, dv = _boundary_distance(fh)
    assert fh.hit.sum() >= 4000 and min(du.min(), dv.min()) > 1e-9
    if name.startswith("image_pole"):       # the guides still cross the 2^-10 switch
        ny = fh.rec["point"][fh.hit][:, 1]
        assert (1.0 - ny * ny < POLE_CAP).sum() >= 100 and (1.0 - ny * ny >= POLE_CAP).sum() >= 5000
    if name == "image_seam":
        u = fh.rec["u"][fh.hit]
        assert (u < 2e-3).sum() >= 10 and (u > 1.0 - 2e-3).sum() >= 10
