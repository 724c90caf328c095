"""Probe scenes that take the texture code to its numerical edges, and per-sample oracle helpers.

A probe is a tiny scene rendered with max_depth = 1 over a black solid background.  With these settings a pixel is
sqrt(mean over samples of the first hit's texture value) (renderer.rs:48-55: albedo x white at depth 0), so a wrong
texture value cannot average away through bounces.  tests/test_texture_probes_cpu.py checks on the oracle alone that each
probe reaches the edge it is here for; tests/test_gpu_texture_edges.py renders every probe through every route that has
texture code of its own.

PROBES is the table: name -> Probe(kind, shape, camera, build, routes).  `kind` decides the assertion of the GPU test
("image": no pixel beyond TOL; "noise" / "checker": every pixel within TOL, the bulk within TIGHT), `routes` the routes the
probe runs on (ALL_ROUTES unless the probe's docstring says why not).

first_hits() restates the camera of oracle/trace.c (orc_pixel_u, orc_sample_radiance_u, get_ray) with a numpy Philox of
include/rt_rng.h's contract, so that the rays of a whole frame are formed at once; test_texture_probes_cpu.py holds it to
orc_pixel_u and orc_rng_double.
"""
import ctypes as C
import functools
import math
from collections import namedtuple

import numpy as np

import scenes_py as S
import variant_scenes as V

abi = S.abi
L = abi.RT_MAT_LAMBERTIAN

# ---- routes ----------------------------------------------------------------------------------------------------------------
# name -> Scene options, and what scene.variant() must then report (checked before any comparison)
Route = namedtuple("Route", "kernel arithmetic closest_hit exact")
ROUTES = {
    # texture_value_deferred, the texture table in LDS, a plain sphere's (u, v) in f32 with certification
    "pool-fast": Route(abi.RT_KERNEL_POOL, abi.RT_ARITH_FAST, abi.RT_HIT_LINEAR, 0),
    # ... the texture table in global memory (the tree's forms are PRIMS_ANY, whatever the scene holds)
    "pool-fast-bvh": Route(abi.RT_KERNEL_POOL, abi.RT_ARITH_FAST, abi.RT_HIT_BVH, 0),
    "pool-exact": Route(abi.RT_KERNEL_POOL, abi.RT_ARITH_REFERENCE, abi.RT_HIT_LINEAR, 1),
    # texture_value_full
    "v1-fast": Route(abi.RT_KERNEL_V1, abi.RT_ARITH_FAST, abi.RT_HIT_LINEAR, 0),
    "v1-exact": Route(abi.RT_KERNEL_V1, abi.RT_ARITH_REFERENCE, abi.RT_HIT_LINEAR, 1),
    # texture_value_full with no LDS gradients: the albedo plane of render_guides, one ray per pixel
    "guides": None,
}
ALL_ROUTES = tuple(ROUTES)
EXACT_ROUTES = ("pool-exact", "v1-exact")

Probe = namedtuple("Probe", "kind shape cam build routes")
BLACK = (0.0, 0.0, 0.0)
IMAGE_W, IMAGE_H = 2048, 1024


@functools.lru_cache(maxsize=None)
def big_image():
    """2048 x 1024 texels of random RGB: a neighbouring texel differs by ~0.3 per channel, so a mis-selected one shows."""
    img = np.random.default_rng(3).integers(0, 256, size=(IMAGE_H, IMAGE_W, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


def small_image(w, h, seed):
    img = np.random.default_rng(seed).integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    img[..., 3] = 255
    return np.ascontiguousarray(img)


def image_texture(index):
    return abi.RtTexture(abi.RT_TEX_IMAGE, -1, -1, index, -1, 0, abi.D3(0, 0, 0), 0.0)


def noise_texture(table, depth, scale=4.0):
    return abi.RtTexture(abi.RT_TEX_NOISE, -1, -1, -1, table, depth, abi.D3(0.9, 0.8, 0.7), scale)


def checker_texture(even, odd):
    return abi.RtTexture(abi.RT_TEX_CHECKERED, even, odd, -1, -1, 0, abi.D3(0, 0, 0), 0.0)


def _bundle(prims, textures, images=(), perlins=(), fillers=False):
    """One Lambertian per texture (material i reads texture i).  `fillers`: six small spheres far outside every probe's
    view, so that the RT_HIT_BVH route walks a tree with inner nodes; no camera ray reaches them, the frame is the same."""
    textures = list(textures)
    prims = list(prims)
    if fillers:
        textures.append(abi.solid((0.5, 0.5, 0.5)))
        for i in range(6):
            prims.append(abi.sphere((1.0e4 + 40.0 * i, 1.0e4, 1.0e4 + 25.0 * i), 1.0, len(textures) - 1))
    materials = [abi.material(L, i) for i in range(len(textures))]
    for i, p in enumerate(prims):
        p.obj_id = i + 1
    return abi.SceneBundle(prims, materials, textures, abi.solid_background(BLACK), images=list(images), perlins=list(perlins))


# ---- image probes ------------------------------------------------------------------------------------------------------------

def _image_sphere(kind="plain"):
    def build(fillers=False, roll=0):
        img = big_image() if not roll else np.ascontiguousarray(np.roll(big_image(), roll, axis=1))
        if kind == "plain":
            prim = abi.sphere((0.0, 0.0, 0.0), 1.0, 0)
        elif kind == "shell":       # a negative radius: the outward normal points at the centre
            prim = abi.sphere((0.0, 0.0, 0.0), -1.0, 0)
        elif kind == "wrapped":     # RotateY then Translate: PRIMS_ANY with flags, the f64 (u, v) only
            prim = V.wrap(abi.sphere((0.0, 0.0, 0.0), 1.0, 0), 30.0, (0.5, 0.0, 0.0))
        else:                       # a MovingSphere: (u, v) of the POINT (moving_sphere.rs:76)
            prim = abi.moving_sphere((0.0, 0.0, 0.0), (0.0, 0.3, 0.0), 1.0, 0, 0, 0.0, 1.0)
        return _bundle([prim], [image_texture(0)], images=[img], fillers=fillers)
    return build


def _cam(look_from, look_at, vfov, scene_up=(0.0, 1.0, 0.0)):
    return dict(look_from=look_from, look_at=look_at, vfov=vfov, scene_up=scene_up)


IMAGE_SHAPE = (128, 128, 4)


def _images_two_sizes(fillers=False):
    """Three XY rects side by side with a 1x1, a 7x1 and a 5x3 image: three image records, three image textures, the
    5x3 one behind a Checkered whose other side is a solid colour.  (The rects stand at z = 0.1, not 0: sin(10 z) of a
    point on the plane z = 0 takes its sign from the point's last bits, which is checker_zero_plane's subject.)"""
    images = [small_image(1, 1, 5), small_image(7, 1, 6), small_image(5, 3, 7)]
    textures = [image_texture(0), image_texture(1), image_texture(2), abi.solid((0.2, 0.9, 0.4)), checker_texture(3, 2)]
    prims = [abi.rect(abi.RT_PRIM_XY_RECT, -3.0, -1.0, -1.0, 1.0, 0.1, 0),
             abi.rect(abi.RT_PRIM_XY_RECT, -1.0, 1.0, -1.0, 1.0, 0.1, 1),
             abi.rect(abi.RT_PRIM_XY_RECT, 1.0, 3.0, -1.0, 1.0, 0.1, 4)]
    return _bundle(prims, textures, images=images, fillers=fillers)


# ---- noise probes ------------------------------------------------------------------------------------------------------------
NOISE_DEPTHS = (0, 1, 8, 9, 10, 16, 24)
NOISE_CAM = _cam((0.0, 0.0, 8.0), (0.0, 0.0, 0.0), 28.0)    # the rect of half-size 2 fills the frame (8 tan 14 deg = 1.99)
ROOM_CAM = _cam((278.0, 278.0, -200.0), (278.0, 278.0, 0.0), 40.0)


def _noise_rect(depth, scale=4.0, room=False):
    def build(fillers=False, depth=depth):
        if room:     # the Cornell room's back wall: half-size 278 around (278, 278, 555)
            prim = abi.rect(abi.RT_PRIM_XY_RECT, 0.0, 556.0, 0.0, 556.0, 555.0, 0)
        else:
            prim = abi.rect(abi.RT_PRIM_XY_RECT, -2.0, 2.0, -2.0, 2.0, 0.0, 0)
        return _bundle([prim], [noise_texture(0, depth, scale)], perlins=[V.perlin(False, 7)], fillers=fillers)
    return build


def _noise_two_tables(shuffled):
    """Two rects, a Noise on table 0 and a Noise on table 1.  Both tables the identity: table 0's gradients are in LDS, and
    table 1 must not be served from them.  Table 1 shuffled: no gradients in LDS, both tables are read from global memory."""
    def build(fillers=False, table1=1):
        prims = [abi.rect(abi.RT_PRIM_XY_RECT, -2.0, 0.0, -2.0, 2.0, 0.0, 0),
                 abi.rect(abi.RT_PRIM_XY_RECT, 0.0, 2.0, -2.0, 2.0, 0.0, 1)]
        textures = [noise_texture(0, 7), noise_texture(table1, 7)]
        return _bundle(prims, textures, perlins=[V.perlin(False, 7), V.perlin(shuffled, 8)], fillers=fillers)
    return build


# ---- checker probes ----------------------------------------------------------------------------------------------------------

def _checker_room(sign):
    """Checkered(red, blue) on three mutually orthogonal room-sized rects at +-555: |10 x| up to 5 550.  sign = -1 is the
    room mirrored through the origin, plain rects at negative coordinates (a Translate wrapper would take the scene out of
    the rects-only kernels).  No rect lies in a coordinate plane (checker_zero_plane's subject)."""
    def build(fillers=False, swap=False):
        lo, hi = min(0.0, sign * 555.0), max(0.0, sign * 555.0)
        k = sign * 555.0
        prims = [abi.rect(abi.RT_PRIM_XY_RECT, lo, hi, lo, hi, k, 2),
                 abi.rect(abi.RT_PRIM_XZ_RECT, lo, hi, lo, hi, k, 2),
                 abi.rect(abi.RT_PRIM_YZ_RECT, lo, hi, lo, hi, k, 2)]
        red, blue = abi.solid((0.7, 0.2, 0.15)), abi.solid((0.15, 0.25, 0.7))
        textures = [red, blue, checker_texture(1, 0) if swap else checker_texture(0, 1)]
        return _bundle(prims, textures, fillers=fillers)
    return build


def _checker_zero_plane(fillers=False):
    """Checkered on an XZ rect at y = 0: sin(10 y) is sin(+-0) or the sine of a last-bit residue of o.y + t d.y.  A zero
    factor makes the product 0, which is not negative: the even side.  RT_ARITH_REFERENCE routes only: the fast flavour's
    last bits may differ from the reference's, and here the last bit decides the side."""
    textures = [abi.solid((0.7, 0.2, 0.15)), abi.solid((0.15, 0.25, 0.7)), checker_texture(0, 1)]
    return _bundle([abi.rect(abi.RT_PRIM_XZ_RECT, -40.0, 40.0, -40.0, 40.0, 0.0, 2)], textures, fillers=fillers)


def _mirror(cam):
    return dict(cam, look_from=tuple(-x for x in cam["look_from"]), look_at=tuple(-x for x in cam["look_at"]))


CHECKER_ROOM_CAM = _cam((100.0, 100.0, -600.0), (420.0, 420.0, 555.0), 50.0)

PROBES = {
    # cell boundaries inside the f32 error; both arms of the certification
    "image_equator": Probe("image", IMAGE_SHAPE, _cam((0.0, 0.0, 8.0), (0.0, 0.0, 0.0), 20.0), _image_sphere(), ALL_ROUTES),
    # atan2 at +-pi, u clamped at 0 and 1
    "image_seam": Probe("image", IMAGE_SHAPE, _cam((-8.0, 0.0, 0.0), (0.0, 0.0, 0.0), 20.0), _image_sphere(), ALL_ROUTES),
    # the 2^-10 switch to f64, v at 0 and 1
    "image_pole_up": Probe("image", IMAGE_SHAPE, _cam((0.0, 8.0, 0.0), (0.0, 0.0, 0.0), 3.0, (0.0, 0.0, 1.0)), _image_sphere(),
                           ALL_ROUTES),
    "image_pole_down": Probe("image", IMAGE_SHAPE, _cam((0.0, -8.0, 0.0), (0.0, 0.0, 0.0), 3.0, (0.0, 0.0, 1.0)), _image_sphere(),
                             ALL_ROUTES),
    # a camera inside a sphere of radius -1: front faces whose outward normal points at the centre ...
    "image_shell": Probe("image", IMAGE_SHAPE, _cam((0.0, 0.0, 0.5), (0.3, 0.2, -1.0), 50.0), _image_sphere("shell"), ALL_ROUTES),
    # ... and inside a sphere of radius 1: back faces, the flipped normal that the exact-uv lambda has to un-flip
    "image_inside": Probe("image", IMAGE_SHAPE, _cam((0.0, 0.0, 0.5), (0.3, 0.2, -1.0), 50.0), _image_sphere(), ALL_ROUTES),
    # the f64-only arms
    "image_wrapped": Probe("image", IMAGE_SHAPE, _cam((0.5, 0.0, 8.0), (0.5, 0.0, 0.0), 20.0), _image_sphere("wrapped"), ALL_ROUTES),
    "image_moving": Probe("image", IMAGE_SHAPE, _cam((0.0, 0.15, 8.0), (0.0, 0.15, 0.0), 24.0), _image_sphere("moving"), ALL_ROUTES),
    # per-texture image record copy, N x 1, 1 x 1
    "images_two_sizes": Probe("image", (96, 48, 2), _cam((0.0, 0.0, 8.0), (0.0, 0.0, 0.0), 20.0), _images_two_sizes, ALL_ROUTES),
    # the pi == 0 choice of the cooperative turbulence
    "noise_two_tables": Probe("noise", (64, 64, 2), NOISE_CAM, _noise_two_tables(False), ALL_ROUTES),
    "noise_two_tables_shuffled": Probe("noise", (64, 64, 2), NOISE_CAM, _noise_two_tables(True), ALL_ROUTES),
    # lattice indices past 2^31 after doubling: saturation of the conversion and the wrap of index + 1
    "noise_room": Probe("noise", (64, 64, 2), ROOM_CAM, _noise_rect(24, room=True), ALL_ROUTES),
    # scale 1500 x z 555: sin_lean's three-term reduction at k ~ 5e5 (inside its documented range of ~1e6)
    "noise_big_argument": Probe("noise", (64, 64, 2), ROOM_CAM, _noise_rect(7, scale=1500.0, room=True), ALL_ROUTES),
    # more than eight lanes of one wave want a Noise lookup: a second round of request slots
    "noise_wave": Probe("noise", (16, 16, 2), NOISE_CAM, _noise_rect(7), ALL_ROUTES),
    # reduction and floor parity at |10 x| ~ 5 500, both signs
    "checker_room": Probe("checker", (64, 64, 2), CHECKER_ROOM_CAM, _checker_room(1.0), ALL_ROUTES),
    "checker_room_negative": Probe("checker", (64, 64, 2), _mirror(CHECKER_ROOM_CAM), _checker_room(-1.0), ALL_ROUTES),
    # sin(+-0): product not negative -> even side
    "checker_zero_plane": Probe("checker", (64, 64, 2), _cam((0.3, 1.0, 4.0), (0.0, 0.0, 0.0), 40.0), _checker_zero_plane, EXACT_ROUTES),
}
# the pass loop of the cooperative turbulence (eight octaves per pass), including no octave at all
for _d in NOISE_DEPTHS:
    PROBES["noise_depth[%d]" % _d] = Probe("noise", (64, 64, 2), NOISE_CAM, _noise_rect(_d), ALL_ROUTES)
del _d

CASES = [(name, route) for name, probe in PROBES.items() for route in probe.routes]


# ---- rendering a probe with the oracle ---------------------------------------------------------------------------------------

def camera(orc, probe, shape=None):
    w, h, _ = shape or probe.shape
    c = probe.cam
    return orc.camera(c["look_from"], c["look_at"], c["vfov"], 0.0, 10.0, w, h, scene_up=c["scene_up"])


def params(probe, shape=None):
    w, h, spp = shape or probe.shape
    return abi.render_params(w, h, spp, max_depth=1)


def guide_shape(probe):
    """The frame of the guides route.  Its rays go through the pixel centres, without a draw.  With the probes' square,
    even frames and a camera on a coordinate axis, whole lines of pixel centres hit a sphere where (u W, v H) sits EXACTLY
    on a cell boundary: the centre row and column lie in the coordinate planes (u = 1/4, 3/4, v = 1/2, and the seam, where
    atan2(-+0, x < 0) = -+pi), and seen from a pole the diagonals have |x| = |z| (u = 1/8, 3/8, ... = cell 256, 768, ...).
    There the texel is chosen by the sign of a zero, which the fast arithmetic (the only flavour the guides are compiled
    in) does not promise to share with the reference: measured, 5 to 12 of the 16 384 guide pixels of a pole probe took the
    neighbouring texel, all of them on these lines.  The image probes therefore render their guides 1 pixel narrower and 3
    lower: both sizes odd (no centre in a coordinate plane) and unequal (the pixels are no longer square, by 1e-4, so no
    centre lies on a diagonal); every other edge of the probe is still on screen.  test_texture_probes_cpu.py holds the
    guide lookups of every image probe to at least 1e-9 of a cell away from any boundary."""
    w, h, _ = probe.shape
    return (w - 1, h - 3, 1) if probe.kind == "image" else (w, h, 1)


def oracle_frame(orc, probe, bundle):
    """-> (frame, segments) of the oracle (its linear scan where a primitive is wrapped, as everywhere in the suite)."""
    return orc.render(bundle.desc, camera(orc, probe), params(probe), use_bvh=V.oracle_use_bvh(bundle))


# ---- per-sample helpers ------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xffffffff)
RT_RNG_PIXEL, RT_RNG_CAMERA, RT_RNG_SAMPLE_PIXEL, PHILOX_ROUNDS = 0, 1, 0xFFFFFFFF, 7    # include/rt_rng.h


def philox_doubles(seed, pixel, sample, segment, purpose, block=0):
    """(d0, d1) of include/rt_rng.h's draw for arrays of pixels and samples: Philox4x32-7 over
    ctr = {pixel, sample, segment << 8 | purpose, block}, key = {seed lo, seed hi}; u53(hi, lo) = ((hi << 32 | lo) >> 11) 2^-53."""
    pixel, sample = np.broadcast_arrays(np.asarray(pixel, dtype=np.uint64), np.asarray(sample, dtype=np.uint64))
    c = [pixel & _M32, sample & _M32, np.full(pixel.shape, (segment << 8) | purpose, dtype=np.uint64),
         np.full(pixel.shape, block, dtype=np.uint64)]
    k0, k1 = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    for _ in range(PHILOX_ROUNDS):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    u53 = lambda hi, lo: (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return u53(c[0], c[1]), u53(c[2], c[3])


HIT_DTYPE = np.dtype([("point", "f8", 3), ("normal", "f8", 3), ("t", "f8"), ("u", "f8"), ("v", "f8"), ("front_face", "i4"),
                      ("material", "i4"), ("obj_id", "i4"), ("_pad", "i4")])

FirstHits = namedtuple("FirstHits", "px py sample origin dirs time hit rec")


def primary_rays(cam, prm):
    """Every (pixel, sample) of a pinhole camera, row-major then by sample -> (px, py, sample, dirs [N, 3], time [N]).
    oracle/trace.c:717-732: u = (px + ju(pixel)) / (W - 1), shared by a pixel's samples; v = (py + jv(pixel, sample)) / (H - 1);
    d = ulc + u horizontal - v vertical - origin, in that order (the lens offset of a pinhole is zero);
    time = time_a + (time_b - time_a) d1 of the same block."""
    assert cam.lens_radius == 0.0
    w, h, spp, seed = prm.width, prm.height, prm.samples, int(prm.seed)
    pixel = np.repeat(np.arange(w * h, dtype=np.int64), spp)
    sample = np.tile(np.arange(spp, dtype=np.int64), w * h)
    px, py = pixel % w, pixel // w
    ju, _ = philox_doubles(seed, pixel, RT_RNG_SAMPLE_PIXEL, 0, RT_RNG_PIXEL)
    jv, d1 = philox_doubles(seed, pixel, sample, 0, RT_RNG_CAMERA)
    u = (px.astype(np.float64) + ju) / float(w - 1)
    v = (py.astype(np.float64) + jv) / float(h - 1)
    ulc, hor, ver, org = (np.array(x[:]) for x in (cam.upper_left_corner, cam.horizontal, cam.vertical, cam.origin))
    dirs = ((ulc[None, :] + hor[None, :] * u[:, None]) - ver[None, :] * v[:, None]) - org[None, :]
    time = cam.time_a + (cam.time_b - cam.time_a) * d1
    return px, py, sample, np.ascontiguousarray(dirs), time


def _hits(orc, bundle, cam, px, py, sample, dirs, time):
    lib = orc.lib()
    n = len(px)
    dirs = np.ascontiguousarray(dirs)
    scene = lib.orc_scene_build(C.byref(bundle.desc), V.oracle_use_bvh(bundle), 1)
    recs = (orc.OrcHit * n)()
    dirs_c = (abi.D3 * n).from_buffer(dirs)
    origin = orc.d3(cam.origin)
    hit = np.zeros(n, dtype=bool)
    inf = math.inf
    hit_time = lib.orc_scene_hit_time
    try:
        for i in range(n):
            hit[i] = hit_time(scene, origin, dirs_c[i], time[i], 0.001, inf, C.byref(recs[i]))
    finally:
        lib.orc_scene_free(scene)
    assert C.sizeof(orc.OrcHit) == HIT_DTYPE.itemsize
    rec = np.frombuffer(recs, dtype=HIT_DTYPE).copy()
    return FirstHits(px, py, sample, np.array(cam.origin[:]), dirs, time, hit, rec)


def first_hits(orc, bundle, cam, prm):
    """For every (pixel, sample) of a pinhole camera: the oracle's primary ray and its OrcHit over [0.001, inf).
    -> FirstHits(px, py, sample, origin [3], dirs [N, 3], time [N], hit [N] bool, rec [N] of HIT_DTYPE).
    The hit is orc_scene_hit's at the ray's own time (orc_scene_hit is orc_scene_hit_time at time 0: the same for every
    scene without a MovingSphere)."""
    return _hits(orc, bundle, cam, *primary_rays(cam, prm))


def guide_hits(orc, bundle, cam, width, height):
    """The same for the rays of the guide planes (include/rt_abi.h, tests/denoise_model.py: oracle_guides): one per pixel
    through its centre, at the middle of the shutter interval."""
    pixel = np.arange(width * height, dtype=np.int64)
    px, py = pixel % width, pixel // width
    u, v = (px + 0.5) / (width - 1), (py + 0.5) / (height - 1)
    ulc, hor, ver, org = (np.array(x[:]) for x in (cam.upper_left_corner, cam.horizontal, cam.vertical, cam.origin))
    dirs = ((ulc[None, :] + u[:, None] * hor[None, :]) - v[:, None] * ver[None, :]) - org[None, :]
    time = np.full(len(px), (cam.time_a + cam.time_b) * 0.5)
    return _hits(orc, bundle, cam, px, py, np.zeros_like(px), dirs, time)


def texture_values(orc, bundle, hits):
    """orc_texture_value of every first hit's material [N, 3] (zeros where the ray missed: the black background)."""
    lib = orc.lib()
    out = np.zeros((len(hits.hit), 3))
    tex = (C.c_double * 3)()
    desc = bundle.desc
    for i in np.flatnonzero(hits.hit):
        r = hits.rec[i]
        lib.orc_texture_value(C.byref(desc), desc.materials[int(r["material"])].texture, float(r["u"]), float(r["v"]),
                              orc.d3(r["point"]), tex)
        out[i] = tex[:]
    return out


def frame_from_samples(values, prm):
    """sqrt(sum over a pixel's samples x (1 / samples)), summed in sample order like the oracle's loop (cpu.rs:39-52)."""
    v = values.reshape(prm.height, prm.width, prm.samples, 3)
    acc = np.zeros((prm.height, prm.width, 3))
    for s in range(prm.samples):
        acc = acc + v[:, :, s, :]
    return np.sqrt((1.0 / float(prm.samples)) * acc)
