"""A restatement of rt_render_frame_nee's estimator for the tests, on the oracle's own pieces.

The plain estimator's steps are the oracle's (oracle/trace.c: ray_color, scatter, get_ray), taken one segment at a time
with the oracle's closest hit, texture lookups and addressed draws (orc_scene_hit_time, orc_texture_value,
orc_rng_double, orc_rng_triple): with no light listed the model IS the plain estimator, and tests/test_nee_cpu.py holds it
to orc.render.  On top of that it takes the light sample of the contract at every eligible Lambertian vertex and
weights both terms by multiple importance sampling.

Scope: whatever the oracle's linear closest hit takes (rects, spheres, moving spheres, boxes, Translate and RotateY
wrappers, the lens, any texture it evaluates, on a light too), Lambertian, Metal, Dielectric and DiffuseLight; listed
lights are plain spheres and rects of any axis.  tests/test_nee_cpu.py verifies it on cornell_box, three_balls,
mixed_scene and the scene of every kernel form (tests/variant_scenes.py), with and without `light2`: lights off it is
orc.render to 1e-12 with the same segments, and with several lights of every kind its mean is the plain mean.  The hit
primitive is found by its obj_id, so a scene given to the model has unique obj_ids.  Scalar Python over (pixel, sample):
meant for frames of a few thousand samples.
"""
import ctypes as C
import math

import numpy as np

RT_RNG_CAMERA, RT_RNG_LENS, RT_RNG_SCATTER, RT_RNG_DIELECTRIC, RT_RNG_LIGHT = 1, 2, 3, 4, 8
SPHERE, XY, XZ, YZ = 0, 1, 2, 3
LAMBERTIAN, METAL, DIELECTRIC, LIGHT = 0, 1, 2, 3
POWER, BALANCE = 0, 1
MAX_LIGHTS = 64


def eligible(desc, i):
    """Is primitive i listed (before the cap)?  A plain sphere of positive radius or a rect of non-zero area, no
    wrapper, DiffuseLight."""
    p = desc.primitives[i]
    if p.flags != 0 or desc.materials[p.material].kind != LIGHT:
        return False
    if p.kind == SPHERE:
        return p.p[3] > 0.0
    if p.kind in (XY, XZ, YZ):
        return (p.p[1] - p.p[0]) * (p.p[3] - p.p[2]) != 0.0
    return False


def light_list(desc, max_lights=MAX_LIGHTS):
    """The listed primitives in table order, capped at min(max_lights, 64)."""
    return [i for i in range(desc.n_primitives) if eligible(desc, i)][:min(max_lights, MAX_LIGHTS)]


def _axis(kind):
    return {XY: 2, XZ: 1, YZ: 0}[kind]


def _unit(v):
    return v / math.sqrt(float(v @ v))


def mis(p, q, heuristic):
    if heuristic == POWER:
        p, q = p * p, q * q
    return p / (p + q) if p > 0.0 else 0.0


def light_pdf(prim, x, y, w, p_pick):
    """Solid-angle pdf of a listed light from x toward its point y along the unit direction w."""
    if prim.kind == SPHERE:
        c = np.array(prim.p[:3])
        r2 = prim.p[3] * prim.p[3]
        dc2 = float((c - x) @ (c - x))
        if dc2 <= r2:
            return 0.0
        return p_pick / (2.0 * math.pi * (1.0 - math.sqrt(max(0.0, 1.0 - r2 / dc2))))
    g = abs(w[_axis(prim.kind)]) * abs((prim.p[1] - prim.p[0]) * (prim.p[3] - prim.p[2]))
    return p_pick * float((y - x) @ (y - x)) / g if g > 0.0 else math.inf


def sample_light(prim, x, e1, e2, p_pick):
    """-> (unit direction, solid-angle pdf); pdf 0: no sample."""
    if prim.kind == SPHERE:  # uniform in the cone the sphere subtends
        c = np.array(prim.p[:3])
        r2 = prim.p[3] * prim.p[3]
        cx = c - x
        dc2 = float(cx @ cx)
        if dc2 <= r2:
            return None, 0.0
        one_m = 1.0 - math.sqrt(max(0.0, 1.0 - r2 / dc2))
        if not one_m > 0.0:
            return None, 0.0
        cos_t = 1.0 - e1 * one_m
        sin_t = math.sqrt(max(0.0, 1.0 - cos_t * cos_t))
        phi = 2.0 * math.pi * e2
        z = cx / math.sqrt(dc2)
        sign = math.copysign(1.0, z[2])  # Duff et al. 2017
        a = -1.0 / (sign + z[2])
        b = z[0] * z[1] * a
        b1 = np.array([1.0 + sign * z[0] * z[0] * a, sign * b, -sign * z[0]])
        b2 = np.array([b, sign + z[1] * z[1] * a, -z[1]])
        return sin_t * math.cos(phi) * b1 + sin_t * math.sin(phi) * b2 + cos_t * z, p_pick / (2.0 * math.pi * one_m)
    axis = _axis(prim.kind)
    ca, cb = prim.p[0] + (prim.p[1] - prim.p[0]) * e1, prim.p[2] + (prim.p[3] - prim.p[2]) * e2
    y = [np.array([prim.p[4], ca, cb]), np.array([ca, prim.p[4], cb]), np.array([ca, cb, prim.p[4]])][axis]
    v = y - x
    dist2 = float(v @ v)
    w = v / math.sqrt(dist2)
    g = abs(w[axis]) * abs((prim.p[1] - prim.p[0]) * (prim.p[3] - prim.p[2]))
    if not (g > 0.0 and dist2 > 0.0):
        return None, 0.0
    return w, p_pick * dist2 / g


class Model:
    """rt_render_frame_nee's frame for one scene description (a SceneBundle's .desc)."""

    def __init__(self, orc, desc):
        self.orc, self.lib, self.desc = orc, orc.lib(), desc
        ids = [desc.primitives[i].obj_id for i in range(desc.n_primitives)]
        assert len(set(ids)) == len(ids), "the model finds the hit primitive by its obj_id: give every primitive its own"
        self.by_id = {oid: i for i, oid in enumerate(ids)}
        self.scene = self.lib.orc_scene_build(C.byref(desc), 0, 0)  # linear closest hit
        self.hit = orc.OrcHit()

    def close(self):
        if self.scene:
            self.lib.orc_scene_free(self.scene)
            self.scene = None

    def __del__(self):
        self.close()

    # ------------------------------------------------------------------ pieces of the oracle
    def _trace(self, o, d, time):
        h = self.hit
        if not self.lib.orc_scene_hit_time(self.scene, self.orc.d3(o), self.orc.d3(d), time, 0.001, math.inf, C.byref(h)):
            return None
        return self.by_id[h.obj_id], np.array(h.point[:]), np.array(h.normal[:]), h.u, h.v, h.front_face

    def _tex(self, mat, u, v, point):
        out = (C.c_double * 3)()
        self.lib.orc_texture_value(C.byref(self.desc), self.desc.materials[mat].texture, u, v, self.orc.d3(point), out)
        return np.array(out[:])

    def _triple(self, seed, pixel, sample, seg, purpose, block):
        e = (C.c_double * 3)()
        self.lib.orc_rng_triple(seed, pixel, sample, seg, purpose, block, e)
        return e[0], e[1], e[2]

    def _in_unit_sphere(self, seed, pixel, sample, seg):
        i = 0
        while True:
            e = self._triple(seed, pixel, sample, seg, RT_RNG_SCATTER, i)
            p = np.array([-1.0 + 2.0 * e[0], -1.0 + 2.0 * e[1], -1.0 + 2.0 * e[2]])
            if float(p @ p) < 1.0:
                return p
            i += 1

    # ------------------------------------------------------------------ one sample
    def sample(self, cam, params, lights, heuristic, px, py, s, u):
        """-> (radiance [3], path segments) of sample s of pixel (px, py)."""
        seed, W, H = params.seed, params.width, params.height
        pixel = py * W + px
        draw = self.lib.orc_rng_double
        v = (py + draw(seed, pixel, s, 0, RT_RNG_CAMERA, 0, 0)) / (H - 1)
        i = 0
        while True:  # util.rs:25-39
            rx = -1.0 + 2.0 * draw(seed, pixel, s, 0, RT_RNG_LENS, i, 0)
            ry = -1.0 + 2.0 * draw(seed, pixel, s, 0, RT_RNG_LENS, i, 1)
            if rx * rx + ry * ry < 1.0:
                break
            i += 1
        offset = np.array(cam.right[:]) * (rx * cam.lens_radius) + np.array(cam.up[:]) * (ry * cam.lens_radius)
        origin = np.array(cam.origin[:])
        o = origin + offset
        d = np.array(cam.upper_left_corner[:]) + np.array(cam.horizontal[:]) * u - np.array(cam.vertical[:]) * v - origin - offset
        time = cam.time_a + (cam.time_b - cam.time_a) * draw(seed, pixel, s, 0, RT_RNG_CAMERA, 0, 1)

        n_lights = len(lights)
        p_pick = 1.0 / n_lights if n_lights else 0.0
        T, acc = np.ones(3), np.zeros(3)
        seg, segments = 0, 0
        eligible_prev, x_prev, cos_b = False, None, 0.0
        if params.max_depth <= 0:
            return T, 0
        while True:
            segments += 1
            hit = self._trace(o, d, time)
            if hit is None:
                bg = (C.c_double * 3)()
                self.lib.orc_background_color(C.byref(self.desc.background), self.orc.d3(d), bg)
                return acc + T * np.array(bg[:]), segments
            prim, point, normal, hu, hv, front = hit
            P = self.desc.primitives[prim]
            M = self.desc.materials[P.material]
            if M.kind == LIGHT:
                w = 1.0
                if eligible_prev and prim in lights:  # a listed light found by the bounce of an NEE vertex
                    w = mis(cos_b / math.pi, light_pdf(P, x_prev, point, _unit(d), p_pick), heuristic)
                return acc + T * self._tex(P.material, hu, hv, point) * w, segments
            if M.kind == LAMBERTIAN:
                r = self._in_unit_sphere(seed, pixel, s, seg)
                dr = normal + r / math.sqrt(float(r @ r))
                if np.all(np.abs(dr) < 1e-8):
                    dr = normal
                T = T * self._tex(P.material, hu, hv, point)
                eligible_prev = n_lights > 0 and seg + 1 < params.max_depth
                if eligible_prev:
                    x_prev = point
                    cos_b = float(normal @ dr) / math.sqrt(float(dr @ dr))
                    e0, e1, e2 = self._triple(seed, pixel, s, seg, RT_RNG_LIGHT, 0)
                    L = lights[min(int(math.floor(e0 * n_lights)), n_lights - 1)]
                    w, p_l = sample_light(self.desc.primitives[L], point, e1, e2, p_pick)
                    cos_x = float(normal @ w) if p_l > 0.0 else 0.0
                    if cos_x > 0.0:
                        shadow = self._trace(point, 2.0 * cos_x * w, time)
                        if shadow is not None and shadow[0] == L:
                            p_b = cos_x / math.pi
                            Le = self._tex(self.desc.primitives[L].material, shadow[3], shadow[4], shadow[1])
                            acc = acc + T * Le * (p_b / p_l * mis(p_l, p_b, heuristic))
                o, d = point, dr
            elif M.kind == METAL:
                eligible_prev = False
                ud = _unit(d)
                dr = ud - normal * (2.0 * float(ud @ normal)) + self._in_unit_sphere(seed, pixel, s, seg) * M.fuzz
                if float(dr @ normal) < 0.0:
                    return acc, segments
                T = T * self._tex(P.material, hu, hv, point)
                o, d = point, dr
            else:  # Dielectric
                eligible_prev = False
                ratio = 1.0 / M.refraction_index if front else M.refraction_index
                ud = _unit(d)
                cos_t = min(float(-ud @ normal), 1.0)
                sin_t = math.sqrt(1.0 - cos_t * cos_t)
                reflect = ratio * sin_t > 1.0
                if not reflect:
                    r0 = ((1.0 - ratio) / (1.0 + ratio)) ** 2
                    reflect = r0 + (1.0 - r0) * math.pow(1.0 - cos_t, 5.0) > draw(seed, pixel, s, seg, RT_RNG_DIELECTRIC, 0, 0)
                if reflect:
                    dr = ud - normal * (2.0 * float(ud @ normal))
                else:
                    perp = (ud + normal * cos_t) * ratio
                    dr = perp + normal * (-math.sqrt(abs(1.0 - float(perp @ perp))))
                o, d = point, dr
            seg += 1
            if seg >= params.max_depth:
                return acc + T, segments

    def render(self, cam, params, max_lights=MAX_LIGHTS, heuristic=POWER):
        """-> (float64 [H, W, 3] gamma-encoded frame, path segments)."""
        lights = light_list(self.desc, max_lights)
        out = np.zeros((params.height, params.width, 3))
        segments = 0
        for py in range(params.height):
            for px in range(params.width):
                u = self.lib.orc_pixel_u(C.byref(params), px, py)
                total = np.zeros(3)
                for s in range(params.samples):
                    c, n = self.sample(cam, params, lights, heuristic, px, py, s, u)
                    total = total + c
                    segments += n
                out[py, px] = np.sqrt(total * (1.0 / params.samples))
        return out, segments


def mixed_scene(abi):
    """A rect light, a sphere light, an unlisted moving-sphere emitter, Lambertian, Metal and Dielectric spheres, and a
    Lambertian sphere inside a large light sphere; unique obj_ids.  -> (SceneBundle, camera dict)."""
    textures = [abi.solid((0.6, 0.6, 0.6)), abi.solid((0.7, 0.2, 0.2)), abi.solid((0.8, 0.8, 0.9)), abi.solid((4.0, 4.0, 4.0)),
                abi.solid((6.0, 3.0, 1.0)), abi.solid((1.0, 4.0, 1.0)), abi.solid((0.5, 0.5, 2.0))]
    materials = [abi.material(LAMBERTIAN, 0), abi.material(LAMBERTIAN, 1), abi.material(METAL, 2, fuzz=0.3),
                 abi.material(DIELECTRIC, -1, ior=1.5), abi.material(LIGHT, 3), abi.material(LIGHT, 4),
                 abi.material(LIGHT, 5), abi.material(LIGHT, 6)]
    prims = [abi.rect(abi.RT_PRIM_XZ_RECT, -6, 6, -6, 6, 0.0, 0, 1),        # floor
             abi.rect(abi.RT_PRIM_XY_RECT, -6, 6, 0, 6, -5.0, 0, 2),        # back wall
             abi.rect(abi.RT_PRIM_XZ_RECT, -1, 1, -1, 1, 4.0, 4, 3),        # rect light
             abi.sphere((2.2, 1.5, 0.0), 0.4, 5, 4),                        # sphere light
             abi.moving_sphere((-2.2, 1.0, -1.0), (-2.2, 1.4, -1.0), 0.3, 6, 5),  # moving emitter: never listed
             abi.sphere((0.0, 0.7, 0.0), 0.7, 1, 6),                        # Lambertian
             abi.sphere((-1.5, 0.5, 1.2), 0.5, 2, 7),                       # Metal
             abi.sphere((1.2, 0.5, 1.4), 0.5, 3, 8),                        # Dielectric
             abi.sphere((3.5, 1.2, -3.0), 1.0, 7, 9),                       # large light sphere ...
             abi.sphere((3.5, 1.2, -3.0), 0.3, 0, 10)]                      # ... with a Lambertian sphere inside
    cam = dict(look_from=(0.0, 2.5, 9.0), look_at=(0.0, 1.0, 0.0), vfov=45.0, aperture=0.0, focus_distance=10.0)
    return abi.SceneBundle(prims, materials, textures, abi.solid_background((0.05, 0.05, 0.08))), cam


def block_z(nee_frames, plain_frames, block=4):
    """z-scores of the block means of linear radiance (rgb^2) of two estimators, each given as frames at independent
    seeds: (mean_a - mean_b) / sqrt(se_a^2 + se_b^2) per block and channel, the standard errors from the seeds' spread.
    Blocks where both spreads are 0 must agree exactly (z = 0 there, inf otherwise)."""
    def stats(frames):
        lin = np.stack([f * f for f in frames])  # [seeds, H, W, 3]
        s, h, w, _ = lin.shape
        b = lin[:, :h // block * block, :w // block * block].reshape(s, h // block, block, w // block, block, 3).mean(axis=(2, 4))
        return b.mean(axis=0), b.var(axis=0, ddof=1) / s
    ma, va = stats(nee_frames)
    mb, vb = stats(plain_frames)
    se = np.sqrt(va + vb)
    diff = ma - mb
    z = np.where(se > 0, diff / np.where(se > 0, se, 1.0), np.where(diff == 0, 0.0, np.inf))
    return z
