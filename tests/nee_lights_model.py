"""A restatement of the extended light list (rt_scene_set_lights) for the tests, on tests/nee_model.py's
tracing helpers and therefore on the oracle's pieces: its own list, pick weights, light sample and pdf.

  list     a DiffuseLight Sphere (r > 0) or rect (area != 0), wrapped ones with RT_LIGHTS_WRAPPED; a Box of positive surface
           area with RT_LIGHTS_BOXES (a wrapped one needs WRAPPED too); a MovingSphere (r > 0) with RT_LIGHTS_MOVING; table
           order, at most 64.
  pick     uniform: k = min(floor(e0 n), n - 1), p = 1 / n.  By power: w = A L, p_k = w_k / sum, cdf the running sum over
           the total with cdf[n - 1] = 1, k the first index with e0 < cdf[k]; uniform when the sum is not positive and finite.
  frame    x_o = rot_fwd(x - tr), directions take the rotation only; sample and pdf from (x_o, w_o) alone.

With the default params (nothing extended listed, uniform pick) the model IS nee_model.Model: the same functions run, so
the frames are equal bit for bit.  As the library does, a list that holds an extended light or a pick by power evaluates
EVERY light, plain ones too, by the object-frame formulas.
"""
import ctypes as C
import math

import numpy as np

import nee_model as NM

PLAIN, WRAPPED, BOXES, MOVING, ALL = 0, 1, 2, 4, 7
UNIFORM, POWER_PICK = 0, 1
BOX, MOVING_SPHERE = 4, 5
ROTATE_Y, TRANSLATE = 1, 2
SOLID_COLOR = 0
RT_RNG_LIGHT = 8


def box_area(p):
    a, b, c = abs(p[3] - p[0]), abs(p[4] - p[1]), abs(p[5] - p[2])
    return 2.0 * (a * b + b * c + c * a)


def eligible(desc, i, kinds):
    p = desc.primitives[i]
    if desc.materials[p.material].kind != NM.LIGHT:
        return False
    if p.flags != 0 and not kinds & WRAPPED:
        return False
    if p.kind == NM.SPHERE:
        return p.p[3] > 0.0
    if p.kind in (NM.XY, NM.XZ, NM.YZ):
        return (p.p[1] - p.p[0]) * (p.p[3] - p.p[2]) != 0.0
    if p.kind == BOX:
        return bool(kinds & BOXES) and box_area(p.p) > 0.0
    if p.kind == MOVING_SPHERE:
        return bool(kinds & MOVING) and p.p[3] > 0.0
    return False


def light_list(desc, kinds=PLAIN, max_lights=NM.MAX_LIGHTS):
    return [i for i in range(desc.n_primitives) if eligible(desc, i, kinds)][:min(max_lights, NM.MAX_LIGHTS)]


def is_plain(desc, i):
    p = desc.primitives[i]
    return p.flags == 0 and p.kind in (NM.SPHERE, NM.XY, NM.XZ, NM.YZ)


def weight(desc, i):
    """w = A L: the object-frame area times the largest colour component of a SolidColor emitter (negative or not finite:
    0), else 1."""
    p = desc.primitives[i]
    if p.kind in (NM.SPHERE, MOVING_SPHERE):
        area = 4.0 * math.pi * (p.p[3] * p.p[3])
    elif p.kind == BOX:
        area = box_area(p.p)
    else:
        area = abs((p.p[1] - p.p[0]) * (p.p[3] - p.p[2]))
    t = desc.textures[desc.materials[p.material].texture]
    L = 1.0
    if t.kind == SOLID_COLOR:
        c = list(t.color[:])
        L = math.nan if any(math.isnan(v) for v in c) else max(c)
        if not math.isfinite(L) or L < 0.0:
            L = 0.0
    return area * L


def pick_table(desc, lights, n, pick):
    """-> (p, cdf, uniform) of the first n listed lights."""
    n = min(n, len(lights))
    if n <= 0:
        return [], [], True
    w = [weight(desc, i) for i in lights[:n]]
    total = 0.0
    for v in w:   # (in table order, one f64 addition each: not Python's compensated sum)
        total = total + v
    uniform = pick != POWER_PICK or not total > 0.0 or not math.isfinite(total)
    if uniform:
        return [1.0 / n] * n, [(k + 1) / n for k in range(n - 1)] + [1.0], True
    p, cdf, run = [], [], 0.0
    for v in w:
        run = run + v
        p.append(v / total)
        cdf.append(run / total)
    cdf[-1] = 1.0
    return p, cdf, False


def pick_light(e0, n, cdf, uniform):
    if uniform:
        return min(int(math.floor(e0 * n)), n - 1)
    for k in range(n):
        if e0 < cdf[k]:
            return k
    return n - 1


# ------------------------------------------------------------------------------------------------------ the object frame
def _flags(prim):
    return 0 if prim.kind == MOVING_SPHERE else prim.flags


def rot_fwd(a, s, c):
    return np.array([c * a[0] - s * a[2], a[1], s * a[0] + c * a[2]])


def rot_back(a, s, c):
    return np.array([c * a[0] + s * a[2], a[1], -s * a[0] + c * a[2]])


def point_to_object(prim, x):
    f = _flags(prim)
    x = np.array(x, dtype=np.float64)
    if f & TRANSLATE:
        x = x - np.array(prim.translate[:])
    if f & ROTATE_Y:
        x = rot_fwd(x, prim.rot_sin, prim.rot_cos)
    return x


def dir_to_object(prim, w):
    return rot_fwd(w, prim.rot_sin, prim.rot_cos) if _flags(prim) & ROTATE_Y else np.array(w, dtype=np.float64)


def dir_to_world(prim, w):
    return rot_back(w, prim.rot_sin, prim.rot_cos) if _flags(prim) & ROTATE_Y else w


def _center(prim, time):
    c = np.array(prim.p[:3])
    if prim.kind == MOVING_SPHERE:
        c = c + (np.array(prim.center_b[:]) - c) * ((time - prim.time_a) * (1.0 / (prim.time_b - prim.time_a)))
    return c


def box_side(p, s):
    """box.rs:22-71 -> (axis, a0, a1, b0, b1, k) of side s."""
    axis = 2 - (s >> 1)
    if axis == 2:
        return axis, p[0], p[3], p[1], p[4], (p[2] if s & 1 else p[5])
    if axis == 1:
        return axis, p[0], p[3], p[2], p[5], (p[1] if s & 1 else p[4])
    return axis, p[1], p[4], p[2], p[5], (p[0] if s & 1 else p[3])


def _in_plane(axis):
    return (1 if axis == 0 else 0), (1 if axis == 2 else 2)


def box_pdf(p, xo, wo, p_k):
    """Every side the half-line xo + t wo, t > 0, crosses: p_k / A_tot * sum t^2 / |w_axis|."""
    total = 0.0
    for s in range(6):
        axis, a0, a1, b0, b1, k = box_side(p, s)
        wa = wo[axis]
        if wa == 0.0:
            continue
        t = (k - xo[axis]) / wa
        ia, ib = _in_plane(axis)
        a, b = xo[ia] + t * wo[ia], xo[ib] + t * wo[ib]
        if t > 0.0 and a0 <= a <= a1 and b0 <= b <= b1:
            total += t * t / abs(wa)
    return p_k / box_area(p) * total


def light_pdf(prim, x, w, p_k, time=0.0):
    """Solid-angle density the light sampler has for the unit world direction w from x (which found the light)."""
    xo, wo = point_to_object(prim, x), dir_to_object(prim, w)
    if prim.kind in (NM.SPHERE, MOVING_SPHERE):
        c = _center(prim, time)
        r2 = prim.p[3] * prim.p[3]
        dc2 = float((c - xo) @ (c - xo))
        if dc2 <= r2:
            return 0.0
        return p_k / (2.0 * math.pi * (1.0 - math.sqrt(max(0.0, 1.0 - r2 / dc2))))
    if prim.kind == BOX:
        return box_pdf(prim.p, xo, wo, p_k)
    axis = NM._axis(prim.kind)
    wa = wo[axis]
    if wa == 0.0:
        return math.inf
    t = (prim.p[4] - xo[axis]) / wa
    return p_k * (t * t) / (abs(wa) * abs((prim.p[1] - prim.p[0]) * (prim.p[3] - prim.p[2])))


class _Geo:
    """What nee_model.sample_light reads of a primitive, for a sphere around another centre or a box side as a rect."""

    def __init__(self, kind, p):
        self.kind, self.p = kind, p


def sample_light(prim, x, e1, e2, face, p_k, time=0.0):
    """-> (unit world direction, solid-angle pdf); pdf 0: no sample.  `face`: the box's face draw."""
    xo = point_to_object(prim, x)
    if prim.kind in (NM.SPHERE, MOVING_SPHERE):
        c = _center(prim, time)
        wo, p = NM.sample_light(_Geo(NM.SPHERE, [c[0], c[1], c[2], prim.p[3]]), xo, e1, e2, p_k)
    elif prim.kind == BOX:
        areas = []
        for s in range(6):
            _, a0, a1, b0, b1, _ = box_side(prim.p, s)
            areas.append(abs(a1 - a0) * abs(b1 - b0))
        target, run, side = face * box_area(prim.p), 0.0, 5
        for s in range(5):
            run += areas[s]
            if target < run:
                side = s
                break
        axis, a0, a1, b0, b1, k = box_side(prim.p, side)
        ca, cb = a0 + (a1 - a0) * e1, b0 + (b1 - b0) * e2
        y = [np.array([k, ca, cb]), np.array([ca, k, cb]), np.array([ca, cb, k])][axis]
        v = y - xo
        dist2 = float(v @ v)
        if not dist2 > 0.0:
            return None, 0.0
        wo = v / math.sqrt(dist2)
        p = box_pdf(prim.p, xo, wo, p_k)
    else:
        wo, p = NM.sample_light(_Geo(prim.kind, list(prim.p[:])), xo, e1, e2, p_k)
    if not p > 0.0:
        return None, 0.0
    return dir_to_world(prim, wo), p


class Model(NM.Model):
    """rt_render_frame_nee's frame after rt_scene_set_lights(kinds, pick)."""

    def __init__(self, orc, desc, kinds=PLAIN, pick=UNIFORM):
        super().__init__(orc, desc)
        self.kinds, self.pick = kinds, pick
        listed = light_list(desc, kinds)
        self.extended = pick == POWER_PICK or any(not is_plain(desc, i) for i in listed)
        self._pick_of = (None, None, None)
        self.log = None

    def lights(self, max_lights=NM.MAX_LIGHTS):
        return light_list(self.desc, self.kinds, max_lights)

    def weights(self, max_lights=NM.MAX_LIGHTS):
        lights = self.lights()
        return pick_table(self.desc, lights, min(max_lights, len(lights)), self.pick)[0]

    def sample(self, cam, params, lights, heuristic, px, py, s, u):
        if not self.extended:   # nothing of the extension is in play: nee_model's own sample, bit for bit
            return super().sample(cam, params, lights, heuristic, px, py, s, u)
        seed, W, H = params.seed, params.width, params.height
        pixel = py * W + px
        draw = self.lib.orc_rng_double
        v = (py + draw(seed, pixel, s, 0, NM.RT_RNG_CAMERA, 0, 0)) / (H - 1)
        i = 0
        while True:  # util.rs:25-39
            rx = -1.0 + 2.0 * draw(seed, pixel, s, 0, NM.RT_RNG_LENS, i, 0)
            ry = -1.0 + 2.0 * draw(seed, pixel, s, 0, NM.RT_RNG_LENS, i, 1)
            if rx * rx + ry * ry < 1.0:
                break
            i += 1
        offset = np.array(cam.right[:]) * (rx * cam.lens_radius) + np.array(cam.up[:]) * (ry * cam.lens_radius)
        origin = np.array(cam.origin[:])
        o = origin + offset
        d = np.array(cam.upper_left_corner[:]) + np.array(cam.horizontal[:]) * u - np.array(cam.vertical[:]) * v - origin - offset
        time = cam.time_a + (cam.time_b - cam.time_a) * draw(seed, pixel, s, 0, NM.RT_RNG_CAMERA, 0, 1)

        n_lights = len(lights)
        key = tuple(lights)
        if self._pick_of[0] != key:   # one table per render, not per sample
            self._pick_of = (key, pick_table(self.desc, lights, n_lights, self.pick), {prim: k for k, prim in enumerate(lights)})
        (p_pick, cdf, uniform), slot = self._pick_of[1], self._pick_of[2]
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
            if M.kind == NM.LIGHT:
                w = 1.0
                if eligible_prev and prim in slot:  # a listed light found by the bounce of an NEE vertex
                    p_l = light_pdf(P, x_prev, NM._unit(d), p_pick[slot[prim]], time)
                    w = NM.mis(cos_b / math.pi, p_l, heuristic)
                    if self.log is not None:
                        self.log.append(dict(seg=seg, bounce_found=prim, kind=P.kind, p_l=p_l, cos_b=cos_b, w=w))
                return acc + T * self._tex(P.material, hu, hv, point) * w, segments
            if M.kind == NM.LAMBERTIAN:
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
                    k = pick_light(e0, n_lights, cdf, uniform)
                    L = lights[k]
                    LP = self.desc.primitives[L]
                    face = draw(seed, pixel, s, seg, RT_RNG_LIGHT, 1, 0) if LP.kind == BOX else 0.0
                    w, p_l = sample_light(LP, point, e1, e2, face, p_pick[k], time)
                    cos_x = float(normal @ w) if p_l > 0.0 else 0.0
                    if cos_x > 0.0:
                        shadow = self._trace(point, 2.0 * cos_x * w, time)
                        if shadow is not None and shadow[0] == L:
                            p_b = cos_x / math.pi
                            Le = self._tex(LP.material, shadow[3], shadow[4], shadow[1])
                            acc = acc + T * Le * (p_b / p_l * NM.mis(p_l, p_b, heuristic))
                    if self.log is not None:   # (a test's or a probe's look at one sample)
                        self.log.append(dict(seg=seg, vertex=prim, light=L, kind=LP.kind, p_l=p_l, cos_x=cos_x, acc=acc.copy()))
                o, d = point, dr
            elif M.kind == NM.METAL:
                eligible_prev = False
                ud = NM._unit(d)
                dr = ud - normal * (2.0 * float(ud @ normal)) + self._in_unit_sphere(seed, pixel, s, seg) * M.fuzz
                if float(dr @ normal) < 0.0:
                    return acc, segments
                T = T * self._tex(P.material, hu, hv, point)
                o, d = point, dr
            else:  # Dielectric
                eligible_prev = False
                ratio = 1.0 / M.refraction_index if front else M.refraction_index
                ud = NM._unit(d)
                cos_t = min(float(-ud @ normal), 1.0)
                sin_t = math.sqrt(1.0 - cos_t * cos_t)
                reflect = ratio * sin_t > 1.0
                if not reflect:
                    r0 = ((1.0 - ratio) / (1.0 + ratio)) ** 2
                    reflect = r0 + (1.0 - r0) * math.pow(1.0 - cos_t, 5.0) > draw(seed, pixel, s, seg, NM.RT_RNG_DIELECTRIC, 0, 0)
                if reflect:
                    dr = ud - normal * (2.0 * float(ud @ normal))
                else:
                    perp = (ud + normal * cos_t) * ratio
                    dr = perp + normal * (-math.sqrt(abs(1.0 - float(perp @ perp))))
                o, d = point, dr
            seg += 1
            if seg >= params.max_depth:
                return acc + T, segments

    def render(self, cam, params, max_lights=NM.MAX_LIGHTS, heuristic=NM.POWER):
        """-> (float64 [H, W, 3] gamma-encoded frame, path segments)."""
        lights = self.lights(max_lights)
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
