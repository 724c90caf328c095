"""Small synthetic scenes, one per trace-kernel form, for the variant matrix (tests/test_gpu_variants.py) and the oracle-only
checks that keep it honest (tests/test_variant_matrix.py).

A form is (prims_class, textured, specular, bvh): rt_scene_create_ex picks k_trace_pool_f64<PRIMS, TEXTURED, SPECULAR, BVH>
(and k_trace_f64<PRIMS, TEXTURED, SPECULAR> for RT_KERNEL_V1) from what the description holds.  Every scene here is
built from a feature spec; the features are spread over the forms so that each appears in every class whose kernel has
code for it (a pairwise design, not a full product):
  camera       pinhole / lens (the lens_lds branch and its grid)        every class
  moving       a MovingSphere                                           PRIMS_ANY, linear and BVH
  perlin       identity (gradients in LDS) / shuffled (global tables)   every textured class
  textures     image, a Checkered over an image or a Noise, solid, and a Noise on a DiffuseLight
  metal fuzz   0 / > 0, a Dielectric (on spheres with a negative-radius shell)
  wrappers     Translate and RotateY on a sphere and on a rect (the `flags` that send a rect to PRIMS_ANY)
  background   sky / solid
  light2       off in every spec; build(form, light2=True) adds plain YZ and XY rect lights and a second sphere light,
               for the next-event-estimation tests (a pick among several lights, every rect axis)
`probes` names the features a scene is there to exercise and the value that turns each off: the oracle must see the
difference (test_variant_matrix.py: sensitivity), so a GPU case would fail if the kernel's arm for it were wrong.
"""
import math

import numpy as np

import scenes_py as S

abi = S.abi
L, M, D, E = abi.RT_MAT_LAMBERTIAN, abi.RT_MAT_METAL, abi.RT_MAT_DIELECTRIC, abi.RT_MAT_DIFFUSE_LIGHT
RECTS, SPHERES, ANY = 0, 1, 2
W, H, SPP, DEPTH = 64, 36, 8, 20

# (prims_class, textured, specular, bvh) -> feature spec
SPECS = {
    (RECTS, 0, 0, 0): dict(lens=False, bg="solid", probes={"bg": "sky"}),
    (RECTS, 0, 1, 0): dict(lens=True, bg="sky", fuzz=0.0, probes={"metal": False, "lens": False}),
    (RECTS, 1, 0, 0): dict(lens=True, bg="solid", perlin="identity", image=True, noise_light=True,
                           probes={"image": False, "noise_light": False, "lens": False}),
    (RECTS, 1, 1, 0): dict(lens=False, bg="sky", perlin="shuffled", fuzz=0.3, image=True,
                           probes={"perlin": "identity", "metal": False, "fuzz": 0.0}),
    (SPHERES, 0, 0, 0): dict(lens=True, bg="sky", probes={"lens": False}),
    (SPHERES, 0, 1, 0): dict(lens=False, bg="solid", fuzz=0.3, shell=True,
                             probes={"fuzz": 0.0, "dielectric": False, "metal": False}),
    (SPHERES, 1, 0, 0): dict(lens=False, bg="sky", perlin="shuffled", probes={"perlin": "identity"}),
    (SPHERES, 1, 1, 0): dict(lens=True, bg="solid", perlin="identity", fuzz=0.0, image=True, noise_light=True,
                             probes={"lens": False, "metal": False, "image": False, "noise_light": False}),
    (ANY, 0, 0, 0): dict(lens=False, bg="sky", moving=True, wrap=True, probes={"moving": False, "wrap": False}),
    (ANY, 0, 1, 0): dict(lens=True, bg="solid", fuzz=0.3, shell=True, wrap=True,
                         probes={"lens": False, "metal": False, "wrap": False}),
    (ANY, 1, 0, 0): dict(lens=True, bg="sky", moving=True, perlin="identity", image=True, noise_light=True,
                         probes={"moving": False, "lens": False, "noise_light": False}),
    (ANY, 1, 1, 0): dict(lens=False, bg="solid", perlin="shuffled", fuzz=0.0, wrap=True, moving=True,
                         probes={"perlin": "identity", "metal": False, "moving": False}),
    (ANY, 0, 0, 1): dict(lens=False, bg="sky", moving=True, wrap=True, probes={"moving": False, "wrap": False}),
    (ANY, 0, 1, 1): dict(lens=True, bg="solid", fuzz=0.3, shell=True, probes={"lens": False, "metal": False, "fuzz": 0.0}),
    (ANY, 1, 0, 1): dict(lens=True, bg="sky", moving=True, perlin="identity", image=True,
                         probes={"lens": False, "image": False, "moving": False}),
    (ANY, 1, 1, 1): dict(lens=False, bg="solid", perlin="shuffled", fuzz=0.0, moving=True, noise_light=True,
                         probes={"perlin": "identity", "metal": False, "noise_light": False}),
}


def perlin(shuffled, seed=7):
    rng = np.random.default_rng(seed)
    pl = abi.RtPerlin()
    g = rng.uniform(-1.0, 1.0, size=(256, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    for i in range(256):
        for k in range(3):
            pl.ranvec[i][k] = float(g[i, k])
    perms = [rng.permutation(256) if shuffled else np.arange(256) for _ in range(3)]
    for i in range(256):
        pl.perm_x[i], pl.perm_y[i], pl.perm_z[i] = int(perms[0][i]), int(perms[1][i]), int(perms[2][i])
    return pl


def image(w=8, h=4):
    img = np.zeros((h, w, 4), dtype=np.uint8)
    img[..., 3] = 255
    for y in range(h):
        for x in range(w):
            img[y, x, :3] = (30 * x + 10, 255 - 60 * y, 40 + 25 * ((x + y) % 4))
    return img


def wrap(prim, deg, offset):
    """RotateY(deg) then Translate(offset) around a primitive (the Sandbox's order, scenes_py.cornell_box_boxes)."""
    rad = deg * math.pi / 180.0
    prim.flags = abi.RT_PRIM_HAS_ROTATE_Y | abi.RT_PRIM_HAS_TRANSLATE
    prim.rot_sin, prim.rot_cos = math.sin(rad), math.cos(rad)
    prim.translate = abi.D3(*offset)
    return prim


class _Tables:
    def __init__(self):
        self.textures, self.materials = [], []

    def tex(self, t):
        self.textures.append(t)
        return len(self.textures) - 1

    def mat(self, kind, texture=-1, fuzz=0.0, ior=0.0):
        self.materials.append(abi.material(kind, texture, fuzz, ior))
        return len(self.materials) - 1


def build(form, **override):
    """-> (SceneBundle, camera dict) of the form's spec, with `override` applied to the spec's features."""
    prims_class, textured, specular, bvh = form
    f = dict(lens=False, bg="sky", moving=False, perlin=None, image=False, noise_light=False,
             fuzz=None, shell=False, wrap=False, metal=True, dielectric=True, light2=False)
    f.update({k: v for k, v in SPECS[form].items() if k != "probes"})
    f.update(override)
    T = _Tables()
    perlins = [perlin(f["perlin"] == "shuffled")] if (textured and f["perlin"]) else []
    images = [image()] if (textured and f["image"]) else []
    grey = T.tex(abi.solid((0.55, 0.55, 0.5)))
    red = T.tex(abi.solid((0.7, 0.2, 0.15)))
    blue = T.tex(abi.solid((0.15, 0.25, 0.7)))
    mat_grey, mat_red, mat_blue = T.mat(L, grey), T.mat(L, red), T.mat(L, blue)
    mat_ground = mat_grey
    mat_feature = mat_blue       # what the textured arm shades: an image, or a Noise marble
    if textured:
        # a Checkered ground whose odd side is the Noise (or the image) and whose even side is a solid colour
        odd = None
        if perlins:
            odd = T.tex(abi.RtTexture(abi.RT_TEX_NOISE, -1, -1, -1, 0, 3, abi.D3(0.9, 0.8, 0.7), 4.0))
            mat_feature = T.mat(L, odd)
        if images:
            img_tex = T.tex(abi.RtTexture(abi.RT_TEX_IMAGE, -1, -1, 0, -1, 0, abi.D3(0, 0, 0), 0.0))
            mat_feature = T.mat(L, img_tex)
            odd = img_tex if odd is None else odd
        if odd is None:  # (a textured form always has a Perlin table or an image: SPECS)
            odd = red
        mat_ground = T.mat(L, T.tex(abi.RtTexture(abi.RT_TEX_CHECKERED, grey, odd, -1, -1, 0, abi.D3(0, 0, 0), 0.0)))
    if textured and f["noise_light"] and perlins:
        mat_light = T.mat(E, T.tex(abi.RtTexture(abi.RT_TEX_NOISE, -1, -1, -1, 0, 2, abi.D3(4.0, 3.5, 3.0), 6.0)))
    else:
        mat_light = T.mat(E, T.tex(abi.solid((4.0, 3.5, 3.0))))
    mat_metal = mat_red
    if specular and f["metal"]:
        mat_metal = T.mat(M, T.tex(abi.solid((0.85, 0.85, 0.8))), fuzz=f["fuzz"] or 0.0)
    mat_glass = mat_grey
    if specular and f["dielectric"]:
        mat_glass = T.mat(D, -1, ior=1.5)

    prims = []
    if prims_class == RECTS:
        # (the grounds stand at y = -0.05, not 0: at y = 0 the Checkered's sin(10 y) factor would take its sign from the
        # last bits of the hit point, and the fast arithmetic's last bits are allowed to differ from the reference's)
        prims += [abi.rect(abi.RT_PRIM_XZ_RECT, -5, 5, -5, 3, -0.05, mat_ground),        # ground
                  abi.rect(abi.RT_PRIM_XY_RECT, -3, 3, 0, 3, -2.0, mat_feature),         # back wall
                  abi.rect(abi.RT_PRIM_YZ_RECT, 0, 3, -2, 2, -2.6, mat_red),             # side wall
                  abi.rect(abi.RT_PRIM_XY_RECT, 0.2, 1.8, 0.1, 1.7, 0.3, mat_metal),     # mirror panel
                  abi.rect(abi.RT_PRIM_YZ_RECT, 0, 1.4, -1.2, 1.2, -0.9, mat_glass),     # glass pane
                  abi.rect(abi.RT_PRIM_XZ_RECT, -1.2, 1.2, -1.5, 0.5, 2.6, mat_light)]   # light
    else:
        if prims_class == SPHERES:
            prims.append(abi.sphere((0.0, -1000.0, 0.0), 1000.0, mat_ground))
        else:
            prims.append(abi.rect(abi.RT_PRIM_XZ_RECT, -6, 6, -6, 3, -0.05, mat_ground))
        prims += [abi.sphere((0.0, 0.7, -0.3), 0.7, mat_feature),
                  abi.sphere((-1.6, 0.6, 0.0), 0.6, mat_metal),
                  abi.sphere((1.6, 0.6, 0.0), 0.6, mat_glass)]
        if specular and f["dielectric"] and f["shell"]:
            prims.append(abi.sphere((1.6, 0.6, 0.0), -0.5, mat_glass))              # a hollow glass ball
        if prims_class == SPHERES:
            prims.append(abi.sphere((0.0, 3.2, -1.0), 0.6, mat_light))
        else:
            prims.append(abi.rect(abi.RT_PRIM_XZ_RECT, -1.2, 1.2, -1.5, 0.5, 2.8, mat_light))
            prims.append(abi.box((-0.6, 0.0, -2.2), (0.6, 1.8, -1.6), mat_red))           # a bare box
            if f["wrap"]:
                prims.append(wrap(abi.box((0.0, 0.0, 0.0), (0.8, 0.8, 0.8), mat_grey), 30.0, (2.4, 0.0, -1.2)))
                prims.append(wrap(abi.sphere((0.0, 0.0, 0.0), 0.35, mat_red), -20.0, (-0.7, 0.35, 1.0)))
                prims.append(wrap(abi.rect(abi.RT_PRIM_XY_RECT, -0.6, 0.6, 0.0, 1.2, 0.0, mat_blue), 40.0, (-2.6, 0.0, -0.8)))
            else:
                prims.append(abi.box((2.0, 0.0, -1.6), (2.8, 0.8, -0.8), mat_grey))
                prims.append(abi.sphere((-0.7, 0.35, 1.0), 0.35, mat_red))
                prims.append(abi.rect(abi.RT_PRIM_XY_RECT, -3.2, -2.0, 0.0, 1.2, -0.8, mat_blue))
            if f["moving"]:
                prims.append(abi.moving_sphere((0.8, 0.3, 1.2), (0.8, 0.9, 1.2), 0.3, mat_blue, 0, 0.0, 1.0))
            else:
                prims.append(abi.sphere((0.8, 0.6, 1.2), 0.3, mat_blue))
        if bvh:
            for i in range(12):  # a few more, so that the tree has some depth
                a = 2.0 * math.pi * i / 12
                prims.append(abi.sphere((3.2 * math.cos(a), 0.2, -1.0 + 2.2 * math.sin(a)), 0.2, (mat_red, mat_blue, mat_grey)[i % 3]))
    if f["light2"]:
        # more listed lights, plain and unwrapped so that the form stays its own: the YZ and XY arms of the rect
        # light's pdf and sample (the scenes' own rect light is XZ), and a pick among several (p_pick < 1)
        if prims_class == RECTS:
            prims += [abi.rect(abi.RT_PRIM_YZ_RECT, 0.4, 1.6, -0.6, 0.6, 2.4, mat_light),
                      abi.rect(abi.RT_PRIM_XY_RECT, -2.4, -1.4, 0.3, 1.3, -1.9, mat_light)]
        if prims_class == ANY:
            prims += [abi.rect(abi.RT_PRIM_YZ_RECT, 0.4, 1.6, -0.6, 0.6, 3.4, mat_light),
                      abi.rect(abi.RT_PRIM_XY_RECT, -2.4, -1.4, 0.3, 1.3, -2.4, mat_light)]
        if prims_class != RECTS:
            prims.append(abi.sphere((-2.4, 1.8, 0.6), 0.3, mat_light))
    for i, p in enumerate(prims):
        p.obj_id = i + 1
    bg = abi.sky() if f["bg"] == "sky" else abi.solid_background((0.35, 0.3, 0.4))
    bundle = abi.SceneBundle(prims, T.materials, T.textures, bg, images=images, perlins=perlins)
    cam = dict(look_from=(0.0, 1.6, 6.0), look_at=(0.0, 0.7, 0.0), vfov=42.0, aperture=0.35 if f["lens"] else 0.0,
               focus_distance=6.0)
    return bundle, cam


def oracle_use_bvh(bundle):
    """The oracle's BVH reproduces RotateY's mis-sized bounding box (tests/test_gpu_parity.py): wrapped primitives are
    compared with its linear scan."""
    return 0 if any(bundle.primitives[i].flags for i in range(bundle.desc.n_primitives)) else 1


def large_bvh_scene(n=3000):
    """Thousands of spheres, textured and specular: the BVH node array does not fit the 32 KiB of LDS it may take, so the
    walk reads the nodes from global memory (the direction-ordered copies)."""
    rng = np.random.default_rng(11)
    T = _Tables()
    pl = perlin(False)
    noise = T.tex(abi.RtTexture(abi.RT_TEX_NOISE, -1, -1, -1, 0, 3, abi.D3(0.9, 0.8, 0.7), 4.0))
    mats = [T.mat(L, T.tex(abi.solid((0.8, 0.3, 0.3)))), T.mat(L, noise), T.mat(M, T.tex(abi.solid((0.9, 0.9, 0.9))), fuzz=0.1),
            T.mat(D, -1, ior=1.5)]
    centers = rng.uniform(-30.0, 30.0, size=(n, 3))
    centers[:, 2] = rng.uniform(-70.0, -8.0, size=n)
    radii = rng.uniform(0.3, 0.9, size=n)
    prims = [abi.sphere(tuple(centers[i]), float(radii[i]), mats[i % 4], i + 1) for i in range(n)]
    bundle = abi.SceneBundle(prims, T.materials, T.textures, abi.sky(), perlins=[pl])
    cam = dict(look_from=(0.0, 0.0, 5.0), look_at=(0.0, 0.0, -40.0), vfov=50.0, aperture=0.0, focus_distance=10.0)
    return bundle, cam


def unbounded_scene():
    """A Lambertian colour above 1: the scene has no radiance bound, so the fixed-point sums of the two-item (OVERLAP)
    forms cannot hold it and rt_scene_create_ex sends it to the RT_ARITH_REFERENCE copy (rt_scene_create.hip)."""
    bundle, cam = build((ANY, 0, 1, 0))
    bundle.textures[0].color = abi.D3(1.3, 0.9, 0.9)
    return bundle, cam
