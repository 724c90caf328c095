"""Scenes for the extended light list (rt_scene_set_lights): one with a light of every extended kind, the Cornell box with
its light inside a Translate (the "wrapper twin"), and the variant scenes of tests/variant_scenes.py with extended lights
appended.  Every primitive has its own obj_id (tests/nee_model.py finds the hit primitive by it)."""
import nee_model as NM
import scenes_py as S
import variant_scenes as V

abi = S.abi
L, M, D, E = abi.RT_MAT_LAMBERTIAN, abi.RT_MAT_METAL, abi.RT_MAT_DIELECTRIC, abi.RT_MAT_DIFFUSE_LIGHT


def all_kinds_scene():
    """A box light, a RotateY + Translate rect light, a translated sphere light and a moving sphere light, next to
    Lambertian, Metal and Dielectric spheres over a floor and in front of a wall.  Nothing in it is listed by
    rt_scene_create.  -> (SceneBundle, camera dict)."""
    textures = [abi.solid((0.6, 0.6, 0.6)), abi.solid((0.7, 0.2, 0.2)), abi.solid((0.8, 0.8, 0.9)), abi.solid((5.0, 4.0, 3.0)),
                abi.solid((2.0, 6.0, 2.0)), abi.solid((3.0, 3.0, 9.0)), abi.solid((8.0, 2.0, 2.0))]
    materials = [abi.material(L, 0), abi.material(L, 1), abi.material(M, 2, fuzz=0.2), abi.material(D, -1, ior=1.5),
                 abi.material(E, 3), abi.material(E, 4), abi.material(E, 5), abi.material(E, 6)]
    translated = abi.sphere((0.0, 0.0, 0.0), 0.35, 6)
    translated.flags = abi.RT_PRIM_HAS_TRANSLATE
    translated.translate = abi.D3(2.3, 1.6, 0.2)
    prims = [abi.rect(abi.RT_PRIM_XZ_RECT, -6, 6, -6, 6, 0.0, 0),                                      # floor
             abi.rect(abi.RT_PRIM_XY_RECT, -6, 6, 0, 6, -4.0, 1),                                      # back wall
             V.wrap(abi.box((0.0, 0.0, 0.0), (0.9, 0.25, 0.7), 4), 25.0, (-0.4, 3.2, -0.6)),          # box lamp
             V.wrap(abi.rect(abi.RT_PRIM_XY_RECT, -0.5, 0.5, 0.0, 1.0, 0.0, 5), 35.0, (-2.6, 0.4, -1.0)),  # wrapped rect light
             translated,                                                                               # translated sphere light
             abi.moving_sphere((1.2, 2.4, -1.5), (1.2, 2.9, -1.5), 0.3, 7),                            # moving sphere light
             abi.sphere((0.0, 0.7, 0.0), 0.7, 1),                                                      # Lambertian
             abi.sphere((-1.5, 0.5, 1.2), 0.5, 2),                                                     # Metal
             abi.sphere((1.3, 0.5, 1.3), 0.5, 3)]                                                      # Dielectric
    for i, p in enumerate(prims):
        p.obj_id = i + 1
    cam = dict(look_from=(0.0, 2.2, 8.0), look_at=(0.0, 1.2, 0.0), vfov=45.0, aperture=0.0, focus_distance=10.0)
    return abi.SceneBundle(prims, materials, textures, abi.solid_background((0.03, 0.03, 0.05))), cam


TWIN_OFFSET = (100, -200, 50)   # integers: every coordinate of the twin's light stays exactly representable


def cornell_twin(offset=TWIN_OFFSET):
    """scenes_py.cornell_box with the ceiling light written as the same rect, moved by -offset, inside Translate(offset):
    the same surface, which rt_scene_create no longer lists.  -> (SceneBundle, camera dict)."""
    bundle, cam, _ = S.cornell_box()
    prims = list(bundle.primitives)[:6]
    lamp = prims[5]
    ox, oy, oz = offset
    a0, a1, b0, b1, k = lamp.p[0], lamp.p[1], lamp.p[2], lamp.p[3], lamp.p[4]
    for j, v in enumerate((a0 - ox, a1 - ox, b0 - oz, b1 - oz, k - oy)):
        lamp.p[j] = float(v)
    lamp.flags = abi.RT_PRIM_HAS_TRANSLATE
    lamp.translate = abi.D3(float(ox), float(oy), float(oz))
    return abi.SceneBundle(prims, list(bundle.materials)[:4], list(bundle.textures)[:4], bundle.desc.background), dict(cam)


def _light_material(bundle):
    for m in range(bundle.desc.n_materials):
        if bundle.materials[m].kind == E:
            return m
    raise AssertionError("the scene has no DiffuseLight material")


def extend(bundle, prims):
    """A new bundle: `bundle`'s tables with `prims` appended to its primitives, obj_ids continued."""
    d = bundle.desc
    old = list(bundle.primitives)[:d.n_primitives]
    for i, p in enumerate(prims):
        p.obj_id = len(old) + i + 1
    return abi.SceneBundle(old + list(prims), list(bundle.materials)[:d.n_materials], list(bundle.textures)[:d.n_textures],
                           d.background, images=list(bundle._image_arrays), perlins=list(bundle.perlins)[:d.n_perlins])


def variant_case(form):
    """The form's light2 scene (tests/variant_scenes.py; PRIMS_ANY forms) plus a box light, a wrapped rect light, a wrapped
    sphere light and, where the form has `moving`, a moving sphere light, all of the scene's own light material (a Noise
    light where the form has one).  -> (SceneBundle, camera dict)."""
    assert form[0] == V.ANY
    bundle, cam = V.build(form, light2=True)
    m = _light_material(bundle)
    more = [V.wrap(abi.box((0.0, 0.0, 0.0), (0.5, 0.2, 0.4), m), 20.0, (1.5, 2.2, -0.4)),
            V.wrap(abi.rect(abi.RT_PRIM_YZ_RECT, 0.0, 0.8, -0.4, 0.4, 0.0, m), -30.0, (-2.9, 0.6, 0.9)),
            V.wrap(abi.sphere((0.0, 0.0, 0.0), 0.25, m), 15.0, (2.6, 1.6, 0.8))]
    if V.SPECS[form].get("moving"):
        # (off every plane of the scene: a light centre in the plane of a rect it lights — z = -0.8 holds one — leaves the sign
        # of the cone basis' z.z to the last bit of the vertex, and the two arithmetic flavours then draw different directions)
        more.append(abi.moving_sphere((-1.4, 2.2, -0.65), (-1.4, 2.6, -0.65), 0.2, m, 0, 0.0, 1.0))
    return extend(bundle, more), cam


def n_extended(form):
    return 4 if V.SPECS[form].get("moving") else 3
