"""The hit and scatter code against the oracle, ray by ray, at its edges: every probe of tests/ray_probes.py through every
route that has hit or scatter code of its own.

  pool-fast      k_trace_pool_f64, RT_ARITH_FAST, the linear loop in the form the probe's scene selects: rects-only
                 (rect_closest_update's v_cmpx tests, the camera-batch primary trace), spheres-only (sphere_t with the per-ray
                 reciprocal), any-primitive (the rect, sphere and BOX groups, box_slab_t, prim_t<PRIMS_ANY> for the wrapped)
  pool-fast-bvh  the same over the tree: the f32 culling boxes, the compact leaf records, prim_t<PRIMS_ANY> for the others
  pool-exact     RT_ARITH_REFERENCE: IEEE divisions, no contraction, the six rect tests of a box
  v1-fast/exact  k_trace_f64
  guides         render_guides' obj_id, normal and position of one ray per pixel: the most direct per-ray readout there is

A probe's camera makes every sample the same ray (or a fan with one direction component exactly zero), so NO pixel is excused:
tests/test_ray_probes_cpu.py proves on the CPU that the reference alone decides each ray, and not by a rounding.  The bounds
are the project's own: TIGHT where the pixel sums are f64; for the fixed-point sums of the pooled any-primitive and tree
forms the pair of test_gpu_overlap.py / test_gpu_parity_proofs.py, 1e-11 in radiance and 5e-8 in the frame.  On the routes
whose code comments declare a tie open (box_slab_t's side, the tree's visiting order) a tie probe, rendered at max_depth 1,
must show the colour of one of the tied candidates and nothing else."""
import numpy as np
import pytest

import ray_probes as P

pytestmark = pytest.mark.gpu
abi = P.abi
TIGHT = 1e-9                          # f64 against f64 with the same draws (tests/test_gpu_texture_edges.py)
FIXED_RADIANCE, FIXED_FRAME = 1e-11, 5e-8      # fixed-point pixel sums (tests/test_gpu_parity_proofs.py)
GUIDE = 1e-9                          # tests/test_gpu_denoise.py: the guides' planes against the oracle's

CASES = [(name, route) for name, probe in P.PROBES.items() for route in probe.routes]


@pytest.fixture(scope="module")
def reference(orc):
    """Oracle frames and guide planes, one per (probe, with fillers): computed once, never written to."""
    frames, guides = {}, {}

    def frame(name, fillers):
        if (name, fillers) not in frames:
            ref, segments = P.oracle_frame(orc, P.PROBES[name], fillers=fillers)
            ref.setflags(write=False)
            frames[name, fillers] = (ref, segments)
        return frames[name, fillers]

    def guide(name):
        if name not in guides:
            guides[name] = P.oracle_guides(orc, P.PROBES[name])
        return guides[name]
    return frame, guide


def _assert_within(name, route, got, ref, fixed_point):
    d = float(np.abs(got - ref).max())
    d2 = float(np.abs(got ** 2 - ref ** 2).max())
    print("%s %s: max |delta| %.3g (radiance %.3g)" % (name, route, d, d2))
    if fixed_point:
        assert d2 < FIXED_RADIANCE and d < FIXED_FRAME, "max |delta| = %g, in radiance %g" % (d, d2)
    else:
        assert d < TIGHT, "max |delta| = %g" % d        # every pixel: the cap on left-out pixels is zero


def _tied_colours(probe, bundle):
    """The depth-1 pixel of each tied candidate: sqrt(mean of spp equal albedos) (renderer.rs:48-55)."""
    out = []
    for obj_id in probe.tie[1]:
        m = bundle.materials[bundle.primitives[obj_id - 1].material]
        out.append(np.sqrt(np.array(bundle.textures[m.texture].color[:])))
    return out


@pytest.mark.parametrize("name,route", CASES, ids=lambda x: str(x))
def test_probe_matches_oracle(rt, orc, gpu, reference, name, route):
    probe = P.PROBES[name]
    w, h, spp = probe.shape
    frame_ref, guide_ref = reference
    cam = probe.camera()
    open_tie = probe.tie is not None and route in probe.tie[0]
    if route == "guides":
        scene = rt.Scene(probe.bundle())
        try:
            got = scene.render_guides(cam, probe.params(probe.guide_shape()))
        finally:
            scene.close()
        ref = guide_ref(name)
        hit = ref["obj_id"] >= 0
        print("%s guides: %d of %d rays hit, max |delta position| %.3g" %
              (name, hit.sum(), hit.size, np.abs(got["position"] - ref["position"]).max()))
        assert np.array_equal(got["obj_id"], ref["obj_id"])
        assert np.abs(got["position"] - ref["position"]).max() < GUIDE
        if open_tie and probe.tie[2]:     # the side of a box on its edge: the normal of one of the tied sides, against the ray
            tied = [np.array(n) for n in probe.tie[2]]
            for n in got["normal"][hit]:
                assert any(np.array_equal(n, t) for t in tied), n
            return
        assert np.abs(got["normal"] - ref["normal"]).max() < GUIDE
        nz = ref["normal"] != 0.0         # the sign of every non-zero component (a rect's comes from dir[axis]'s sign bit)
        assert np.array_equal(np.signbit(got["normal"][nz]), np.signbit(ref["normal"][nz]))
        return
    r = P.ROUTES[route]
    bvh = r.closest_hit == abi.RT_HIT_BVH
    bundle = probe.bundle(fillers=bvh)
    scene = rt.Scene(bundle, closest_hit=r.closest_hit, kernel=r.kernel, arithmetic=r.arithmetic)
    try:
        variant = scene.variant()
        got = scene.render_frame(cam, probe.params())
        stats = scene.last_stats()
    finally:
        scene.close()
    # the route is the one meant
    want = dict(kernel=int(r.kernel == abi.RT_KERNEL_V1), textured=0, use_bvh=int(bvh), exact=r.exact,
                has_moving=int(probe.cls == "moving_sphere"))
    assert {k: variant[k] for k in want} == want
    if bvh:
        assert variant["bvh_nodes_in_lds"] == int(probe.cls != "bvh_global")
    else:
        assert variant["prims_class"] == probe.form
    ref, ref_segments = frame_ref(name, bvh)
    assert np.isfinite(got).all()
    assert stats.samples == w * h * spp
    assert int(stats.segments) == ref_segments        # exactly: one fixed ray has no silhouette
    fixed_point = r.kernel == abi.RT_KERNEL_POOL and not r.exact and (bvh or probe.form == P.ANY)      # rt_api.hip: sum_scale
    if open_tie and len(probe.tie[1]) > 1:
        assert probe.depth == 1
        colours = _tied_colours(probe, bundle)
        d = np.min([np.abs(got - c).max(axis=-1) for c in colours], axis=0)
        print("%s %s: max |delta| to the nearest tied colour %.3g" % (name, route, d.max()))
        assert d.max() < (FIXED_FRAME if fixed_point else TIGHT)
        return
    _assert_within(name, route, got, ref, fixed_point)
