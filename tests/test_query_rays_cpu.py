"""The ray families of tests/query_ray_sets.py on the CPU, with the oracle alone: the conditions the comparisons of
tests/test_gpu_query_rays.py rest on, at that test's own n.

  S  both models commute with a power-of-two scale of the direction, bit for bit, on every scene and at every scale;
  Z  every axis direction and sign pair occurs, the rays aimed at a surface hit, next to no ray is tied;
  O  PULL_BACK holds the smallest power of 4 that leaves the box, the windows before and behind the box and the rays
     beside it are misses, the pulled-back ray sees what the base ray saw.

And the kernels' prologue (racer-tracer_amd/csrc/rt_query_ray.h) through tests/query_ray_driver.cpp, built with the host
compiler: plainly, and with -fsanitize=address,undefined as the stand-alone program it is (nothing preloaded)."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kernel_asm
import multihit_model as M
import query_ray_sets as R
import ray_query_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "racer-tracer_amd", "csrc")
K = 8


def bits(a):
    return np.ascontiguousarray(a).view(np.int64) if a.dtype.kind == "f" else a


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def test_the_scene_list_and_the_scales_are_the_ones_meant():
    assert len(R.SCENES) == 16 + 3 + 3 and len(set(R.SCENES)) == len(R.SCENES)
    assert R.SCALES == (-300, -130, -80, -65, -63, -24, -1, 0, 1, 24, 63, 65, 80, 130, 300)
    assert all(R.scales_for(name) == R.SCALES for name in R.SCENES)      # no scale dropped anywhere
    assert sorted(R.PULL_BACK) == sorted(R.SCENES)


# ---- S ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.SCENES)
def test_both_models_commute_with_a_power_of_two_scale(orc, name):
    """expected() and multihit_model at k = 8: at every e the planes of e = 0, t 2^e bit-equal, everything else bit-equal.
    Bits, not a tolerance."""
    bundle = R.scene(name)[0]
    rays = R.s_base(name)
    want = R.closest_model(orc, bundle, rays)
    want_multi = M.expected(R.hit_lists(orc, bundle, rays), K)
    hit = want["prim"] >= 0
    assert 0.2 <= hit.mean() <= 0.98 and (want_multi["count"] > 1).any()
    capped = np.isfinite(rays["t_max"])
    assert capped.mean() == 0.25 and (want["prim"][capped] >= 0).any() and (want["prim"][capped] < 0).any()
    for e in R.scales_for(name):
        s = R.scaled(rays, e)
        assert same_bits(s["direction"] * math.ldexp(1.0, -e), rays["direction"])      # the scaling itself lost nothing
        got = R.closest_model(orc, bundle, s)
        got_multi = M.expected(R.hit_lists(orc, bundle, s), K)
        for model, ref in ((got, want), (got_multi, want_multi)):
            for plane in ref:
                a = model[plane] * math.ldexp(1.0, e) if plane == "t" else model[plane]
                assert same_bits(a, ref[plane]), (name, e, plane)


# ---- Z ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.SCENES)
def test_zero_component_rays_meet_their_conditions(orc, name):
    bundle = R.scene(name)[0]
    z = R.z_family(orc, name)
    d, kind = z["direction"], z["kind"]
    along = z["axis_dir"] >= 0
    # what the rays are: exactly two zero components on a ray along an axis, exactly one on a plane ray
    assert ((d[along] == 0.0).sum(axis=1) == 2).all()
    assert ((d[kind == 1] == 0.0).sum(axis=1) == 1).all()
    assert ((d[kind == 2] == 0.0).sum(axis=1) >= 1).all()
    # all six axis directions and all four sign pairs occur (a ray along its target's flat surface is still one of them)
    assert sorted(set(z["axis_dir"][along])) == list(range(6))
    seen = set()
    for dv, a in zip(d[along], z["axis_dir"][along]):
        others = [x for x in range(3) if x != a // 2]
        seen.add(tuple(bool(np.signbit(dv[x])) for x in others))
        assert (dv[a // 2] > 0) == (a % 2 == 0)
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    assert sorted(set(z["pair"][along])) == [0, 1, 2, 3]
    has_rects = bool(R.plain_rects(bundle))
    assert (kind == 2).sum() >= (R.N_IN_PLANE if has_rects else 0)
    want = R.closest_model(orc, bundle, z)
    aimed = kind < 2
    share = (want["prim"][aimed] >= 0).mean()
    tied = R.tied_closest(orc, bundle, z, want)
    print("%s: %d rays (%d axis, %d plane, %d in-plane); hit share of the aimed ones %.3f, of the in-plane ones %.3f; tied %.4f"
          % (name, len(kind), (kind == 0).sum(), (kind == 1).sum(), (kind == 2).sum(), share,
             (want["prim"][kind == 2] >= 0).mean() if (kind == 2).any() else math.nan, tied.mean()))
    assert aimed.sum() >= 100 and share >= 0.9
    assert tied.mean() <= R.TIE_CAP.get(name, 0.01)
    # the reference's own answer: NaN only on in-plane rays, and steady under a re-parametrisation on EVERY ray that is
    # compared — by less than an eighth of the device tests' bound, so that the bound is a fair one
    lists = R.hit_lists(orc, bundle, z)
    degenerate = R.degenerate(lists, bundle, z)
    steady = R.z_conditioning(orc, name, z, want, lists)
    print("%s: %d degenerate rays; the reference moves by %s on the others" % (name, degenerate.sum(), {p: "%.2g" % v for p, v in steady.items()}))
    assert not degenerate[aimed].any()
    split = R.models_disagree(want, lists) & ~degenerate
    print("%s: the reference's scan and its per-primitive tests disagree on rays %s" % (name, np.nonzero(split)[0].tolist()))
    assert split.sum() <= 2 and not split[aimed].any()
    assert all(np.isfinite(h[0]) for i in np.nonzero(~degenerate)[0] for h in lists[i])
    assert max(steady.values()) <= 1e-9 / 8
    # no ray left that is tangent to a curved target
    normal_at = np.abs((z["direction"] * want["normal"]).sum(axis=1)) / np.linalg.norm(z["direction"], axis=1)
    curved = (want["prim"] >= 0) & ~degenerate & (normal_at > 0.0)
    print("%s: smallest |d . n| / |d| on a hit %.3g" % (name, normal_at[curved].min()))


# ---- O ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.SCENES)
def test_outside_rays_meet_their_conditions(orc, name):
    bundle = R.scene(name)[0]
    o = R.o_family(orc, name)
    mn, mx = o["box"]
    base = R.base(name)
    n = len(base["origin"])
    # f is the smallest power of 4 that puts 0.9 of the origins outside
    f = R.PULL_BACK[name]
    assert f == R.pull_back_factor(mn, mx, base), (name, R.pull_back_factor(mn, mx, base))
    assert math.log(f, 4) == round(math.log(f, 4))
    out = R.outside(mn, mx, o["pulled"]["origin"])
    assert out.mean() >= 0.9 and (f == 1 or R.outside(mn, mx, base["origin"] - (f // 4) * base["direction"]).mean() < 0.9)
    assert o["crossing"].mean() >= 0.75 and len(o["before"]["origin"]) == o["crossing"].sum() == len(o["behind"]["origin"])
    # the windows before and behind the box, and the lines beside it: misses on every ray
    t_enter, t_exit = R.slab_interval(mn, mx, o["beside"]["origin"], o["beside"]["direction"])
    assert len(t_enter) == R.N_BESIDE and (t_enter > t_exit).all() and R.outside(mn, mx, o["beside"]["origin"]).all()
    for which in ("before", "behind", "beside"):
        rays = o[which]
        assert (rays["t_max"] >= rays["t_min"]).all() and (rays["t_min"] >= Q.T_MIN).all()
        want = R.closest_model(orc, bundle, rays)
        assert (want["prim"] == Q.MISS).all(), (name, which)
        assert all(found == [] for found in R.hit_lists(orc, bundle, rays)), (name, which)
    # the pulled-back ray with its window moved by f names the primitive the base ray named
    want = R.closest_model(orc, bundle, base)
    pulled = R.closest_model(orc, bundle, o["pulled"])
    between = R.closest_model(orc, bundle, o["between"])
    agree = pulled["prim"] == want["prim"]
    hit = agree & (want["prim"] >= 0)
    shift = np.abs(pulled["t"][hit] - f - want["t"][hit])
    print("%s: f = %d, %.3f of the origins outside, %.3f crossing; pulled agrees on %d of %d, max |t(o - f d) - f - t(o)| %.3g"
          " (relative to t + f %.3g); %d hit in the default window, %d of them in front of the base origin"
          % (name, f, out.mean(), o["crossing"].mean(), agree.sum(), n, shift.max(), (shift / (want["t"][hit] + f)).max(),
             (between["prim"] >= 0).sum(), ((between["prim"] >= 0) & (between["t"] < f)).sum()))
    assert agree.mean() >= 0.98
    moved = R.far_origin_movement(orc, name, o)
    print("%s: the reference's t moves by %.2g between the base ray and the pulled-back one" % (name, moved))
    assert moved <= (1e-9 / 8 if f == 1 else 2.5e-10)      # (f = 256: 2.1e-10)
    # neither S nor O holds a ray without an expected answer
    for rays in (R.s_base(name), o["pulled"], o["between"]):
        lists = R.hit_lists(orc, bundle, rays)
        assert not R.degenerate(lists, bundle, rays).any() and not R.models_disagree(R.closest_model(orc, bundle, rays), lists).any()
    assert ((between["prim"] >= 0) >= (pulled["prim"] >= 0)).all()      # the default window holds the moved one


# ---- the prologue's header ---------------------------------------------------------------------------------------------------------

def build_driver(exe, extra=()):
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "query_ray_driver.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


def run_driver(exe, seed, env=None):
    run = subprocess.run([exe, str(seed)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    words = run.stdout.split()
    assert words[0] == "ok", run.stdout
    tally = {k: int(v) for k, v in zip(words[1::2], words[2::2])}
    assert tally["cases"] > 100000
    # the defects are still in the walk, the cure in the prologue: e = -70, -80, -130 lost to the clamp, -300 to the f32 window
    assert tally["clamped_before"] == 3 and tally["window_before"] == 1
    return tally


def test_prologue_rules_on_the_host(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "query_ray_driver")
    build = build_driver(exe)
    assert build.returncode == 0, build.stderr[-3000:]
    for seed in (1, 2026):
        print(run_driver(exe, seed))


def test_query_ray_driver_is_clean_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "query_ray_driver_san")
    build = build_driver(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("sanitizer runtimes not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run_driver(exe, 1, env=env)


def test_the_k8_tree_kernel_keeps_four_waves_per_simd():
    """rt_query_ray.h reads the caller's direction AGAIN behind the walk (caller_direction, a volatile load) so that it is not
    held in registers beside the walked one: held, k_trace_rays_multi_f64<true, 8> took 132 VGPRs in the fast flavour, past
    the 128 that four waves per SIMD allow, and 15 % longer.  A compiler that undoes this shows here (124 today)."""
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    text = kernel_asm.asm_text("multihit", "fast")
    m = re.search(r"\.amdhsa_kernel _ZN\d+rtdev_fast\d+k_trace_rays_multi_f64ILb1ELi8EEE\w*\n(.*?)\.end_amdhsa_kernel", text, re.S)
    assert m, "k_trace_rays_multi_f64<true, 8> is not in the compiled unit"
    vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(1)).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(1)).group(1))
    print("k_trace_rays_multi_f64<true, 8>, fast: %d VGPRs, %d B of scratch" % (vgprs, scratch))
    assert vgprs <= 128 and scratch == 0
