"""The ambient-occlusion query's model (tests/ambient_model.py) on the CPU, with the oracle alone: its directions are unit,
lie in the normal's hemisphere and follow the cosine law; the seeds of tests/test_gpu_ambient.py keep every candidate clear
of the acceptance edge, so that an acceptance cannot flip between the arithmetic flavours there; the model's verdicts on
scenes with a closed form; and the CLI's --ao values."""
import math
import os
import subprocess

import numpy as np
import pytest

import ambient_model as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IDENTITY, WALL = A.IDENTITY, A.WALL


@pytest.fixture(scope="module")
def wall_draws(orc):
    seed, base, n, samples = WALL
    return A.draws(orc, seed, base, n, samples)


def random_normals(n, seed=5):
    """Normals of any direction and of lengths between 1e-3 and 1e3."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    return v * (10.0 ** rng.uniform(-3, 3, n))[:, None]


def test_directions_are_unit_in_the_hemisphere_and_cosine_weighted(orc, wall_draws):
    """N = 4096 * 64 rays.  |dhat| = 1 to 4 ulp; dhat . nhat >= 0 (dir = nhat + a unit vector: the dot product is
    1 + cos >= 0 before the last normalisation, up to rounding); the mean of dhat . nhat is 2/3 for the cosine law (its
    variance 1/18; a uniform hemisphere would give 1/2) within five standard errors."""
    seed, base, n, samples = WALL
    u = wall_draws[0]
    normals = random_normals(n)
    r = A.rays(orc, np.zeros((n, 3)), normals, samples, seed=seed, index_base=base, u=u)
    d = r["direction"]
    N = n * samples
    assert d.shape == (N, 3) and r["valid"].all() and np.isfinite(d).all()
    norm = np.sqrt((d * d).sum(axis=1))
    print("largest | |dhat| - 1 | = %.3g (%.2f ulp)" % (np.abs(norm - 1).max(), np.abs(norm - 1).max() / 2.0 ** -52))
    assert np.abs(norm - 1.0).max() <= 4 * 2.0 ** -52
    nhat = normals / np.sqrt((normals * normals).sum(axis=1))[:, None]
    cos = (d * np.repeat(nhat, samples, axis=0)).sum(axis=1)
    print("smallest dhat . nhat = %.3g, mean %.6f (2/3 +- %.2g)" % (cos.min(), cos.mean(), 5 * math.sqrt((1 / 18) / N)))
    assert cos.min() >= 0.0      # (dhat . nhat = |dir| / 2, and no |dir| of this set is anywhere near 2^-26, where rounding could turn it)
    assert abs(cos.mean() - 2.0 / 3.0) <= 5 * math.sqrt((1.0 / 18.0) / N)
    # the origins, windows and times are the points' own, ray p * S + s
    assert (r["origin"] == 0).all() and (r["t_min"] == A.BIAS).all() and (r["t_max"] == math.inf).all() and (r["time"] == 0).all()


def test_the_seeds_keep_every_candidate_clear_of_the_acceptance_edge(orc, wall_draws):
    """No candidate, accepted or rejected, of the draws the GPU tests compare has | |c|^2 - 1 | < 2^-40: |c|^2 differs
    between the flavours by a few 2^-53 (contraction), so an acceptance there never flips."""
    for name, (seed, base, n, samples), got in (("wall", WALL, wall_draws), ("identity", IDENTITY, None)):
        u, edge, blocks = got if got is not None else A.draws(orc, seed, base, n, samples)
        print("%s: smallest | |c|^2 - 1 | = %.3g over %d candidates (%.3f per sample)" % (name, edge, blocks.sum(), blocks.mean()))
        assert edge >= 2.0 ** -40, name
        # the acceptance rate of a ball in its cube is pi / 6: the draws are the rejection loop's
        assert abs(1.0 / blocks.mean() - math.pi / 6.0) < 0.01, name
        assert (np.sqrt((u * u).sum(axis=-1)) < 1.0).all()


def test_the_draws_are_addressed_by_index_not_by_position(orc):
    """Point p of a batch that starts at index_base draws what point index_base + p of a batch from 0 draws, and another
    seed, sample or purpose draws something else."""
    whole = A.draws(orc, 11, 0, 8, 4)[0]
    tail = A.draws(orc, 11, 5, 3, 4)[0]
    assert np.array_equal(whole[5:], tail)
    assert not np.array_equal(whole, A.draws(orc, 12, 0, 8, 4)[0])
    assert np.array_equal(A.draws(orc, 11, 0, 8, 2)[0], whole[:, :2])
    # (the last index of the 32-bit range is one like any other)
    assert np.array_equal(A.draws(orc, 11, 2 ** 32 - 2, 2, 1)[0][1:], A.draws(orc, 11, 2 ** 32 - 1, 1, 1)[0])


def test_scaled_normals_and_invalid_points(orc):
    """Step 1 leaves a normal inside 2^+-32 alone and brings one outside it to [1, 2); the validity rule is the ray
    query's with the normal in the direction's place."""
    n = np.array([[3.0, -4.0, 0.0], [2.0 ** -40, 0.0, 0.0], [0.0, 3 * 2.0 ** 200, -2.0 ** 199], [5e-324, 0.0, 0.0]])
    s = A.scaled_normal(n)
    assert np.array_equal(s[0], n[0]) and np.array_equal(s[1], [1.0, 0.0, 0.0]) and np.array_equal(s[2], [0.0, 1.5, -0.25])
    assert s[3, 0] == 5e-324 * 2.0 ** 1022
    nan, inf = math.nan, math.inf
    pts = np.zeros((9, 3))
    nrm = np.tile([0.0, 1.0, 0.0], (9, 1))
    t_min, t_max, time = np.full(9, 1e-3), np.full(9, inf), np.zeros(9)
    pts[1, 0], nrm[2, 2], nrm[3] = nan, inf, 0.0
    time[4], t_min[5], t_min[6], t_max[7], t_max[8] = inf, -1e-9, inf, nan, 0.5e-3
    valid = A.valid_points(pts, nrm, t_min, t_max, time)
    assert valid.tolist() == [True] + [False] * 8
    r = A.rays(orc, pts, nrm, 2, t_min=t_min, t_max=t_max, time=time)
    assert (r["direction"][2:] == 0).all() and np.isfinite(r["direction"][:2]).all()


def test_the_model_counts_what_the_closed_forms_say(orc):
    floor, box = A.floor_and_box()
    rng = np.random.default_rng(3)
    n, samples = 24, 8
    on_floor = np.column_stack([rng.uniform(-5, 5, n), np.zeros(n), rng.uniform(-5, 5, n)])
    up = np.tile([0.0, 2.5, 0.0], (n, 1))
    assert (A.expected(orc, floor, on_floor, up, samples, seed=1) == samples).all()
    assert (A.expected(orc, floor, on_floor + [0.0, 1.0, 0.0], -up, samples, seed=1) < samples).any()      # looking down at it
    inside = rng.uniform(-0.5, 0.5, (n, 3))
    any_way = rng.normal(size=(n, 3))
    assert (A.expected(orc, box, inside, any_way, samples, seed=1) == 0).all()
    assert (A.expected(orc, box, inside, any_way, samples, seed=1, radius=0.4) == samples).all()
    bad = any_way.copy()
    bad[3] = 0.0
    got = A.expected(orc, box, inside, bad, samples, seed=1)
    assert got[3] == A.INVALID and (np.delete(got, 3) == 0).all()


def test_cli_refuses_bad_ao_values():
    """--ao's values are refused the way --pick's are: before a scene is loaded or a device is touched."""
    exe = os.path.join(ROOT, "racer-tracer_amd", "bin", "racer-tracer-amd")
    base = [exe, "-c", os.path.join(ROOT, "scenes", "config_c1.yml"), "-s", os.path.join(ROOT, "scenes", "three_balls.yml"),
            "--image-action", "none"]
    for bad in ("0", "3", "2048", "-4", "16,", "16,0", "16,-1", "16,nan", "16,x", "x", "", "16,1,2", "16.5"):
        r = subprocess.run(base + ["--ao", bad], capture_output=True, text=True, cwd=ROOT, timeout=60)
        assert r.returncode != 0 and r.stdout == "" and "--ao" in r.stderr, (bad, r.stderr)
    for other in (["--denoise"], ["--nee"], ["--devices", "2"], ["--adaptive", "0.1"]):
        r = subprocess.run(base + ["--ao", "16"] + other, capture_output=True, text=True, cwd=ROOT, timeout=60)
        assert r.returncode != 0 and "--ao" in r.stderr, (other, r.stderr)
