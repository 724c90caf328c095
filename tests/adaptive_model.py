"""numpy restatement of rt_render_adaptive's tile error and stop rule (include/rt_abi.h).

The input is what a progressive render hands out: the cumulative frame f_c at every chunk boundary b_c of the frame's
chunk plan (rt_render_progressive with pass_samples = 1).  The running sum of a pixel after c chunks is S_c = f_c^2 b_c
and the chunk sums are the differences between boundaries."""
import numpy as np


def pixel_error(S, Q, s, k):
    """e of every pixel and channel from the running sums S, the sums of squares Q = sum_j S_j^2 / n_j, the samples s and
    the chunks k (>= 2): sigma / (sqrt(m + sigma) + sqrt(m)) with m = S / s, V = max(0, Q - S m) / (k - 1),
    sigma = sqrt(V / s); 0 where sigma = 0."""
    S = np.asarray(S, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    m = S / s
    var = np.maximum(0.0, Q - S * m) / (k - 1)
    sigma = np.sqrt(var / s)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(sigma > 0.0, sigma / (np.sqrt(m + sigma) + np.sqrt(m)), 0.0)


def pixel_error_difference_form(S, Q, s, k):
    """The same quantity written as sqrt(m + sigma) - sqrt(m) (cancels badly where sigma << m; for the tests only)."""
    m = np.asarray(S, dtype=np.float64) / s
    sigma = np.sqrt(np.maximum(0.0, np.asarray(Q, dtype=np.float64) - np.asarray(S, dtype=np.float64) * m) / (k - 1) / s)
    return np.sqrt(m + sigma) - np.sqrt(m)


def tile_max(e):
    """[H, W, 3] -> [ceil(H/8), ceil(W/8)]: the largest value over each 8x8 tile's pixels inside the image and channels."""
    h, w = e.shape[:2]
    th, tw = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((th * 8, tw * 8), dtype=np.float64)
    pad[:h, :w] = e.max(axis=-1)
    return pad.reshape(th, 8, tw, 8).max(axis=(1, 3))


def sums_at_boundaries(frames, bounds):
    """frames[c]: the cumulative frame at chunk boundary bounds[c] (bounds without the leading 0) -> (S[c], Q[c]), the
    running sums and sums of squares after c + 1 chunks."""
    S_prev = None
    Q = None
    S_all, Q_all = [], []
    prev_b = 0
    for f, b in zip(frames, bounds):
        S = np.asarray(f, dtype=np.float64) ** 2 * b
        Sj = S if S_prev is None else S - S_prev
        q = Sj * Sj / (b - prev_b)
        Q = q if Q is None else Q + q
        S_all.append(S)
        Q_all.append(Q)
        S_prev, prev_b = S, b
    return S_all, Q_all


def tile_errors(S, Q, s, k):
    """Every tile's error after k chunks (s samples); -1 with fewer than 2 chunks."""
    if k < 2:
        return np.full(tile_max(np.zeros_like(S)).shape, -1.0)
    return tile_max(pixel_error(S, Q, s, k))


def simulate(frames, bounds, pass_bounds, threshold, min_samples):
    """The stop rule over the passes ending at pass_bounds (a subset of bounds ending at N).
    -> (samples per tile [ty, tx], every tile's error at its last pass, {pass boundary: errors of that pass})."""
    S_all, Q_all = sums_at_boundaries(frames, bounds)
    n = bounds[-1]
    shape = tile_max(np.zeros_like(S_all[0])).shape
    running = np.ones(shape, dtype=bool)
    samples = np.full(shape, n, dtype=np.int64)
    last_err = np.full(shape, -1.0)
    per_pass = {}
    for b in pass_bounds:
        c = bounds.index(b)
        k = c + 1
        err = tile_errors(S_all[c], Q_all[c], b, k)
        per_pass[b] = err
        last_err = np.where(running, err, last_err)
        if threshold > 0 and k >= 4 and b >= min_samples:
            stop = running & (err <= threshold)
            samples[stop] = b
            running &= ~stop
        if not running.any():
            break
    return samples, last_err, per_pass


def expand(tiles, h, w):
    """[ty, tx] -> [h, w]: every pixel takes its tile's value."""
    return np.repeat(np.repeat(tiles, 8, axis=0), 8, axis=1)[:h, :w]
