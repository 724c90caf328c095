"""numpy restatement of csrc/rt_variance_filter.hip: the definition the variance-filter kernels are held to.

A still frame's variance-guided filter.  The input is what an adaptive render leaves behind: per pixel and channel the
running sum S and Q = sum_j S_j^2 / n_j over the chunks done [H, W, 3], and per pixel the samples s and the chunks k of
its tile [H, W] int.  Guides are denoise_model's; the levels are temporal_model's (the kernels behind them are shared), the
spatial fall-back is temporal_model.variance on a length-1 history.  The arithmetic follows the kernels' order, so the two
agree to rounding.
"""
import numpy as np

import denoise_model as M
import temporal_model as T

DEMODULATE = M.DEMODULATE
LUMA = T.LUMA
DEFAULTS = dict(sigma_luminance=4.0, min_chunks=4)


def chunk_sums(chunk_means, counts):
    """(S, Q) of a pixel's chunks: chunk_means[j] [..., 3] the mean radiance of chunk j over counts[j] samples, added in
    chunk order as the renderer does."""
    S = Q = None
    for mean, n in zip(chunk_means, counts):
        Sj = np.asarray(mean, dtype=np.float64) * n
        S = Sj if S is None else S + Sj
        Q = Sj * Sj / n if Q is None else Q + Sj * Sj / n
    return S, Q


def sigma(S, Q, s, k):
    """rt_abi.h's adaptive sigma per channel: sqrt(max(0, Q - S m) / (k - 1) / s) with m = S / s (k >= 2)."""
    s3, k3 = np.asarray(s, dtype=np.float64)[..., None], np.asarray(k, dtype=np.float64)[..., None]
    m = S / s3
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(np.maximum(0.0, Q - S * m) / (k3 - 1.0) / s3)


def batch_variance(S, Q, samples, chunks, guides, flags=DEMODULATE, min_chunks=4, sigma_normal=0.1, sigma_plane=1.0,
                   **_unused):
    """rt_batch_variance_device -> (C [H, W, 3], var [H, W]): C = (S / s) / a with a = max(albedo, 1e-3) or 1; var the
    squared luminance of sigma / a where k >= min_chunks, 0 on a guide miss, else the 7x7 spatial estimate over C."""
    S, Q = np.asarray(S, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    a = np.maximum(guides["albedo"], 1e-3) if flags & DEMODULATE else np.ones_like(S)
    C = (S / np.asarray(samples, dtype=np.float64)[..., None]) / a
    sp = sigma(S, Q, samples, chunks) / a
    sl = LUMA[0] * sp[..., 0] + LUMA[1] * sp[..., 1] + LUMA[2] * sp[..., 2]
    batch = np.asarray(chunks) >= min_chunks
    var = np.where(batch, sl * sl, 0.0)
    if not batch.all():
        l = T.luminance(C)
        once = {"radiance": C, "moments": np.stack([l, l * l], axis=-1), "length": np.ones(l.shape)}
        var = np.where(batch, var, T.variance(once, guides, sigma_normal, sigma_plane))
    var[guides["obj_id"] < 0] = 0.0
    return C, var


def denoise_variance(C, var, guides, iterations=5, flags=DEMODULATE, sigma_color=0.0, sigma_normal=0.1, sigma_plane=1.0,
                     sigma_luminance=4.0, **_unused):
    """rt_denoise_variance_device: the levels over (C, var), then sqrt(max(C albedo, 0)) -> the gamma-encoded frame."""
    I = C
    if sigma_luminance > 0:
        for i in range(iterations):
            I, var = T.atrous_var(I, var, guides, i, sigma_color, sigma_normal, sigma_plane, sigma_luminance)
    else:
        for i in range(iterations):
            I = M.atrous(I, guides, i, sigma_color, sigma_normal, sigma_plane)
    L = I * guides["albedo"] if flags & DEMODULATE else I
    return np.sqrt(np.maximum(L, 0.0))


def filter_frame(S, Q, samples, chunks, guides, dparams, sigma_luminance=4.0, min_chunks=4):
    """Both steps, dparams being denoise_model.params_kwargs' dict -> (filtered frame, var)."""
    C, var = batch_variance(S, Q, samples, chunks, guides, flags=dparams["flags"], min_chunks=min_chunks,
                            sigma_normal=dparams["sigma_normal"], sigma_plane=dparams["sigma_plane"])
    return denoise_variance(C, var, guides, sigma_luminance=sigma_luminance, **dparams), var


def filter_kwargs(fp):
    """An abi.RtVarianceFilterParams as keyword arguments."""
    return dict(sigma_luminance=fp.sigma_luminance, min_chunks=fp.min_chunks)


def chunks_of(samples, bounds):
    """The chunks done at every pixel: samples [H, W] are boundaries of the frame's chunk plan, bounds those boundaries
    without the leading 0."""
    lut = {b: c + 1 for c, b in enumerate(bounds)}
    return np.vectorize(lut.__getitem__, otypes=[np.int32])(samples)
