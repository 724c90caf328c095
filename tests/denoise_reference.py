"""The denoiser of DESIGN.md 4.6 restated from its text alone, in mpmath at 40 significant digits: an independent reference
for tests/denoise_model.py (and through it the device kernels of csrc/rt_denoise.hip).

Plain per-pixel loops, nothing shared with the model: every input double is taken exactly, every operation is carried at
40 digits and the result is rounded to f64 once, at the end.  The definition, from DESIGN.md 4.6:
  demod    I = g^2 / max(albedo, 1e-3) per channel (or g^2 with demodulation off);
  level i  step s = 2^i; I'_p = sum_q w_pq I_q / sum_q w_pq over q = p + s (dx, dy), dx, dy in -2..2, taps outside the
           image dropped; w_pq = h(dx) h(dy) [id_p = id_q] w_n w_x w_c with h = (1, 4, 6, 4, 1) / 16,
           w_n = exp(-|n_p - n_q|^2 / sigma_n^2), w_x = exp(-(n_p . (x_q - x_p))^2 / (sigma_x s footprint_p)^2),
           w_c = exp(-|sqrt I_p - sqrt I_q|^2 / (sigma_c 2^-i)^2); a sigma <= 0 switches its stop off; a miss (id < 0)
           passes through;
  remod    sqrt(max(I_K albedo, 0)) (or sqrt(max(I_K, 0))); K = 0 is an exact copy.

`footprint_of` and `color_halves` exist only so that a test can show the fixture tells the definition from two plausible
misreadings of it (the plane stop scaled by the neighbour's footprint, a colour stop that does not narrow per level).
"""
import mpmath

DIGITS = 40
DEMODULATE = 1


def denoise(rgb, guides, iterations=5, flags=DEMODULATE, sigma_color=0.0, sigma_normal=0.1, sigma_plane=1.0,
            footprint_of="p", color_halves=True):
    """rgb [H, W, 3] (anything indexable as rgb[y][x][c], or a numpy array) -> list of rows of [r, g, b] python floats."""
    ctx = mpmath.mp.clone()
    ctx.dps = DIGITS
    mpf = ctx.mpf
    height, width = len(rgb), len(rgb[0])
    if iterations == 0:
        return [[[float(rgb[y][x][c]) for c in range(3)] for x in range(width)] for y in range(height)]

    ids = [[int(guides["obj_id"][y][x]) for x in range(width)] for y in range(height)]
    normal = [[[mpf(float(guides["normal"][y][x][c])) for c in range(3)] for x in range(width)] for y in range(height)]
    position = [[[mpf(float(guides["position"][y][x][c])) for c in range(3)] for x in range(width)] for y in range(height)]
    albedo = [[[mpf(float(guides["albedo"][y][x][c])) for c in range(3)] for x in range(width)] for y in range(height)]
    footprint = [[float(guides["footprint"][y][x]) for x in range(width)] for y in range(height)]
    demodulate = (flags & DEMODULATE) != 0
    floor = mpf("0.001")
    h = [mpf(1) / 16, mpf(4) / 16, mpf(6) / 16, mpf(4) / 16, mpf(1) / 16]
    sn, sx, sc = mpf(float(sigma_normal)), mpf(float(sigma_plane)), mpf(float(sigma_color))

    # demodulation
    I = [[[None] * 3 for _ in range(width)] for _ in range(height)]
    for y in range(height):
        for x in range(width):
            for c in range(3):
                g = mpf(float(rgb[y][x][c]))
                L = g * g
                I[y][x][c] = L / max(albedo[y][x][c], floor) if demodulate else L

    # K a-trous levels
    for i in range(iterations):
        s = 2 ** i
        sigma_c_i = sc / mpf(2) ** i if color_halves else sc
        root = [[[ctx.sqrt(v) for v in px] for px in row] for row in I]
        out = [[None] * width for _ in range(height)]
        for py in range(height):
            for px in range(width):
                if ids[py][px] < 0:     # a miss passes through
                    out[py][px] = list(I[py][px])
                    continue
                acc = [mpf(0), mpf(0), mpf(0)]
                wsum = mpf(0)
                for dy in range(-2, 3):
                    qy = py + s * dy
                    if qy < 0 or qy >= height:
                        continue
                    for dx in range(-2, 3):
                        qx = px + s * dx
                        if qx < 0 or qx >= width:
                            continue
                        if ids[qy][qx] != ids[py][px]:
                            continue
                        w = h[dx + 2] * h[dy + 2]
                        if sigma_normal > 0:
                            d2 = sum((normal[py][px][c] - normal[qy][qx][c]) ** 2 for c in range(3))
                            w *= ctx.exp(-d2 / (sn * sn))
                        if sigma_plane > 0:
                            fp = footprint[py][px] if footprint_of == "p" else footprint[qy][qx]
                            plane = sum(normal[py][px][c] * (position[qy][qx][c] - position[py][px][c]) for c in range(3))
                            scale = sx * s * mpf(fp)
                            w *= ctx.exp(-(plane * plane) / (scale * scale))
                        if sigma_color > 0:
                            d2 = sum((root[py][px][c] - root[qy][qx][c]) ** 2 for c in range(3))
                            w *= ctx.exp(-d2 / (sigma_c_i * sigma_c_i))
                        for c in range(3):
                            acc[c] += w * I[qy][qx][c]
                        wsum += w
                out[py][px] = [acc[c] / wsum for c in range(3)]
        I = out

    # remodulation, then the one rounding to f64
    result = []
    for y in range(height):
        row = []
        for x in range(width):
            px = []
            for c in range(3):
                L = I[y][x][c] * albedo[y][x][c] if demodulate else I[y][x][c]
                px.append(float(ctx.sqrt(max(L, mpf(0)))))
            row.append(px)
        result.append(row)
    return result
