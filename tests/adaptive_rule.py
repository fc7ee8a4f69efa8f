"""numpy float32 mirror of the adaptive render (include/ptk.h ptk_render_adaptive): the convergence rule, the dilation within
16x16 tiles and the round loop.  Given every sample of every pixel, it says what each pixel must hold afterwards: its count
n_p, S1 and S2 folded in sample order, and the 8-bit resolve S1 / n_p.

Layout: everything as the accumulator lies - rows bottom-up, [H][W] / [H][W][3] - like ptk_read_accum; the tile geometry
(16x16 tiles from the image's top-left, the rank's tiles, include/ptk.h ptk_set_tile) is applied to the flipped rows."""
import numpy as np

TILE = 16
f32 = np.float32


def owned_mask(W, H, rank=0, world=1):
    """[H][W] bool, rows bottom-up: the pixels of the tiles `rank` owns."""
    tiles_x, tiles_y = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    top = np.zeros((H, W), bool)
    for tile in range(rank, tiles_x * tiles_y, world):
        ty = tile // tiles_x
        tx = (tile % tiles_x + tiles_x - (3 * ty) % tiles_x) % tiles_x
        top[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = True
    return top[::-1]


def done(S1, S2, n, threshold):
    """The rule, operation by operation in float32.  S1, S2: [..., 3] float32; n: [...] counts (> 1)."""
    with np.errstate(all="ignore"):
        nf = n.astype(f32)
        m = S1.astype(f32) / nf[..., None]
        v = S2.astype(f32) / nf[..., None] - m * m
        v = np.where(v < f32(0), f32(0), v).astype(f32)          # (NaN < 0 is False: NaN stays)
        err2 = ((v[..., 0] + v[..., 1]) + v[..., 2]) / (f32(3.0) * (nf - f32(1.0)))
        lum = ((m[..., 0] + m[..., 1]) + m[..., 2]) / f32(3.0)
        tol = f32(threshold) * (lum + f32(1.0) / f32(256.0))
        return err2 < tol * tol


def dilate_in_tiles(need):
    """[H][W] bool (rows bottom-up) -> pixels with a `need` pixel in their 3x3 neighbourhood within the same 16x16 tile."""
    top = need[::-1]
    H, W = top.shape
    out = np.zeros_like(top)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sy, sx = ys + dy, xs + dx
            ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W) & (sy // TILE == ys // TILE) & (sx // TILE == xs // TILE)
            out |= ok & top[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)]
    return out[::-1]


def next_active(active, S1, S2, n, threshold, test=True):
    """One convergence step: the active set of the next round."""
    if not test:
        return active.copy()
    need = active & ~done(S1, S2, n, threshold)
    return active & dilate_in_tiles(need)


def fold(samples, n_p):
    """S1, S2 of every pixel over its first n_p samples, in sample order (float32 adds; S2 = S2 + v*v)."""
    S = samples.shape[0]
    S1 = np.zeros(samples.shape[1:], f32)
    S2 = np.zeros(samples.shape[1:], f32)
    for s in range(S):
        take = (n_p > s)[..., None]
        v = samples[s].astype(f32)
        S1 = np.where(take, S1 + v, S1).astype(f32)
        S2 = np.where(take, S2 + v * v, S2).astype(f32)
    return S1, S2


def resolve_rgb8(S1, n_p):
    """pathtracer.cpp:802-812 by each pixel's own count (0 where n_p = 0)."""
    with np.errstate(all="ignore"):
        x = S1 / n_p.astype(f32)[..., None]
    x = np.where(x < 0, f32(0), np.where(x > 1, f32(1), x))
    x = np.where(np.isnan(x), f32(0), x).astype(f32)
    return (x * f32(255)).astype(np.uint8)


def adaptive(samples, threshold, min_spp, step, max_spp, rank=0, world=1):
    """The round loop.  samples: [S >= max_spp][H][W][3] float32, rows bottom-up (sample s of a plain render).  Returns
    dict(n [H][W] uint32, S1, S2 [H][W][3] float32, rgb8 [H][W][3], rounds, active_pixels)."""
    S, H, W, _ = samples.shape
    assert S >= max_spp and step >= 2 and min_spp % step == 0 and max_spp % step == 0 and min_spp <= max_spp
    active = owned_mask(W, H, rank, world)
    n = np.zeros((H, W), np.uint32)
    rounds = 0
    for r in range(max_spp // step):
        if not active.any():
            break
        n[active] += step
        rounds += 1
        S1, S2 = fold(samples[:(r + 1) * step], n)
        active = next_active(active, S1, S2, n, threshold, test=(r + 1) * step >= min_spp)
    S1, S2 = fold(samples[:max(max_spp, 1)], n)
    rgb = resolve_rgb8(S1, n)
    rgb[n == 0] = 0
    return dict(n=n, S1=S1, S2=S2, rgb8=rgb, rounds=rounds, active_pixels=int(active.sum()))


def oracle_samples(o, ocam, W, H, depth, count, seed):
    """Per-sample values of a plain render from the CPU oracle: sample s = render(s, 1) on a zeroed total."""
    return np.stack([o.render(ocam, W, H, depth, s, 1, seed, want_rgb8=False)[0] for s in range(count)]).astype(f32)
