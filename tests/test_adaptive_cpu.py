"""CPU tests of the adaptive render's numpy mirror (tests/adaptive_rule.py: the rule include/ptk.h ptk_render_adaptive documents,
which tests/test_gpu_adaptive.py holds the kernels to bit for bit) and of the render CLI's adaptive options."""
import numpy as np

import adaptive_rule as AR

f32 = np.float32


def _const(S, H, W, value):
    return np.full((S, H, W, 3), value, f32)


def test_constant_pixel_converges_at_min_spp():
    r = AR.adaptive(_const(64, 16, 16, 0.5), threshold=0.01, min_spp=16, step=4, max_spp=64)
    assert (r["n"] == 16).all() and r["rounds"] == 4 and r["active_pixels"] == 0
    assert np.array_equal(r["S1"], np.full((16, 16, 3), f32(8.0)))


def test_threshold_zero_never_converges():
    rng = np.random.default_rng(1)
    s = _const(32, 20, 24, 0.25)                     # even a noiseless pixel: err2 = 0 is not < 0
    s[:, :4] = rng.uniform(0, 1, (32, 4, 24, 3))
    r = AR.adaptive(s, threshold=0.0, min_spp=4, step=4, max_spp=32)
    assert (r["n"] == 32).all() and r["active_pixels"] == 20 * 24
    assert np.array_equal(r["S1"], AR.fold(s, np.full((20, 24), 32, np.uint32))[0])


def test_nan_never_converges():
    s = _const(16, 16, 16, 0.5)
    s[:, 3, 3, 1] = np.nan
    r = AR.adaptive(s, threshold=1e6, min_spp=4, step=2, max_spp=16)
    assert r["n"][3, 3] == 16
    assert AR.done(np.array([[np.nan, 0, 0]], f32), np.zeros((1, 3), f32), np.array([4]), 1e6).tolist() == [False]


def test_dilation_crosses_quadrants_but_not_tiles():
    # one noisy pixel at top-down (7, 7) - the corner of quadrant 0 of tile 0 - and one at (15, 16): the left edge of tile 1
    H, W = 32, 32
    need_top = np.zeros((H, W), bool)
    need_top[7, 7] = True
    need_top[15, 16] = True
    d = AR.dilate_in_tiles(need_top[::-1])[::-1]
    expect = np.zeros((H, W), bool)
    expect[6:9, 6:9] = True                          # reaches quadrants 1, 2 and 3 of tile 0
    expect[14:16, 16:18] = True                      # stays in tile 1: not row 16 (tile row 1), not column 15 (tile 0)
    assert np.array_equal(d, expect)


def test_active_set_only_shrinks_and_counts_follow_it():
    rng = np.random.default_rng(7)
    H, W, S = 40, 37, 48
    scale = rng.uniform(0, 1, (H, W, 1)) ** 4
    s = (0.3 + scale * rng.normal(0, 1, (S, H, W, 3))).astype(f32)
    active = AR.owned_mask(W, H)
    n = np.zeros((H, W), np.uint32)
    counts = set()
    for r in range(S // 4):
        n[active] += 4
        S1, S2 = AR.fold(s[:(r + 1) * 4], n)
        new = AR.next_active(active, S1, S2, n, 0.05, test=(r + 1) * 4 >= 8)
        assert not (new & ~active).any()
        active = new
    counts = set(np.unique(n).tolist())
    r = AR.adaptive(s, 0.05, 8, 4, S)
    assert np.array_equal(r["n"], n) and len(counts) >= 3
    assert r["rgb8"].dtype == np.uint8


def test_split_owned_pixels_partition_the_frame():
    W, H = 53, 37
    total = sum(AR.owned_mask(W, H, k, 3).astype(int) for k in range(3))
    assert (total == 1).all()


def test_render_cli_parses_noise_threshold():
    from pbrpathtracer_amd import render
    a = render.build_parser().parse_args(["s.pts", "--noise-threshold", "0.02", "--min-spp", "16", "--step", "4", "--spp", "256"])
    assert (a.noise_threshold, a.min_spp, a.step, a.spp) == (0.02, 16, 4, 256)
    a = render.build_parser().parse_args(["s.pts"])
    assert a.noise_threshold is None
