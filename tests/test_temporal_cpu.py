"""Properties of tests/temporal_rule.py, the numpy float32 mirror of temporal reprojection (include/ptk.h ptk_reproject_planes) - no
GPU.  The GPU tests (tests/test_gpu_temporal.py) hold the kernels to this mirror bit for bit; these hold the mirror to what the rule
is for."""
import numpy as np
import pytest

import temporal_rule as TR

f32 = np.float32
W, H = 96, 54


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def case():
    return TR.random_case(W, H, seed=7)


def defaults(**kw):
    return dict(TR.params(TR.EXTENT / 100.0), **kw)


def test_view_is_an_orthonormal_image_plane():
    for deg in (0.0, 10.0, 77.0, 200.0):
        v = TR.view_of(TR.orbit_camera(deg), W, H)
        r, u = v["right"].astype(np.float64), v["up"].astype(np.float64)
        assert abs(r @ u) < 1e-6 and abs(r @ r - 1) < 1e-6 and abs(u @ u - 1) < 1e-6
        assert v["delta_x"] > 0 and abs(float(v["delta_x"]) / float(v["delta_y"]) - 1) < 1e-6          # square pixels
        assert all(v[k].dtype == f32 for k in ("pos", "right", "up", "top_left"))


def test_self_projection_returns_every_pixel_to_itself():
    """(a) a pixel's first hit projected through its own view lands on its own column and row (the prototype measured 1e-5)"""
    worst = 0.0
    for deg in (0.0, 10.0, 33.0):
        view = TR.view_of(TR.orbit_camera(deg), W, H)
        ident, pos, _ = TR.trace_analytic(view, W, H)
        col, row, s = TR.project(view, pos)
        valid = ident >= 0
        assert valid.mean() > 0.25 and (~valid).any()
        j = np.broadcast_to(np.arange(W)[None, :], (H, W)); i = np.broadcast_to((H - 1 - np.arange(H))[:, None], (H, W))
        assert col.dtype == f32 and row.dtype == f32 and (s[valid] > 0).all()
        worst = max(worst, np.abs(col - j)[valid].max(), np.abs(row - i)[valid].max())
    print("self-projection: worst offset %.3g pixels" % worst)
    assert worst < 1e-3


def test_constant_radiance_stays_constant_and_counts_add(case):
    """(b) a history of 0.5 blended with a frame of 0.5 is exactly 0.5 under any view, and the counts add"""
    color, count, ident, pos, nrm = case["current"]
    hcolor, hcount, hident, hpos, hnrm = case["history"]
    cur = (np.full_like(color, 0.5), np.where(ident >= 0, count, f32(0)), ident, pos, nrm)
    hist = (np.full_like(hcolor, 0.5), np.full_like(hcount, 4.0), hident, hpos, hnrm)
    out, n, found = TR.reproject(case["hist_view"], cur, hist, defaults(), want_found=True)
    valid = ident >= 0
    assert (out[valid] == f32(0.5)).all()
    assert found.sum() > 1000 and (n[found] == cur[1][found] + f32(4)).all()
    assert (valid & ~found).any() and np.array_equal(n[~found], cur[1][~found])
    assert (cur[1][found] == 0).any()               # (pixels without samples of their own take the history's count)


def test_count_saturates_at_max_history_plus_one():
    """(c) one sample per frame under the identity view: the count climbs to max_history + 1 and stays"""
    rng = np.random.default_rng(3)
    view, (color, _, ident, pos, nrm) = TR.planes_under(TR.orbit_camera(10.0), W, H, rng, poison=False)
    valid = ident >= 0
    one = np.where(valid, f32(1), f32(0)).astype(f32)
    p = defaults(max_history=4.0)
    out, n = TR.no_history((color, one))
    seen = []
    for _ in range(8):
        out, n = TR.reproject(view, (color, one, ident, pos, nrm), (out, n, ident, pos, nrm), p)
        seen.append(n[valid].copy())
    assert (seen[0] == 2).all()
    for a, b in zip(seen, seen[1:]):
        assert (b >= a).all()
    assert (seen[-1] == 5).all() and (seen[-2] == 5).all() and (seen[-3] == 5).all()
    assert np.array_equal(n[~valid], one[~valid])


def test_nothing_to_find_gives_the_current_bits(case):
    """(d) points behind the history camera, NaN positions and a history of invalid ids: the current frame's bits"""
    cur, hist = case["current"], case["history"]
    # a camera on the far side that outside the box that looks away from it: every point lies behind it
    away = TR.orbit_camera(180.0, distance=3.0)
    away["dir"] = (-np.asarray(away["dir"])).astype(f32)
    _, _, s = TR.project(TR.view_of(away, W, H), np.nan_to_num(cur[3]))
    assert (s[cur[2] >= 0] < 0).all()
    out, n = TR.reproject(TR.view_of(away, W, H), cur, hist, defaults())
    assert np.array_equal(bits(out), bits(cur[0])) and np.array_equal(bits(n), bits(cur[1]))
    nanpos = (cur[0], cur[1], cur[2], np.full_like(cur[3], np.nan), cur[4])
    out, n = TR.reproject(case["hist_view"], nanpos, hist, defaults())
    assert np.array_equal(bits(out), bits(cur[0])) and np.array_equal(bits(n), bits(cur[1]))
    dead = (hist[0], hist[1], np.full_like(hist[2], -1), hist[3], hist[4])
    out, n = TR.reproject(case["hist_view"], cur, dead, defaults())
    assert np.array_equal(bits(out), bits(cur[0])) and np.array_equal(bits(n), bits(cur[1]))


def test_invalid_pixels_keep_their_bits_and_reach_nobody(case):
    """(e) invalid pixels of either frame hold NaN and 1e30: the current ones keep their bits, and no valid pixel sees any"""
    cur, hist = case["current"], case["history"]
    inv = cur[2] < 0
    assert inv.any() and np.isnan(cur[0][inv]).all() and (cur[1][inv] == f32(1e30)).all() and np.isnan(hist[0][hist[2] < 0]).all()
    for match in (0, 1):
        out, n, found = TR.reproject(case["hist_view"], cur, hist, defaults(match_id=match), want_found=True)
        assert np.array_equal(bits(out)[inv], bits(cur[0])[inv]) and np.array_equal(bits(n)[inv], bits(cur[1])[inv])
        assert np.isfinite(out[~inv]).all() and np.isfinite(n[~inv]).all() and (n[~inv] <= 64 + 8).all()
        assert not found[inv].any()
        assert not np.array_equal(out[found], cur[0][found])


def test_the_cases_exercise_both_outcomes(case):
    """(f) at a 3 degree orbit step most but not all valid pixels find history (the analytic prototype: 0.95 at 3 degrees, 0.83 at 10)"""
    cur = case["current"]
    _, _, found = TR.reproject(case["hist_view"], cur, case["history"], defaults(), want_found=True)
    frac = found.sum() / (cur[2] >= 0).sum()
    wide = TR.random_case(W, H, seed=7, degrees=10.0)
    _, _, found10 = TR.reproject(wide["hist_view"], wide["current"], wide["history"], defaults(), want_found=True)
    frac10 = found10.sum() / (wide["current"][2] >= 0).sum()
    print("found history: %.3f at 3 degrees, %.3f at 10 degrees" % (frac, frac10))
    assert 0.80 <= frac <= 0.99
    assert frac10 < frac


def test_parameters_do_what_they_say(case):
    cur, hist = case["current"], case["history"]
    base = TR.reproject(case["hist_view"], cur, hist, defaults(), want_found=True)
    loose = TR.reproject(case["hist_view"], cur, hist, defaults(match_id=0, min_normal_dot=-1.0, max_plane_dist=100.0), want_found=True)
    assert loose[2].sum() > base[2].sum() and (loose[2] | ~base[2]).all()
    capped = TR.reproject(case["hist_view"], cur, hist, defaults(max_history=1.0), want_found=True)
    f = capped[2] & (cur[1] > 0)
    assert np.array_equal(capped[2], base[2]) and (capped[1][f] == cur[1][f] + f32(1)).all()
