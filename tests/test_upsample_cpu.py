"""Guided upsampling (include/ptk.h ptk_upsample_planes) without a GPU: tests/upsample_rule.py, the numpy restatement the GPU tests
compare against, held to its purpose on the analytic scene of tests/temporal_rule.py - identity at equal sizes, exactness for a
colour that is constant per surface, holes as the only place a wrong surface's colour shows, texture detail from the high albedo
plane, NaN containment, monotone thresholds - and one check with the CPU oracle that the feature does its job."""
import numpy as np
import pytest

import feature_truth as FT
import ray_cases as RC
import temporal_rule as TR
import upsample_rule as UR

f32 = np.float32
CAM = TR.orbit_camera(10)


def planes(W, H):
    """(id, position, normal) of the analytic scene under CAM at W x H"""
    return TR.trace_analytic(TR.view_of(CAM, W, H), W, H)


def shares(cls, valid):
    return [float((cls[valid] == k).mean()) for k in range(3)]


def prm(wide=1, dist=TR.EXTENT / 100.0, dot=0.9):
    return UR.params(dist, dot, wide)


def test_equal_sizes_without_albedo_return_the_input():
    ident, pos, nrm = planes(96, 54)
    rng = np.random.default_rng(1)
    color = rng.uniform(0.0, 4.0, (54, 96, 3)).astype(f32)
    out, cls = UR.upsample((color, ident, pos, nrm, None), (ident, pos, nrm, None), prm())
    assert out.dtype == f32 and cls.dtype == np.int32
    assert np.array_equal(out, color)
    assert (cls == 0).all()


@pytest.mark.parametrize("w,h,expect", [(48, 27, (0.9984, 0.0008, 0.0008)), (32, 18, (0.984, 0.015, 0.001))])
def test_a_colour_constant_per_id_comes_back(w, h, expect):
    W, H = 96, 54
    lid, lp, ln = planes(w, h)
    hid, hp, hn = planes(W, H)
    color = TR.ALBEDO[np.maximum(lid, 0)].astype(f32)
    want = TR.ALBEDO[np.maximum(hid, 0)]
    lo, hi = (color, lid, lp, ln, None), (hid, hp, hn, None)
    out, cls = UR.upsample(lo, hi, prm(1))
    valid = hid >= 0
    s = shares(cls, valid)
    print(f"{w}x{h} -> {W}x{H}: class shares over valid pixels {s[0]:.4f} / {s[1]:.4f} / {s[2]:.4f}")
    assert np.allclose(s, expect, atol=6e-4), "the shares of the prototype this rule was written from"
    err = np.abs(out - want).max(axis=-1)
    assert err[valid & (cls < 2)].max() <= 1e-6
    # class 2 appears, and a wrong surface's colour shows nowhere else
    assert (cls[valid] == 2).any()
    assert not (err[valid] > 1e-6)[cls[valid] < 2].any()
    assert (err[valid & (cls == 2)] > 1e-3).any()
    if (w, h) == (48, 27):
        assert s[0] >= 0.95 and s[2] <= 0.01
    # wide = 0 turns every class 1 into class 2 and changes nothing else
    out0, cls0 = UR.upsample(lo, hi, prm(0))
    assert (cls == 1).any() and not (cls0 == 1).any()
    assert np.array_equal(cls0 == 2, (cls == 2) | (cls == 1))
    keep = cls != 1
    assert np.array_equal(out0[keep], out[keep]) and np.array_equal(cls0[keep], cls[keep])


def test_texture_detail_comes_from_the_high_albedo_plane():
    w, h, W, H = 48, 27, 96, 54
    lid, lp, ln = planes(w, h)
    hid, hp, hn = planes(W, H)
    # a checker of one high pixel: nothing of it survives at the low resolution
    def checker(Wc, Hc, period):
        y, x = np.mgrid[0:Hc, 0:Wc]
        return np.where((((x // period) + (y // period)) % 2 == 0)[..., None], f32(0.8), f32(0.2)) * np.ones(3, f32)
    lalb = checker(w, h, 1).astype(f32); halb = checker(W, H, 1).astype(f32)
    color = (f32(1.0) * (lalb + UR.ALBEDO_EPS)).astype(f32)               # demodulated colour exactly 1 on every low pixel
    out, cls = UR.upsample((color, lid, lp, ln, lalb), (hid, hp, hn, halb), prm())
    ok = (hid >= 0) & (cls < 2)
    want = f32(1.0) * (halb + UR.ALBEDO_EPS)
    assert np.abs(out - want)[ok].max() <= 1e-6
    # without albedo planes the same input is interpolated as it is: the checker is blurred
    flat, fcls = UR.upsample((color, lid, lp, ln, None), (hid, hp, hn, None), prm())
    assert np.array_equal(fcls, cls)
    assert np.abs(flat - want)[ok].max() > 0.1


def test_nan_in_invalid_low_pixels_reaches_no_valid_high_pixel():
    w, h, W, H = 32, 18, 96, 54
    lid, lp, ln = planes(w, h)
    hid, hp, hn = planes(W, H)
    rng = np.random.default_rng(2)
    color = rng.uniform(0.1, 2.0, (h, w, 3)).astype(f32)
    clean = UR.upsample((color, lid, lp, ln, None), (hid, hp, hn, None), prm())
    pcolor, ppos = color.copy(), lp.copy()
    assert (lid < 0).any()
    pcolor[lid < 0] = np.nan; ppos[lid < 0] = np.nan
    out, cls = UR.upsample((pcolor, lid, ppos, ln, None), (hid, hp, hn, None), prm())
    valid = (hid >= 0) & (cls < 2)
    assert np.isfinite(out[valid]).all()
    assert np.array_equal(cls, clean[1]) and np.array_equal(out[valid], clean[0][valid])


def test_looser_thresholds_only_move_pixels_toward_class_0():
    w, h, W, H = 32, 18, 96, 54
    lid, lp, ln = planes(w, h)
    hid, hp, hn = planes(W, H)
    color = TR.ALBEDO[np.maximum(lid, 0)].astype(f32)
    lo, hi = (color, lid, lp, ln, None), (hid, hp, hn, None)
    chain = [prm(1, TR.EXTENT / 2000.0, 0.9999), prm(1, TR.EXTENT / 400.0, 0.99), prm(1, TR.EXTENT / 100.0, 0.9), prm(1, TR.EXTENT, -1.0)]
    classes = [UR.upsample(lo, hi, p)[1] for p in chain]
    assert (classes[0] != classes[-1]).any(), "the tightest thresholds must reject something the loosest accept"
    for tight, loose in zip(classes, classes[1:]):
        assert (loose <= tight).all()


def test_it_does_its_job_on_the_cornell_box(oracle_mod):
    """Equal ray budgets: 48x32 at 16 spp upsampled to 96x64 against 96x64 at 4 spp, both measured against 96x64 at 256 spp
    (64 x the budget of the direct render).  Measured ratio rmse_up / rmse_direct: 0.40 (0.053 / 0.131), classes 0.996 / 0.004 / 0."""
    OB = oracle_mod
    arrays, cam = RC.scene("s_cornell")
    cam = dict(cam, aperture=0.0)
    o = OB.Oracle(arrays)
    ocam = OB.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], 0.0)
    low = o.render(ocam, 48, 32, 4, 0, 16, 5, want_rgb8=False)[0] / f32(16)
    direct = o.render(ocam, 96, 64, 4, 0, 4, 6, want_rgb8=False)[0] / f32(4)
    ref = o.render(ocam, 96, 64, 4, 0, 256, 7, want_rgb8=False)[0] / f32(256)
    o.close()
    fl = FT.truth(OB, arrays, cam, 48, 32, 5, 0)
    fh = FT.truth(OB, arrays, cam, 96, 64, 5, 0)
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    extent = float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))
    names = ("material", "position", "normal", "albedo")
    up, cls = UR.upsample((low,) + tuple(fl[k] for k in names), tuple(fh[k] for k in names), prm(1, extent / 100.0, 0.9))
    valid = fh["material"] >= 0
    rmse = lambda a: float(np.sqrt(np.mean((a[valid].astype(np.float64) - ref[valid]) ** 2)))
    ratio = rmse(up) / rmse(direct)
    print(f"s_cornell 48x32x16 -> 96x64 vs 96x64x4: rmse {rmse(up):.4f} / {rmse(direct):.4f} = {ratio:.3f}; classes {shares(cls, valid)}")
    assert ratio < 1
