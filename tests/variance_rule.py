"""numpy float32 mirror of the temporal luminance moments and the variance made of them (include/ptk.h ptk_reproject_moments,
ptk_temporal_frame_moments, ptk_variance_planes, ptk_denoise_temporal) - a helper, no tests of its own.  Written from the header
text: vectorised over pixels, sequential over the taps in the stated order, every intermediate a float32 array, one numpy operation
per stated operation.  The projection is tests/temporal_rule.py's; the taps and the blend are restated here with the two moment
channels beside the colour, and nothing in temporal_rule or motion_rule is changed.

Layout: planes [H][W] or [H][W][c] as stored (the reprojection: rows BOTTOM-UP; the variance never flips)."""
import numpy as np

import temporal_rule as TR

f32 = np.float32
PTK_TEMPORAL_RESET, PTK_TEMPORAL_MOVING = 1, 2
PTK_DENOISE_VARIANCE = 1
_dot = TR._dot


def params(extent, radius=3, prefilter=1, min_frames=4.0, min_normal_dot=0.9):
    return dict(radius=int(radius), prefilter=int(prefilter), min_frames=float(min_frames), max_plane_dist=float(extent) / 100.0,
                min_normal_dot=float(min_normal_dot))


def lum(d):
    return ((f32(0.2126) * d[..., 0]) + (f32(0.7152) * d[..., 1])) + (f32(0.0722) * d[..., 2])


def current_moments(color, count, ident, albedo=None):
    """(cm1, cm2) of the current frame: l and l*l of the demodulated colour on valid pixels with samples, else 0"""
    color = np.ascontiguousarray(color, f32); count = np.ascontiguousarray(count, f32)
    with np.errstate(all="ignore"):
        d = color
        if albedo is not None:
            A = np.ascontiguousarray(albedo, f32) + f32(0.00390625)
            d = color / A
        l = lum(d)
        on = (np.asarray(ident) >= 0) & (count > 0)
        return np.where(on, l, f32(0)).astype(f32), np.where(on, l * l, f32(0)).astype(f32)


def reproject_moments(view, current, history, hist_moments, p, albedo=None, prev=None, want_found=False):
    """ptk_reproject_moments.  current, history: the five planes of temporal_rule.reproject; hist_moments [H][W][2]; prev: None or
    (prev_position, prev_normal), the MOVING rule.  Returns (out_color, out_count, out_moments)."""
    p = p.as_dict() if hasattr(p, "as_dict") else p
    color, count, position, normal = (np.ascontiguousarray(current[k], f32) for k in (0, 1, 3, 4))
    ident = np.ascontiguousarray(current[2], np.int32)
    hcolor, hcount, hposition, hnormal = (np.ascontiguousarray(history[k], f32) for k in (0, 1, 3, 4))
    hident = np.ascontiguousarray(history[2], np.int32)
    hmom = np.ascontiguousarray(hist_moments, f32)
    Y, m = (position, normal) if prev is None else (np.ascontiguousarray(prev[0], f32), np.ascontiguousarray(prev[1], f32))
    H, W = count.shape
    mpd = f32(p["max_plane_dist"]); mnd = f32(p["min_normal_dot"]); maxh = f32(p["max_history"]); match = bool(p["match_id"])
    cm1, cm2 = current_moments(color, count, ident, albedo)
    with np.errstate(all="ignore"):
        zz = mpd * mpd
        col, row, s = TR.project(view, Y)
        valid = ident >= 0
        ok = valid & (s > 0) & (col > f32(-1)) & (col < f32(W)) & (row > f32(-1)) & (row < f32(H))
        col = np.where(ok, col, f32(0)); row = np.where(ok, row, f32(0))
        x0 = np.floor(col).astype(np.int32); fx = col - x0.astype(f32)
        i0 = np.floor(row).astype(np.int32); fy = row - i0.astype(f32)
        gx = f32(1.0) - fx; gy = f32(1.0) - fy
        b4 = (gx * gy, fx * gy, gx * fy, fx * fy)
        sc = np.zeros((H, W, 3), f32); sn = np.zeros((H, W), f32); sw = np.zeros((H, W), f32)
        sm1 = np.zeros((H, W), f32); sm2 = np.zeros((H, W), f32)
        for k in range(4):
            qx = x0 + (k & 1); qi = i0 + (k >> 1)
            inside = ok & (qx >= 0) & (qx < W) & (qi >= 0) & (qi < H)
            cx = np.clip(qx, 0, W - 1); cy = np.clip(H - 1 - qi, 0, H - 1)
            hc = hcolor[cy, cx]; hn = hcount[cy, cx]; hi = hident[cy, cx]; hp = hposition[cy, cx]; hm = hnormal[cy, cx]; hq = hmom[cy, cx]
            b = b4[k]
            z = _dot(m, hp - Y)
            cn = _dot(m, hm)
            take = inside & (hi >= 0) & (hn > 0) & (b > 0) & ((z * z) <= zz) & (cn >= mnd)
            if match:
                take &= hi == ident
            sc = np.where(take[..., None], sc + (b[..., None] * hc), sc)
            sn = np.where(take, sn + (b * hn), sn)
            sw = np.where(take, sw + b, sw)
            sm1 = np.where(take, sm1 + (b * hq[..., 0]), sm1)
            sm2 = np.where(take, sm2 + (b * hq[..., 1]), sm2)
        found = ok & (sw > 0)
        hcol = sc / sw[..., None]
        hm1 = sm1 / sw; hm2 = sm2 / sw
        hw = sn / sw
        hw = np.where(hw > maxh, maxh, hw)
        tot = hw + count
        blend = ((hcol * hw[..., None]) + (color * count[..., None])) / tot[..., None]
        b1 = ((hm1 * hw) + (cm1 * count)) / tot
        b2 = ((hm2 * hw) + (cm2 * count)) / tot
        empty = count == 0
        out = np.where(found[..., None], np.where(empty[..., None], hcol, blend), color).astype(f32)
        out_n = np.where(found, np.where(empty, hw, tot), count).astype(f32)
        o1 = np.where(found, np.where(empty, hm1, b1), cm1)
        o2 = np.where(found, np.where(empty, hm2, b2), cm2)
        out_m = np.stack([np.where(valid, o1, f32(0)), np.where(valid, o2, f32(0))], axis=-1).astype(f32)
    return (out, out_n, out_m, found) if want_found else (out, out_n, out_m)


def no_history(current, albedo=None):
    """what a moments call without history gives: the current frame and its own moments"""
    color, count = TR.no_history(current)
    cm1, cm2 = current_moments(current[0], current[1], current[2], albedo)
    return color, count, np.stack([cm1, cm2], axis=-1).astype(f32)


def _vp(vp):
    return vp.as_dict() if hasattr(vp, "as_dict") else vp


def raw_variance(moments, count, frame_count, ident, position, normal, vp, want_branch=False):
    """The rule up to the prefilter: raw [H][W]; with want_branch also the masks (none, temporal, spatial)."""
    vp = _vp(vp)
    mom = np.ascontiguousarray(moments, f32); n = np.ascontiguousarray(count, f32); f = np.ascontiguousarray(frame_count, f32)
    ident = np.ascontiguousarray(ident, np.int32)
    pos = np.ascontiguousarray(position, f32); nrm = np.ascontiguousarray(normal, f32)
    H, W = n.shape
    r = int(vp["radius"]); minf = f32(vp["min_frames"]); mpd = f32(vp["max_plane_dist"]); mnd = f32(vp["min_normal_dot"])
    m1 = mom[..., 0]; m2 = mom[..., 1]
    with np.errstate(all="ignore"):
        zz = mpd * mpd
        none = (ident < 0) | ~(n > 0)
        fr = np.where(f > 0, n / f, f32(1.0)).astype(f32)
        v = m2 - (m1 * m1)
        v = np.where(v > 0, v, f32(0))
        temporal = ~none & (fr >= minf)
        rt = v / (fr - f32(1.0))
        s1 = np.zeros((H, W), f32); s2 = np.zeros((H, W), f32); k = np.zeros((H, W), f32)
        ys = np.arange(H)[:, None]; xs = np.arange(W)[None, :]
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                qy = ys + dy; qx = xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                cy = np.clip(qy, 0, H - 1) + 0 * xs; cx = np.clip(qx, 0, W - 1) + 0 * ys
                if dy == 0 and dx == 0:
                    take = np.ones((H, W), bool)
                else:
                    z = _dot(nrm, pos[cy, cx] - pos)
                    cn = _dot(nrm, nrm[cy, cx])
                    take = inside & (ident[cy, cx] == ident) & (n[cy, cx] > 0) & ((z * z) <= zz) & (cn >= mnd)
                s1 = np.where(take, s1 + m1[cy, cx], s1)
                s2 = np.where(take, s2 + m2[cy, cx], s2)
                k = np.where(take, k + f32(1.0), k)
        a1 = s1 / k; a2 = s2 / k
        vs = a2 - (a1 * a1)
        vs = np.where(vs > 0, vs, f32(0))
        rs = vs / fr
        raw = np.where(none, f32(0), np.where(temporal, rt, rs)).astype(f32)
    return (raw, (none, temporal, ~none & ~temporal)) if want_branch else raw


def prefilter(raw, count, ident):
    """the 3x3 pass over the raw plane"""
    raw = np.ascontiguousarray(raw, f32); n = np.ascontiguousarray(count, f32); ident = np.ascontiguousarray(ident, np.int32)
    H, W = raw.shape
    g = (f32(0.25), f32(0.5), f32(0.25))
    tap = (ident >= 0) & (n > 0)
    ys = np.arange(H)[:, None]; xs = np.arange(W)[None, :]
    with np.errstate(all="ignore"):
        sv = np.zeros((H, W), f32); sw = np.zeros((H, W), f32)
        for j in range(3):
            for i in range(3):
                qy = ys + (j - 1); qx = xs + (i - 1)
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                cy = np.clip(qy, 0, H - 1) + 0 * xs; cx = np.clip(qx, 0, W - 1) + 0 * ys
                take = inside & tap[cy, cx]
                w = g[j] * g[i]
                sv = np.where(take, sv + (w * raw[cy, cx]), sv)
                sw = np.where(take, sw + w, sw)
        return np.where(tap, sv / sw, f32(0)).astype(f32)


def variance(moments, count, frame_count, ident, position, normal, vp):
    """ptk_variance_planes"""
    raw = raw_variance(moments, count, frame_count, ident, position, normal, vp)
    return prefilter(raw, count, ident) if int(_vp(vp)["prefilter"]) else raw


def denoise_mask(count, triangle, emission):
    """ptk_denoise_temporal's mask"""
    ok = (np.asarray(count, f32) > 0) & (np.asarray(triangle) >= 0) & (np.asarray(emission, f32) == 0).all(axis=-1)
    return np.where(ok, 0, -1).astype(np.int32)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def moments_case(W, H, seed, degrees=3.0):
    """temporal_rule.random_case with what the moments entries take beside it: the history's moments (NaN on its invalid pixels) and
    an albedo plane (1e30 on the current frame's invalid pixels)"""
    case = TR.random_case(W, H, seed, degrees=degrees)
    rng = np.random.default_rng(seed + 1000)
    hident = case["history"][2]; ident = case["current"][2]
    m1 = rng.uniform(0.2, 1.5, (H, W)).astype(f32)
    hm = np.stack([m1, (m1 * m1) + rng.uniform(0.0, 0.3, (H, W)).astype(f32)], axis=-1).astype(f32)
    hm[hident < 0] = np.nan
    albedo = TR.ALBEDO[np.maximum(ident, 0)].copy()
    albedo[rng.random((H, W)) < 0.02] = 0                       # (a black surface: the epsilon alone divides)
    albedo[ident < 0] = f32(1e30)
    case.update(hist_moments=hm, albedo=albedo.astype(f32))
    return case


def variance_case(W, H, seed):
    """Planes for ptk_variance_planes over the analytic scene: (moments, count, frame_count, id, position, normal).  Histories of 1,
    2, 3, 5, 8 and 16 frames side by side, so that min_frames = 4 sends about half the pixels each way; about 4 % of the pixels have
    no samples at all, 4 % none in the current frame, 3 % NaN moments; invalid pixels hold NaN moments and positions and counts of
    1e30."""
    rng = np.random.default_rng(seed)
    view = TR.view_of(TR.orbit_camera(10.0), W, H)
    ident, pos, nrm = TR.trace_analytic(view, W, H)
    f = rng.choice(np.array([1, 2, 4], f32), (H, W))
    n = (f * rng.choice(np.array([1, 2, 3, 5, 8, 16], f32), (H, W))).astype(f32)
    n[rng.random((H, W)) < 0.04] = 0
    f[rng.random((H, W)) < 0.04] = 0
    m1 = (f32(0.8) + rng.normal(0, 0.1, (H, W))).astype(f32)
    m2 = ((m1 * m1) + rng.uniform(-0.01, 0.2, (H, W)).astype(f32)).astype(f32)
    mom = np.stack([m1, m2], axis=-1)
    mom[rng.random((H, W)) < 0.03] = np.nan
    inv = ident < 0
    mom[inv] = np.nan; n[inv] = f32(1e30); f[inv] = f32(1e30); pos[inv] = np.nan
    return mom.astype(f32), n, f.astype(f32), ident, pos, nrm
