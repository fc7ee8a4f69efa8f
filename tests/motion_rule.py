"""numpy float32 mirror of temporal reprojection over moving geometry (include/ptk.h ptk_geometry_snapshot, ptk_render_motion,
ptk_reproject_planes_moving, ptk_temporal_frame_moving) - a helper, no tests of its own.  Written from the header text: vectorised
over pixels, every intermediate a float32 array, one numpy operation per stated operation.  The projection, the taps and the blend
are tests/temporal_rule.py's: reproject_moving below repeats its reproject with the header's one substitution, and nothing in
temporal_rule is changed.

Layout: planes [H][W] or [H][W][c], rows BOTTOM-UP; vertex tables [num_tris][9] float32."""
import numpy as np

import temporal_rule as TR

f32 = np.float32


def _cross(a, b):
    return np.stack([(a[..., 1] * b[..., 2]) - (a[..., 2] * b[..., 1]), (a[..., 2] * b[..., 0]) - (a[..., 0] * b[..., 2]),
                     (a[..., 0] * b[..., 1]) - (a[..., 1] * b[..., 0])], axis=-1)


_dot = TR._dot


def previous(tri, bary, position, normal, verts, prev_verts=None, want_cases=False):
    """X' and n' of every pixel: (prev_position [H][W][3], prev_normal [H][W][3]) and, with want_cases, the masks (miss, unmoved,
    moved).  prev_verts None: no snapshot, every triangle is unmoved."""
    tri = np.ascontiguousarray(tri, np.int32)
    bary = np.ascontiguousarray(bary, f32); X = np.ascontiguousarray(position, f32); n = np.ascontiguousarray(normal, f32)
    verts = np.ascontiguousarray(verts, f32).reshape(-1, 9)
    prev = verts if prev_verts is None else np.ascontiguousarray(prev_verts, f32).reshape(-1, 9)
    assert prev.shape == verts.shape
    num = len(verts)
    named = (tri >= 0) & (tri < num)
    k = np.where(named, tri, 0)
    with np.errstate(all="ignore"):
        if num:
            c = verts[k]; p = prev[k]
        else:
            c = p = np.zeros(tri.shape + (9,), f32)
        moved = named & ~(c == p).all(axis=-1)
        u = bary[..., 0]; v = bary[..., 1]
        w = (f32(1.0) - u) - v
        v0, v1, v2 = c[..., 0:3], c[..., 3:6], c[..., 6:9]
        q0, q1, q2 = p[..., 0:3], p[..., 3:6], p[..., 6:9]
        D = (((q0 - v0) * w[..., None]) + ((q1 - v1) * u[..., None])) + ((q2 - v2) * v[..., None])
        Xp = X + D
        e1 = v1 - v0; e2 = v2 - v0; N = _cross(e1, e2)
        f1 = q1 - q0; f2 = q2 - q0; M = _cross(f1, f2)
        a = _dot(n, e1); b = _dot(n, e2); cc = _dot(n, N)
        A = _cross(f2, M); B = _cross(M, f1); nn = _dot(M, M)
        npr = (((a[..., None] * A) + (b[..., None] * B)) + (cc[..., None] * M)) / nn[..., None]
    Xp = np.where(moved[..., None], Xp, X).astype(f32)
    npr = np.where(moved[..., None], npr, n).astype(f32)
    if want_cases:
        return Xp, npr, (tri < 0, (tri >= 0) & ~moved, moved)
    return Xp, npr


def motion(view, tri, prev_position):
    """The motion plane [H][W][2] of X' under `view` (None: NaN everywhere): (col - j, row - i) for column j and top-down row i where
    the pixel hit something and s > 0, else NaN."""
    tri = np.ascontiguousarray(tri, np.int32)
    H, W = tri.shape
    out = np.full((H, W, 2), np.nan, f32)
    if view is None:
        return out
    with np.errstate(all="ignore"):
        col, row, s = TR.project(view, prev_position)
        j = np.arange(W, dtype=np.int32)[None, :].astype(f32)
        i = (H - 1 - np.arange(H, dtype=np.int32))[:, None].astype(f32)
        ok = (tri >= 0) & (s > 0)
        out[..., 0] = np.where(ok, col - j, f32(np.nan))
        out[..., 1] = np.where(ok, row - i, f32(np.nan))
    return out


def render_motion(view, planes, verts, prev_verts=None):
    """ptk_render_motion: planes = (tri, bary, position, normal).  Returns (prev_position, prev_normal, motion)."""
    tri, bary, position, normal = planes
    Xp, npr = previous(tri, bary, position, normal, verts, prev_verts)
    return Xp, npr, motion(view, tri, Xp)


def reproject_moving(view, current, prev_position, prev_normal, history, p, want_found=False):
    """ptk_reproject_planes_moving: temporal_rule.reproject with X' and n' wherever the rule speaks of the history's geometry."""
    p = p.as_dict() if hasattr(p, "as_dict") else p
    color, count = (np.ascontiguousarray(current[k], f32) for k in (0, 1))
    ident = np.ascontiguousarray(current[2], np.int32)
    Xp = np.ascontiguousarray(prev_position, f32); npr = np.ascontiguousarray(prev_normal, f32)
    hcolor, hcount, hposition, hnormal = (np.ascontiguousarray(history[k], f32) for k in (0, 1, 3, 4))
    hident = np.ascontiguousarray(history[2], np.int32)
    H, W = count.shape
    mpd = f32(p["max_plane_dist"]); mnd = f32(p["min_normal_dot"]); maxh = f32(p["max_history"]); match = bool(p["match_id"])
    with np.errstate(all="ignore"):
        zz = mpd * mpd
        col, row, s = TR.project(view, Xp)
        valid = ident >= 0
        ok = valid & (s > 0) & (col > f32(-1)) & (col < f32(W)) & (row > f32(-1)) & (row < f32(H))
        col = np.where(ok, col, f32(0)); row = np.where(ok, row, f32(0))
        x0 = np.floor(col).astype(np.int32); fx = col - x0.astype(f32)
        i0 = np.floor(row).astype(np.int32); fy = row - i0.astype(f32)
        gx = f32(1.0) - fx; gy = f32(1.0) - fy
        b4 = (gx * gy, fx * gy, gx * fy, fx * fy)
        sc = np.zeros((H, W, 3), f32); sn = np.zeros((H, W), f32); sw = np.zeros((H, W), f32)
        for k in range(4):
            qx = x0 + (k & 1); qi = i0 + (k >> 1)
            inside = ok & (qx >= 0) & (qx < W) & (qi >= 0) & (qi < H)
            cx = np.clip(qx, 0, W - 1); cy = np.clip(H - 1 - qi, 0, H - 1)
            hc = hcolor[cy, cx]; hn = hcount[cy, cx]; hi = hident[cy, cx]; hp = hposition[cy, cx]; hm = hnormal[cy, cx]
            b = b4[k]
            z = _dot(npr, hp - Xp)
            cn = _dot(npr, hm)
            take = inside & (hi >= 0) & (hn > 0) & (b > 0) & ((z * z) <= zz) & (cn >= mnd)
            if match:
                take &= hi == ident
            sc = np.where(take[..., None], sc + (b[..., None] * hc), sc)
            sn = np.where(take, sn + (b * hn), sn)
            sw = np.where(take, sw + b, sw)
        found = ok & (sw > 0)
        hcol = sc / sw[..., None]
        hw = sn / sw
        hw = np.where(hw > maxh, maxh, hw)
        tot = hw + count
        blend = ((hcol * hw[..., None]) + (color * count[..., None])) / tot[..., None]
        empty = count == 0
        out = np.where(found[..., None], np.where(empty[..., None], hcol, blend), color).astype(f32)
        out_n = np.where(found, np.where(empty, hw, tot), count).astype(f32)
    return (out, out_n, found) if want_found else (out, out_n)
