"""numpy float32 mirror of temporal reprojection (include/ptk.h ptk_get_view, ptk_reproject_planes, ptk_temporal_frame) - a helper, no
tests of its own.  Written from the header text: vectorised over pixels, sequential over the four taps in the stated order, every
intermediate a float32 array or scalar, one numpy operation per stated operation.

Layout: every plane as it is stored, [H][W] or [H][W][3], rows BOTTOM-UP: plane row y is top-down row i = H-1-y.
A view is a dict of float32: pos, right, up, top_left [3] and delta_x, delta_y (ptk.View.as_dict gives the same)."""
import math

import numpy as np

f32 = np.float32
PTK_TEMPORAL_RESET = 1


def params(max_plane_dist, min_normal_dot=0.9, max_history=64.0, match_id=1):
    return dict(max_plane_dist=float(max_plane_dist), min_normal_dot=float(min_normal_dot), max_history=float(max_history), match_id=int(match_id))


def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def _cross(a, b):
    return np.array([(a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0])], f32)


def _normalize(v):
    """the camera setter's normalisation: x * (1 / sqrt(dot(x, x)))"""
    v = np.asarray(v, f32)
    sqr = ((v[0] * v[0]) + (v[1] * v[1])) + (v[2] * v[2])
    inv = f32(1.0) / np.sqrt(sqr)
    return (v * inv).astype(f32)


def view_of(cam, W, H):
    """The image-plane set-up of the render for the camera `cam` (pos, dir, up, focal, fovy as ptk_set_camera takes them) at W x H:
    the setter's clamps and normalisations, then the frame set-up's float32 arithmetic; tan in double by libm, as the host takes it."""
    pos = np.asarray(cam["pos"], f32)
    dir_ = _normalize(cam["dir"]); up = _normalize(cam["up"])
    focal = f32(cam["focal"]); fovy = f32(cam["fovy"])
    if focal <= 0:
        focal = f32(0.1)
    if fovy <= 0:
        fovy = f32(0.1)
    elif fovy >= 180:
        fovy = f32(179.5)
    center = pos + (dir_ * focal)
    img_h = f32(float(f32(2.0) * focal) * math.tan(float(fovy / f32(2.0)) * 3.14159265358979323846 / 180.0))
    aspect = f32(W) / f32(H)
    img_w = img_h * aspect
    delta_x = img_w / f32(W)
    delta_y = img_h / f32(H)
    right = _normalize(np.array([(up[1] * dir_[2]) - (dir_[1] * up[2]), (up[2] * dir_[0]) - (dir_[2] * up[0]), (up[0] * dir_[1]) - (dir_[0] * up[1])], f32))
    hw = img_w * f32(0.5); hh = img_h * f32(0.5)
    tl = center - (right * hw)
    tl = tl + (up * hh)
    return dict(pos=pos, right=right, up=up, top_left=tl.astype(f32), delta_x=f32(delta_x), delta_y=f32(delta_y))


def _view(view):
    view = view.as_dict() if hasattr(view, "as_dict") else view            # (ptk.View)
    v = {k: np.asarray(view[k], f32) for k in ("pos", "right", "up", "top_left")}
    v["delta_x"] = f32(view["delta_x"]); v["delta_y"] = f32(view["delta_y"])
    return v


def project(view, X):
    """The rule's projection of the points X [..., 3] into `view`: (col, row, s), float32."""
    v = _view(view)
    X = np.asarray(X, f32)
    with np.errstate(all="ignore"):
        nrm = _cross(v["right"], v["up"])
        e = v["top_left"] - v["pos"]
        num = _dot(e, nrm)
        d = X - v["pos"]
        den = _dot(d, nrm)
        s = num / den
        Q = (d * s[..., None]) - e
        col = _dot(Q, v["right"]) / v["delta_x"]
        row = (f32(0) - _dot(Q, v["up"])) / v["delta_y"]
    return col, row, s


def reproject(view, current, history, p, want_found=False):
    """The planes rule.  current and history: (color [H][W][3] f32, count [H][W] f32, id [H][W] i32, position [H][W][3] f32, normal
    [H][W][3] f32); view: the history's.  Returns (out_color, out_count) and, with want_found, the pixels that found history."""
    p = p.as_dict() if hasattr(p, "as_dict") else p                        # (ptk.TemporalParams)
    color, count, position, normal = (np.ascontiguousarray(current[k], f32) for k in (0, 1, 3, 4))
    ident = np.ascontiguousarray(current[2], np.int32)
    hcolor, hcount, hposition, hnormal = (np.ascontiguousarray(history[k], f32) for k in (0, 1, 3, 4))
    hident = np.ascontiguousarray(history[2], np.int32)
    H, W = count.shape
    mpd = f32(p["max_plane_dist"]); mnd = f32(p["min_normal_dot"]); maxh = f32(p["max_history"]); match = bool(p["match_id"])
    with np.errstate(all="ignore"):
        zz = mpd * mpd
        col, row, s = project(view, position)
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
            z = _dot(normal, hp - position)
            cn = _dot(normal, hm)
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


def no_history(current):
    """what a call without history gives: the current frame"""
    return np.ascontiguousarray(current[0], f32).copy(), np.ascontiguousarray(current[1], f32).copy()


def frame_inputs(S1, n):
    """What ptk_temporal_frame takes from the accumulator: (color, count) from S1 [H][W][3] and the per-pixel counts n [H][W]
    (ptk_samples on owned pixels of a plain render, 0 on the others)."""
    S1 = np.ascontiguousarray(S1, f32)
    n = np.asarray(n).astype(np.int64)
    with np.errstate(all="ignore"):
        nf = n.astype(f32)
        color = np.where((n > 0)[..., None], S1 / nf[..., None], f32(0)).astype(f32)
    return color, nf


# ---- an analytic scene under two cameras ------------------------------------------------------------------------------------------
# The inside of the box [-1, 1]^3 with a sphere in it, seen from a camera inside that circles the sphere: the sphere disoccludes
# wall behind it when the camera moves, wall enters over the image's edges, ids change along every edge of the box, and a window
# in the wall z = -1 holds nothing (invalid pixels).
SPHERE_C = np.array([0.1, -0.15, 0.0]); SPHERE_R = 0.3
WINDOW = (0.2, 0.8, 0.0, 0.55)                  # x0, x1, y0, y1 on the wall z = -1
EXTENT = float(np.linalg.norm([2.0, 2.0, 2.0]))


def orbit_camera(degrees, distance=0.85, height=0.2, fovy=60.0):
    """a camera on a circle about the box's centre, `degrees` from the +z axis, looking at the centre"""
    a = math.radians(degrees)
    pos = np.array([distance * math.sin(a), height, distance * math.cos(a)])
    d = -pos / np.linalg.norm(pos)
    r = np.cross([0.0, 1.0, 0.0], d); r /= np.linalg.norm(r)
    up = np.cross(d, r)
    return dict(pos=pos.astype(f32), dir=d.astype(f32), up=up.astype(f32), focal=0.1, fovy=fovy, focal_dist=5.0, aperture=0.0)


def trace_analytic(view, W, H):
    """first hits of the pixels' rays (through the image points of the view) in double: (id [H][W] int32 - 0..5 a wall, 6 the
    sphere, -1 the window -, position, normal), rows bottom-up"""
    v = {k: np.asarray(x, np.float64) for k, x in _view(view).items()}
    j = np.arange(W)[None, :]; i = (H - 1 - np.arange(H))[:, None]
    pt = v["top_left"] + v["right"] * (v["delta_x"] * j)[..., None] - v["up"] * (v["delta_y"] * i)[..., None]
    o = v["pos"]
    d = pt - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        best = np.full((H, W), np.inf); ident = np.full((H, W), -1, np.int32); nrm = np.zeros((H, W, 3))
        walls = [(0, -1.0), (0, 1.0), (1, -1.0), (1, 1.0), (2, -1.0), (2, 1.0)]
        for k, (axis, side) in enumerate(walls):
            t = (side - o[axis]) / d[..., axis]
            hit = (t > 0) & (t < best)
            best = np.where(hit, t, best); ident = np.where(hit, k, ident)
            n = np.zeros(3); n[axis] = -side
            nrm = np.where(hit[..., None], n, nrm)
        q = o + d * best[..., None]
        window = (ident == 4) & (q[..., 0] > WINDOW[0]) & (q[..., 0] < WINDOW[1]) & (q[..., 1] > WINDOW[2]) & (q[..., 1] < WINDOW[3])
        oc = o - SPHERE_C
        bq = (d * oc).sum(-1); cq = (oc * oc).sum() - SPHERE_R ** 2
        disc = bq * bq - cq
        t = -bq - np.sqrt(disc)
        hit = (disc > 0) & (t > 0) & (t < best)
        best = np.where(hit, t, best); ident = np.where(hit, 6, np.where(window, -1, ident))
        q = o + d * best[..., None]
        nrm = np.where(hit[..., None], (q - SPHERE_C) / SPHERE_R, nrm)
        pos = np.where((ident >= 0)[..., None], q, 0.0)
    return ident, pos.astype(f32), nrm.astype(f32)


ALBEDO = np.array([[0.7, 0.2, 0.2], [0.2, 0.7, 0.2], [0.7, 0.7, 0.7], [0.6, 0.6, 0.7], [0.7, 0.7, 0.6], [0.5, 0.5, 0.5], [0.3, 0.4, 0.8]], f32)


def planes_under(cam, W, H, rng, poison=True):
    """(view, five planes) of the analytic scene under `cam`: noisy colours about an albedo per id, counts 0..8 with about 4 % zeros;
    with poison the invalid pixels hold NaN colours, 1e30 counts and NaN positions"""
    view = view_of(cam, W, H)
    ident, pos, nrm = trace_analytic(view, W, H)
    color = (ALBEDO[np.maximum(ident, 0)] * rng.uniform(0.5, 1.5, (H, W, 3))).astype(f32)
    count = rng.integers(1, 9, (H, W)).astype(f32)
    count[rng.random((H, W)) < 0.04] = 0
    inv = ident < 0
    if poison:
        color[inv] = np.nan; count[inv] = 1e30; pos[inv] = np.nan
    return view, (color, count, ident, pos, nrm)


def random_case(W, H, seed, degrees=3.0, start=10.0):
    """History and current planes of the analytic scene under two cameras `degrees` apart on the orbit: dict(view, hist_view, current,
    history, extent)."""
    rng = np.random.default_rng(seed)
    hist_view, history = planes_under(orbit_camera(start), W, H, rng)
    view, current = planes_under(orbit_camera(start + degrees), W, H, rng)
    return dict(view=view, hist_view=hist_view, current=current, history=history, extent=EXTENT)
