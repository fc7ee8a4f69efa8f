"""numpy float32 mirror of guided upsampling (include/ptk.h ptk_upsample_planes, ptk_upsample_frame) - a helper, no tests of its own.
Written from the header text: vectorised over the high pixels, sequential over the taps in the stated order, every intermediate a
float32 array or scalar, one numpy operation per stated operation.

Layout: every plane as it is stored, [H][W] or [H][W][3], rows BOTTOM-UP: plane row y is top-down row i = H-1-y.
lo = (color [h][w][3] f32, id [h][w] i32, position [h][w][3] f32, normal [h][w][3] f32, albedo [h][w][3] f32 or None);
hi = (id [H][W] i32, position, normal, albedo or None)."""
import numpy as np

from display_rule import accum_color                                       # PTK_UPSAMPLE_ACCUM's colour is PTK_DISPLAY_ACCUM's

f32 = np.float32
ALBEDO_EPS = f32(0.00390625)
UPSAMPLE_ACCUM, UPSAMPLE_DENOISED, UPSAMPLE_TEMPORAL = 0, 1, 2


def params(max_plane_dist, min_normal_dot=0.9, wide=1):
    return dict(max_plane_dist=float(max_plane_dist), min_normal_dot=float(min_normal_dot), wide=int(wide))


def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def upsample(lo, hi, p, want_reasons=False):
    """The planes rule.  Returns (out_color [H][W][3] f32, out_class [H][W] i32) and, with want_reasons, a dict of counts: how many
    ring-0 taps were dropped for each reason (outside, id, plane, normal, weight), how many ring-1 taps were taken and how many
    of those came from a clamped (off-image) neighbourhood."""
    p = p.as_dict() if hasattr(p, "as_dict") else p                        # (ptk.UpsampleParams)
    color, position, normal = (np.ascontiguousarray(lo[k], f32) for k in (0, 2, 3))
    ident = np.ascontiguousarray(lo[1], np.int32)
    albedo = None if lo[4] is None else np.ascontiguousarray(lo[4], f32)
    hid = np.ascontiguousarray(hi[0], np.int32)
    hpos, hnrm = (np.ascontiguousarray(hi[k], f32) for k in (1, 2))
    halb = None if hi[3] is None else np.ascontiguousarray(hi[3], f32)
    assert (albedo is None) == (halb is None), "the two albedo planes go together"
    h, w = ident.shape
    H, W = hid.shape
    mpd = f32(p["max_plane_dist"]); mnd = f32(p["min_normal_dot"]); wide = bool(p["wide"])
    reasons = dict(outside=0, id=0, plane=0, normal=0, weight=0, ring1_taken=0, ring1_pixels_at_corner=0)
    with np.errstate(all="ignore"):
        sx = f32(w) / f32(W); sy = f32(h) / f32(H)
        zz = mpd * mpd
        x = np.broadcast_to(np.arange(W, dtype=np.int32)[None, :], (H, W))
        i = np.broadcast_to((H - 1 - np.arange(H, dtype=np.int32))[:, None], (H, W))      # top-down row of plane row y
        col = ((x.astype(f32) + f32(0.5)) * sx) - f32(0.5)
        row = ((i.astype(f32) + f32(0.5)) * sy) - f32(0.5)
        x0 = np.floor(col).astype(np.int32); fx = col - x0.astype(f32)
        i0 = np.floor(row).astype(np.int32); fy = row - i0.astype(f32)
        gx = f32(1.0) - fx; gy = f32(1.0) - fy
        pvalid = hid >= 0

        def tap(tx, ti, b, live, sc, sw, count=False):
            inside = (tx >= 0) & (tx < w) & (ti >= 0) & (ti < h)
            cx = np.clip(tx, 0, w - 1); cy = h - 1 - np.clip(ti, 0, h - 1)
            qc = color[cy, cx]; qi = ident[cy, cx]; qp = position[cy, cx]; qn = normal[cy, cx]
            z = _dot(hnrm, qp - hpos)
            cn = _dot(hnrm, qn)
            same = qi == hid
            plane = (z * z) <= zz
            facing = cn >= mnd
            ok = np.where(pvalid, same & plane & facing, qi < 0)
            take = live & inside & ok & (b > 0)
            if count:
                reasons["outside"] += int((live & ~inside).sum())
                reasons["weight"] += int((live & inside & ~(b > 0)).sum())
                reasons["id"] += int((live & inside & (b > 0) & np.where(pvalid, ~same, qi >= 0)).sum())
                reasons["plane"] += int((live & inside & (b > 0) & pvalid & same & ~plane).sum())
                reasons["normal"] += int((live & inside & (b > 0) & pvalid & same & plane & ~facing).sum())
            v = qc
            if albedo is not None:
                v = np.where((qi >= 0)[..., None], qc / (albedo[cy, cx] + ALBEDO_EPS), qc)
            sc = np.where(take[..., None], sc + (b[..., None] * v), sc)
            sw = np.where(take, sw + b, sw)
            return sc, sw, take

        everywhere = np.ones((H, W), bool)
        sc = np.zeros((H, W, 3), f32); sw = np.zeros((H, W), f32)
        b4 = (gx * gy, fx * gy, gx * fy, fx * fy)
        for k in range(4):
            sc, sw, _ = tap(x0 + (k & 1), i0 + (k >> 1), b4[k], everywhere, sc, sw, count=True)
        class0 = sw > 0
        r = sc / sw[..., None]
        cls = np.where(class0, 0, 2).astype(np.int32)
        if wide:
            need = ~class0
            sc1 = np.zeros((H, W, 3), f32); sw1 = np.zeros((H, W), f32)
            for j in range(4):
                for k in range(4):
                    if j in (1, 2) and k in (1, 2):
                        continue
                    tx = x0 - 1 + k; ti = i0 - 1 + j
                    dx = tx.astype(f32) - col; dy = ti.astype(f32) - row
                    b = f32(1.0) / (f32(1.0) + ((dx * dx) + (dy * dy)))
                    sc1, sw1, take = tap(tx, ti, b, need, sc1, sw1)
                    reasons["ring1_taken"] += int(take.sum())
            class1 = need & (sw1 > 0)
            r = np.where(class1[..., None], sc1 / sw1[..., None], r)
            cls = np.where(class1, 1, cls).astype(np.int32)
            corner = ((x0 - 1 < 0) | (x0 + 2 > w - 1)) & ((i0 - 1 < 0) | (i0 + 2 > h - 1))
            reasons["ring1_pixels_at_corner"] = int((class1 & corner).sum())
        out = r
        if halb is not None:
            out = np.where(pvalid[..., None], r * (halb + ALBEDO_EPS), r)
        xn = np.clip(np.floor(col + f32(0.5)).astype(np.int32), 0, w - 1)
        yn = np.clip(np.floor(row + f32(0.5)).astype(np.int32), 0, h - 1)
        hole = color[h - 1 - yn, xn]
        out = np.where((cls == 2)[..., None], hole, out).astype(f32)
    return (out, cls, reasons) if want_reasons else (out, cls)


def frame_inputs(source, s1=None, counts=None, denoised=None, temporal=None):
    """The colour ptk_upsample_frame takes for `source`, exactly as ptk_display_frame takes it: S1 / n_p (display_rule.accum_color),
    the denoised plane, or the temporal colour."""
    if source == UPSAMPLE_ACCUM:
        return accum_color(s1, counts)
    return np.ascontiguousarray(denoised if source == UPSAMPLE_DENOISED else temporal, f32)

