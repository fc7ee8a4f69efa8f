"""numpy float32 mirror of the a-trous denoiser (include/ptk.h ptk_denoise_planes, ptk_denoise_frame) - a helper, no tests of its
own.  Written from the header text: vectorised over pixels, sequential over the 25 taps in the stated order (rows outer, columns
inner), every intermediate a float32 array, one numpy operation per stated operation.

Layout: every plane as it is stored, [H][W] or [H][W][3]; the rule never flips, so bottom-up planes of a frame go in as they are."""
import numpy as np

f32 = np.float32
H5 = (f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625))
CENTRE = f32(0.140625)
ALBEDO_EPS = f32(0.00390625)
DEN_EPS = f32(1e-10)
LR, LG, LB = f32(0.2126), f32(0.7152), f32(0.0722)
PTK_DENOISE_VARIANCE = 1


def params(iterations=5, normal_squarings=5, sigma_z=1.0, sigma_l=4.0):
    return dict(iterations=int(iterations), normal_squarings=int(normal_squarings), sigma_z=float(sigma_z), sigma_l=float(sigma_l))


def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def _lum(c):
    return ((LR * c[..., 0]) + (LG * c[..., 1])) + (LB * c[..., 2])


def denoise(color, mask, normal, position, albedo, variance, p):
    """The planes rule.  color, normal, position, albedo (or None): [H][W][3] float32; mask [H][W] int32 (valid iff >= 0);
    variance (or None): [H][W] float32.  Returns (out_color [H][W][3], out_variance [H][W] or None)."""
    p = p.as_dict() if hasattr(p, "as_dict") else p           # (ptk.DenoiseParams)
    color = np.ascontiguousarray(color, f32); normal = np.ascontiguousarray(normal, f32)
    position = np.ascontiguousarray(position, f32)
    H, W = color.shape[:2]
    valid = np.asarray(mask) >= 0
    have_var = variance is not None
    sigma_z, sigma_l = f32(p["sigma_z"]), f32(p["sigma_l"])
    with np.errstate(all="ignore"):
        c = color.copy()
        if albedo is not None:
            A = np.ascontiguousarray(albedo, f32) + ALBEDO_EPS
            c = np.where(valid[..., None], color / A, color).astype(f32)
        var = np.ascontiguousarray(variance, f32).copy() if have_var else None
        inv_z = f32(1.0) / sigma_z
        for k in range(p["iterations"]):
            s = 1 << k
            if have_var:
                den = ((sigma_l * sigma_l) * var) + DEN_EPS
            else:
                sk = sigma_l * f32(1.0 / s)
                den = np.full((H, W), sk * sk, f32)
            iden = (f32(1.0) / den).astype(f32)
            lum = _lum(c)
            sc = np.zeros((H, W, 3), f32); sw = np.zeros((H, W), f32); sv = np.zeros((H, W), f32)
            for j in range(5):
                dy = (j - 2) * s
                if abs(dy) >= H:
                    continue
                for i in range(5):
                    dx = (i - 2) * s
                    if abs(dx) >= W:
                        continue
                    # the pixels p whose tap q = p + (dx, dy) lies on the image, and those taps
                    P = (slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx)))
                    Q = (slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx)))
                    if dx == 0 and dy == 0:
                        w = np.full((H, W), CENTRE, f32)
                    else:
                        cn = _dot(normal[P], normal[Q])
                        cn = np.where(cn > 0, cn, f32(0)).astype(f32)
                        for _ in range(p["normal_squarings"]):
                            cn = cn * cn
                        d = position[Q] - position[P]
                        z = _dot(normal[P], d) * inv_z
                        a = f32(1.0) + (z * z)
                        dl = lum[P] - lum[Q]
                        b = f32(1.0) + ((dl * dl) * iden[P])
                        w = ((H5[j] * H5[i]) * cn) / (a * b)
                    take = valid[P] & valid[Q] & (w > 0)
                    sc[P] = np.where(take[..., None], sc[P] + (w[..., None] * c[Q]), sc[P])
                    sw[P] = np.where(take, sw[P] + w, sw[P])
                    if have_var:
                        sv[P] = np.where(take, sv[P] + ((w * w) * var[Q]), sv[P])
            c = np.where(valid[..., None], sc / sw[..., None], c).astype(f32)
            if have_var:
                var = np.where(valid, sv / (sw * sw), var).astype(f32)
        out = c
        if albedo is not None:
            out = np.where(valid[..., None], c * A, c).astype(f32)
        # invalid pixels: the input bits (they were copied through every iteration)
        out = np.where(valid[..., None], out, color)
    return out, var


def frame_inputs(S1, n, triangle, emission, albedo, S2=None):
    """What ptk_denoise_frame feeds the rule: (color, mask, variance or None) from the accumulator S1 [H][W][3], the per-pixel
    counts n [H][W] (ptk_samples on owned pixels of a plain render, 0 on the others) and the feature planes, all as stored.
    S2 given: the PTK_DENOISE_VARIANCE arithmetic."""
    S1 = np.ascontiguousarray(S1, f32)
    n = np.asarray(n).astype(np.int64)
    with np.errstate(all="ignore"):
        nf = n.astype(f32)
        m = S1 / nf[..., None]
        color = np.where((n > 0)[..., None], m, f32(0)).astype(f32)
        valid = (n > 0) & (np.asarray(triangle) >= 0) & (np.asarray(emission) == 0).all(axis=-1)
        var = None
        if S2 is not None:
            valid &= n >= 2
            A = np.ascontiguousarray(albedo, f32) + ALBEDO_EPS
            v = np.ascontiguousarray(S2, f32) / nf[..., None] - m * m
            v = np.where(v < 0, f32(0), v).astype(f32)
            q = v / (A * A)
            var = ((q[..., 0] + q[..., 1]) + q[..., 2]) / (f32(3.0) * (nf - f32(1.0)))
            var = np.where(valid, var, f32(0)).astype(f32)
    return color, np.where(valid, 0, -1).astype(np.int32), var


def resolve_rgb8(x):
    """The 8-bit resolve of the frame (pathtracer.cpp:802-812) applied to a float image."""
    x = np.asarray(x, f32)
    x = np.where(x < 0, f32(0), np.where(x > 1, f32(1), x))
    x = np.where(np.isnan(x), f32(0), x).astype(f32)
    return (x * f32(255)).astype(np.uint8)
