"""Guided upsampling, the worked use (include/ptk.h ptk_render_guides, ptk_upsample_frame): trace a frame at a low
resolution, bring it up to the full one, and spend a few rays on the pixels the upsampler could not serve.

    w, h = low_resolution(W, H, 2.0)                 # a low frame of the output's aspect ratio
    ctx.set_frame(w, h, depth); ctx.render(0, spp, seed)
    ctx.render_features(ptk.UPSAMPLE_GUIDES); ctx.render_guides(W, H)
    ctx.upsample_frame(ptk.UPSAMPLE_ACCUM, ptk.upsample_defaults(extent))
    color, cls = ctx.read_upsampled()
    color, info = fill_holes(ctx, color, cls, ctx.guide_view(), 16, depth)
"""
from __future__ import annotations

import math

import numpy as np

CLASS_BILINEAR, CLASS_WIDE, CLASS_HOLE = 0, 1, 2


def low_resolution(W: int, H: int, scale: float):
    """The frame to trace for an output of W x H shown at `scale` times the traced resolution: the size nearest to
    round(W / scale) x round(H / scale) that has exactly the output's aspect ratio (W*h == H*w, which ptk_upsample_frame asks for:
    the pixel-centre mapping is the camera's only then).  ValueError when there is none, with the scales that work."""
    if not (W > 0 and H > 0 and scale >= 1.0 and math.isfinite(scale)):
        raise ValueError("the output needs a positive size and --upscale a finite scale >= 1")
    g = math.gcd(W, H)
    aw, ah = W // g, H // g
    k = int(round(g / scale))
    if k < 1:
        raise ValueError(f"{W}x{H} has the aspect ratio {aw}:{ah}: no smaller frame than {aw}x{ah} (scale {g}) shares it, and "
                         f"scale {scale:g} asks for less; choose an output whose width and height have a larger common divisor")
    return k * aw, k * ah


def class_shares(cls, valid=None):
    """the shares of the three classes (bilinear, wide ring, hole) over the pixels of `valid`, or all"""
    c = np.asarray(cls)
    c = c[valid] if valid is not None else c.reshape(-1)
    n = max(1, c.size)
    return [float((c == k).sum()) / n for k in range(3)]


def hole_rays(cls, view):
    """The camera rays of the class-2 pixels of an upsampled frame under `view` (ptk.View or a dict of its fields, the guide
    planes' own: Context.guide_view): dict(rows, cols - plane indices, rows bottom-up -, origins, dirs [n, 3] float32).  The ray of
    column j, top-down row i goes from view.pos through top_left + right*(delta_x*j) - up*(delta_y*i), the image point the view
    defines; the direction is normalised in float64 and cast."""
    v = view.as_dict() if hasattr(view, "as_dict") else view
    cls = np.asarray(cls)
    H = cls.shape[0]
    rows, cols = np.nonzero(cls == CLASS_HOLE)
    pos, right, up, tl = (np.asarray(v[k], np.float64) for k in ("pos", "right", "up", "top_left"))
    i = (H - 1 - rows).astype(np.float64)
    pt = tl + right * (float(v["delta_x"]) * cols.astype(np.float64))[:, None] - up * (float(v["delta_y"]) * i)[:, None]
    d = pt - pos
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    origins = np.ascontiguousarray(np.broadcast_to(pos, d.shape), np.float32)
    return dict(rows=rows, cols=cols, origins=origins, dirs=np.ascontiguousarray(d, np.float32))


def fill_holes(ctx, color, cls, view, spp: int, max_depth: int, seed: int = 0, first_sample: int = 0, key_base: int = 0):
    """Traces the class-2 pixels of an upsampled frame - the ones no low-resolution sample of the same surface could serve - with
    Context.trace_rays along their camera rays (hole_rays) and writes sum / spp into exactly those pixels of a copy of `color`.
    Returns (color, info): info is hole_rays' dict plus `sums`, what trace_rays returned, and the call's spp, seed, first_sample
    and key_base.  The rays go through pixel corners' image points with the lens closed, on the RNG streams of (seed, key_base +
    k, sample) for the k-th hole: they are fresh samples of the same radiance, NOT the samples a full-resolution ptk_render would
    have drawn for those pixels - nothing here is bit-pinned to a frame."""
    out = np.array(color, np.float32, copy=True)
    info = hole_rays(cls, view)
    info.update(spp=int(spp), seed=int(seed), first_sample=int(first_sample), key_base=int(key_base))
    n = len(info["rows"])
    if n == 0 or spp <= 0:
        info["sums"] = np.zeros((n, 3), np.float32)
        return out, info
    sums = ctx.trace_rays(info["origins"], info["dirs"], int(max_depth), int(first_sample), int(spp), int(seed), key_base=int(key_base))
    info["sums"] = sums
    out[info["rows"], info["cols"]] = sums / np.float32(spp)
    return out, info
