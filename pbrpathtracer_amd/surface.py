"""Worked uses of surface sampling (include/ptk.h ptk_sample_surface): weight tables for
Context.set_surface_weights, and a bake at sampled surface points that needs neither vertices nor a uv layout - with the
points' colour, shading normal and emission where asked for (ptk_surface_attributes)."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def material_weights(material_ids, chosen) -> np.ndarray:
    """[triangles] float32: 1 where the triangle's material is `chosen` (an index or several), 0 elsewhere - points on the surfaces
    of those materials only, still in proportion to area"""
    ids = np.asarray(material_ids, np.int32).reshape(-1)
    return np.isin(ids, np.atleast_1d(np.asarray(chosen, np.int32))).astype(F32)


def emissive_weights(materials, material_ids) -> np.ndarray:
    """[triangles] float32: the luminance (Rec. 709) of emissive * emissive_intensity of each triangle's material, in float32.
    Times the area - which the table multiplies on - this samples the lights by power; everything that does not emit gets 0 and is
    never drawn."""
    e = np.asarray(materials["emissive"], F32).reshape(-1, 3) * np.asarray(materials["emissive_intensity"], F32).reshape(-1, 1)
    lum = (e[:, 0] * F32(0.2126) + e[:, 1] * F32(0.7152)) + e[:, 2] * F32(0.0722)
    return np.maximum(lum, F32(0)).astype(F32)[np.asarray(material_ids, np.int32).reshape(-1)]


def transfer(ctx, values_per_triangle, points, k, power=2, max_dist=None) -> np.ndarray:
    """Attribute transfer from the scene's triangles to arbitrary points: [n, ...] float64, the inverse-distance blend of
    values_per_triangle [triangles, ...] over the k nearest triangles of each point (ctx.nearest_triangles, include/ptk.h
    ptk_nearest_triangles; ctx: a Context or a PathTracer) with weights (d_0 / d_j) ** power, d_0 the nearest distance, normalised to
    sum 1.  A point on the surface (d_0 = 0) takes the mean over the triangles it lies on; k = 1 copies the nearest triangle's value;
    a point with no triangle within max_dist gets NaN."""
    values = np.asarray(values_per_triangle, np.float64)
    _, tri, dist = ctx.nearest_triangles(points, k, max_dist)[:3]
    d = dist.astype(np.float64)
    d0 = d[:, :1]
    with np.errstate(all="ignore"):
        w = np.where(d0 > 0, (d0 / d) ** float(power), (d == 0).astype(np.float64))
        w = np.where(tri >= 0, w, 0.0)
        w = w / w.sum(axis=1, keepdims=True)                # (0 / 0 where nothing was found: NaN)
        picked = values[np.maximum(tri, 0)]                 # [n, k, ...]
        w = w.reshape(w.shape + (1,) * (picked.ndim - 2))
        return (picked * w).sum(axis=1)


def bake_rays(position, normal, offset):
    """(origins, dirs) [n, 3] float32 of the lightmap bake's ray at each point: origin = P + n * offset - the product rounded to
    float32, then the sum -, direction = -n"""
    p = np.ascontiguousarray(position, F32).reshape(-1, 3); n = np.ascontiguousarray(normal, F32).reshape(-1, 3)
    lift = n * F32(offset)
    return p + lift, -n


def bake_points(ctx, n, spp, offset, max_depth, seed=0, first_sample=0, key_base=0, out=None, attributes=False):
    """A bake without a uv layout: n surface points (ctx.sample_surface at `seed`, `key_base`, sample 0), each traced with
    ctx.trace_rays along bake_rays - the radiance leaving the surface along its normal, as a lightmap texel gathers it - over samples
    [first_sample, first_sample + spp) with the sampling's key_base, so point j and ray j share RNG pixel key_base + j.  Returns
    (position [n, 3], normal [n, 3] float32, tri [n], material [n] int32, radiance [n, 3] float32: the sum over the samples).  out:
    the radiance of earlier samples of the same points, added to in place - a progressive bake equals one long bake.
    attributes=True: a sixth element, the dict of ctx.surface_attributes (include/ptk.h ptk_surface_attributes) at the points with
    albedo, normal (the shading normal, not flipped) and emission [n, 3] float32 - a coloured point cloud; the five others keep their
    bits."""
    tri, bary, position, normal, material = ctx.sample_surface(n, seed=seed, key_base=key_base, sample=0)
    origins, dirs = bake_rays(position, normal, offset)
    radiance = ctx.trace_rays(origins, dirs, max_depth, first_sample, spp, seed, key_base=key_base, out=out)
    if not attributes:
        return position, normal, tri, material, radiance
    from . import ptk
    at = ctx.surface_attributes(tri, bary, None, 1 << ptk.ATTR_ALBEDO | 1 << ptk.ATTR_NORMAL | 1 << ptk.ATTR_EMISSION)
    return position, normal, tri, material, radiance, at
