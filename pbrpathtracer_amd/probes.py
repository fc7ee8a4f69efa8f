"""Irradiance probe helpers for Context.bake_probes / PathTracer.BakeProbes (include/ptk.h ptk_bake_probes): a direction set, the
positions of a regular grid and the projection weight that goes with a uniform direction set - the worked use that keeps the Python
path honest, as rays.equirect_rays and lightmap.grid_atlas are for theirs."""
from __future__ import annotations

import math

import numpy as np


def fibonacci_dirs(num_dirs: int) -> np.ndarray:
    """[num_dirs, 3] float32 unit directions of the spherical Fibonacci lattice: z_i = 1 - (2 i + 1) / D, azimuth i times the
    golden angle; computed and normalised in float64, then cast.  The lattice is a near-uniform quadrature rule of weight
    4 pi / D per direction (sh_weight)."""
    if num_dirs < 1:
        raise ValueError("fibonacci_dirs: at least one direction")
    i = np.arange(num_dirs, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / num_dirs
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(d, np.float32)


def grid_positions(dims, origin, spacing) -> np.ndarray:
    """[nz * ny * nx, 3] float32 positions of a probe grid in the order ptk_probes_irradiance indexes it ((iz * ny + iy) * nx + ix):
    origin + (float)i * spacing per axis, in float32"""
    nx, ny, nz = (int(n) for n in dims)
    if min(nx, ny, nz) < 1:
        raise ValueError("grid_positions: dims must be at least 1")
    o = np.asarray(origin, np.float32).reshape(3)
    s = np.asarray(spacing, np.float32).reshape(3)
    ax = [o[a] + np.arange(n, dtype=np.float32) * s[a] for a, n in enumerate((nx, ny, nz))]
    pos = np.empty((nz, ny, nx, 3), np.float32)
    pos[..., 0] = ax[0][None, None, :]
    pos[..., 1] = ax[1][None, :, None]
    pos[..., 2] = ax[2][:, None, None]
    return pos.reshape(-1, 3)


def sh_weight(num_dirs: int, samples: int) -> float:
    """the projection weight of a uniform direction set: 4 pi / (num_dirs * samples), rounded to float32"""
    return float(np.float32(4.0 * math.pi / (float(num_dirs) * float(samples))))


def default_max_dist(spacing) -> float:
    """the max_dist of bake_probe_visibility for a grid: 1.5 x the cell diagonal sqrt((sx*sx + sy*sy) + sz*sz), every operation in
    float32 - beyond it a surface cannot shadow a query of the probe's own cells"""
    s = np.asarray(spacing, np.float32).reshape(3)
    return float(np.float32(1.5) * np.sqrt(((s[0] * s[0]) + (s[1] * s[1])) + (s[2] * s[2])))


def grid_over_bounds(lo, hi, dims):
    """(origin, spacing) float32 [3] each of a grid of dims probes that spans the box lo..hi: the outermost probes lie on the box;
    an axis of one probe puts it in the middle (spacing 1 there, as for an axis without extent)"""
    lo = np.asarray(lo, np.float64).reshape(3)
    hi = np.asarray(hi, np.float64).reshape(3)
    origin, spacing = np.empty(3, np.float32), np.empty(3, np.float32)
    for a, n in enumerate(dims):
        if n > 1 and hi[a] > lo[a]:
            origin[a], spacing[a] = lo[a], (hi[a] - lo[a]) / (n - 1)
        else:
            origin[a], spacing[a] = (0.5 * (lo[a] + hi[a]) if n == 1 else lo[a]), 1.0
    return origin, spacing


def clearance(ctx, positions):
    """(dist [n] float32, point [n, 3] float32, tri [n] int32) of Context.closest_points(positions) (include/ptk.h
    ptk_closest_points): how far each probe lies from the nearest surface, where that surface is and which triangle it belongs to
    (inf, 0, -1 in a scene without triangles).  numpy positions, numpy results."""
    tri, dist, point, _ = ctx.closest_points(np.ascontiguousarray(positions, np.float32).reshape(-1, 3))
    return dist, point, tri


def inside(ctx, positions, mode="winding"):
    """[n] bool: the probes that sit inside the scene's closed geometry (Context.contains_points with the built-in directions,
    include/ptk.h ptk_contains_points) - probes to drop, not to relocate: no push along the line to the nearest surface point takes
    a probe out of a solid on the right side.  Means nothing for open meshes.  numpy positions, numpy result."""
    return ctx.contains_points(np.ascontiguousarray(positions, np.float32).reshape(-1, 3), None, mode).astype(bool)


def relocate(ctx, positions, min_dist, drop_inside=False):
    """(new positions [n, 3] float32, moved [n] bool): probes nearer to a surface than min_dist pushed away from it, straight along
    the line from the nearest surface point through the probe, until they lie min_dist from that point.  One query with max_dist =
    min_dist; a probe with a hit and dist > 0 moves to point + (p - point) * (min_dist / dist), in float32 in that order; a probe
    with a miss (far enough already), or with dist == 0 (on the surface: no direction to go), stays bit for bit.  ONE step: in a
    corner the move away from one wall may end nearer than min_dist to another, so a caller who needs the clearance iterates until
    nothing moves.  With drop_inside a third value follows, keep [n] bool = ~inside(ctx, positions): a probe inside a solid is not
    worth relocating; it is neither moved nor removed here (new and moved keep their length), the caller drops it by the mask."""
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    md = np.float32(min_dist)
    tri, dist, point, _ = ctx.closest_points(p, np.full(len(p), md, np.float32))
    moved = (tri >= 0) & (dist > 0)
    if drop_inside:
        keep = ~inside(ctx, p)
        moved &= keep
    new = p.copy()
    with np.errstate(all="ignore"):
        scale = (md / dist[moved]).astype(np.float32)
    new[moved] = point[moved] + (p[moved] - point[moved]) * scale[:, None]
    return (new, moved, keep) if drop_inside else (new, moved)
