"""Worked uses of overlap queries (include/ptk.h ptk_overlap_boxes, ptk_overlap_spheres): every triangle of a region
as CSR lists, paged through tri_from, and a voxel occupancy grid.  `ctx` is anything with Context's overlap_boxes / overlap_spheres
(and contains_points for solid grids): a ptk.Context or a PathTracer.  numpy in, numpy out."""
from __future__ import annotations

import numpy as np

from .probes import grid_positions

F32 = np.float32
PAGE = 16                                      # PTK_OVERLAP_MAX_K: the most indices one call lists per query


def _all(query, a, b):
    """page `query(a, b, k, tri_from) -> (count, tris)` until every list is complete: (offsets [n + 1] int64, indices int32)"""
    n = len(a)
    count, tris = query(a, b, PAGE, None)
    offsets = np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int64)
    indices = np.empty(int(offsets[-1]), np.int32)
    got = np.minimum(count, PAGE).astype(np.int64)
    rows = np.arange(n)
    cols = np.arange(PAGE)[None, :]

    def put(which, start, tris, have):
        keep = cols < have[:, None]
        at = (offsets[which] + start)[:, None] + cols
        indices[at[keep]] = tris[keep]

    put(rows, np.zeros(n, np.int64), tris, got)
    open_ = rows[got < count]
    done = got.copy()
    last = tris[:, PAGE - 1].copy() if n else np.zeros(0, np.int32)
    while len(open_):
        # the queries whose lists are still cut off, again from behind the last index listed
        left, tris = query(a[open_], b[open_], PAGE, (last[open_] + 1).astype(np.int32))
        have = np.minimum(left, PAGE).astype(np.int64)
        put(open_, done[open_], tris, have)
        done[open_] += have
        last[open_] = tris[:, PAGE - 1]
        open_ = open_[have < left]
    return offsets, indices


def all_in_boxes(ctx, lo, hi):
    """(offsets [n + 1] int64, indices int32): indices[offsets[i] : offsets[i + 1]] = every triangle that meets the closed box
    [lo[i], hi[i]], ascending - ptk_overlap_boxes called again with tri_from = last listed + 1 for the boxes whose lists were cut
    off at 16, until none is"""
    lo = np.ascontiguousarray(lo, F32).reshape(-1, 3); hi = np.ascontiguousarray(hi, F32).reshape(-1, 3)
    assert len(lo) == len(hi), "one hi per lo"
    return _all(lambda a, b, k, tf: ctx.overlap_boxes(a, b, k, tf), lo, hi)


def all_in_spheres(ctx, centers, radius):
    """all_in_boxes for the spheres (centers[i], radius[i]) (ptk_overlap_spheres)"""
    centers = np.ascontiguousarray(centers, F32).reshape(-1, 3); radius = np.ascontiguousarray(radius, F32).reshape(-1)
    assert len(centers) == len(radius), "one radius per centre"
    return _all(lambda a, b, k, tf: ctx.overlap_spheres(a, b, k, tf), centers, radius)


def voxel_boxes(origin, spacing, dims):
    """(lo, hi, centres) [nz * ny * nx, 3] float32 of the voxels of a grid: voxel (ix, iy, iz) is centred on the grid point origin +
    i * spacing (probes.grid_positions, x fastest) and reaches half a spacing to either side, in float32: centre -+ spacing * 0.5"""
    centres = grid_positions(dims, origin, spacing)
    half = np.asarray(spacing, F32).reshape(3) * F32(0.5)
    return centres - half, centres + half, centres


def voxel_occupancy(ctx, origin, spacing, shape, solid=False):
    """bool [NZ, NY, NX] for shape = (NX, NY, NZ), laid out as render --distance-field's arrays: True where a triangle meets the
    voxel's closed box (voxel_boxes; overlap_boxes' count > 0) - a surface voxelisation, conservative: neighbours that share a face
    the surface lies in are both set.  solid=True ORs in contains_points of the voxel centres (closed geometry: DESIGN.md 4.24)."""
    nx, ny, nz = (int(n) for n in shape)
    lo, hi, centres = voxel_boxes(origin, spacing, (nx, ny, nz))
    count, _ = ctx.overlap_boxes(lo, hi, 0)
    occ = np.asarray(count) > 0
    if solid:
        occ = occ | (np.asarray(ctx.contains_points(centres)) != 0)
    return occ.reshape(nz, ny, nx)
