"""Lightmap helpers for Context.bake_lightmap / PathTracer.BakeLightmap (include/ptk.h ptk_bake_lightmap).

grid_atlas is a trivial automatic unwrap - the worked use that keeps the Python path honest, as rays.equirect_rays is for ray
queries: the reference's scenes carry TEXTURE uvs, which overlap, and a lightmap needs charts that do not."""
from __future__ import annotations

import math

import numpy as np


def grid_layout(num_tris: int, width: int, height: int, gutter: int = 1):
    """(cols, rows, cell_w, cell_h) of grid_atlas: whole-texel cells, two triangles per cell, the cells as large as the map allows."""
    if num_tris < 0 or width < 1 or height < 1 or gutter < 0:
        raise ValueError("grid_atlas: negative count or gutter, or an empty map")
    cells = max(1, (num_tris + 1) // 2)
    need = 3 * gutter + 2            # the inset rectangle's legs stay >= 1.75 texels: each triangle contains a texel centre
    best = None
    for cols in range(1, width // need + 1):
        rows = (cells + cols - 1) // cols
        cw, ch = width // cols, height // rows if rows <= height else 0
        if cw < need or ch < need:
            continue
        key = (min(cw, ch), cw * ch)
        if best is None or key > best[0]:
            best = (key, (cols, rows, cw, ch))
    if best is None:
        raise ValueError(f"grid_atlas: a {width}x{height} map is too small for {num_tris} triangles with gutter {gutter} "
                         f"(each pair needs a cell of {need}x{need} texels)")
    return best[1]


def grid_atlas(num_tris: int, width: int, height: int, gutter: int = 1) -> np.ndarray:
    """uvs[num_tris][6] (the layout of ptk_scene_desc.uvs) of a regular grid of charts: triangles 2c and 2c + 1 are the two halves
    of cell c's rectangle, cells row-major from the map's bottom-left.  A cell spans whole texels; its rectangle is the cell
    inset by `gutter` texels on every side, and each half is pulled back from the diagonal by gutter + 0.25 texels along both
    axes, so the two triangles are disjoint, no two charts share a texel centre and gutter = 0 still separates them.
    Every chart contains at least one texel centre.  Raises ValueError when the map is too small for the count."""
    cols, rows, cw, ch = grid_layout(num_tris, width, height, gutter)
    uv = np.zeros((num_tris, 6), np.float64)
    d = gutter + 0.25
    for k in range(num_tris):
        c = k // 2
        x0, y0 = (c % cols) * cw + gutter, (c // cols) * ch + gutter
        x1, y1 = x0 + cw - 2 * gutter, y0 + ch - 2 * gutter
        if k % 2 == 0:
            pts = (x0, y0, x1 - d, y0, x0, y1 - d)
        else:
            pts = (x1, y1, x0 + d, y1, x1, y0 + d)
        uv[k] = pts
    uv[:, 0::2] /= width
    uv[:, 1::2] /= height
    return np.ascontiguousarray(uv, np.float32)


def guides(ctx, owner, bary):
    """(albedo, normal) [H, W, 3] float32 each: the diffuse colour after its texture and the shading normal - smoothed, normal-mapped,
    not flipped - at every covered texel of a coverage (Context.bake_coverage's owner [H, W] and bary [H, W, 2]), 0 where owner is
    -1: one Context.surface_attributes call (include/ptk.h ptk_surface_attributes).  What denoise takes as `normals` and `albedo=`
    in place of the owner's face normal and no albedo.  ctx: a Context or a PathTracer.  numpy in, numpy out."""
    from . import ptk
    owner = np.ascontiguousarray(owner, np.int32)
    h, w = owner.shape
    at = ctx.surface_attributes(owner.reshape(-1), np.ascontiguousarray(bary, np.float32).reshape(-1, 2), None,
                                1 << ptk.ATTR_ALBEDO | 1 << ptk.ATTR_NORMAL)
    return at["albedo"].reshape(h, w, 3), at["normal"].reshape(h, w, 3)


def denoise(ctx, image, owner, pos, normals, params=None, albedo=None, variance=None, want_variance: bool = False):
    """The a-trous denoiser (include/ptk.h ptk_denoise_planes, Context.denoise_planes) over a baked lightmap: image [H, W, 3] - the
    mean, sums / spp -, owner [H, W] int32 as the mask (uncovered texels, -1, keep their bits and take no part), pos [H, W, 3] from
    Context.bake_coverage as the guide position and the owner's face normal as the guide normal.  normals: [triangles, 3] face
    normals (the scene's tbn[:, 0:3]) or a ready [H, W, 3] plane.  params None: ptk.denoise_defaults for the extent of the covered
    positions.  Apply it before dilate_lightmap: the padding texels then copy denoised values.  numpy in, numpy out."""
    from . import ptk
    owner = np.ascontiguousarray(owner, np.int32)
    h, w = owner.shape
    normals = np.asarray(normals, np.float32)
    if normals.shape != (h, w, 3):
        normals = normals.reshape(-1, 3)[np.maximum(owner, 0)]
    if params is None:
        p = np.asarray(pos, np.float64).reshape(-1, 3)[owner.reshape(-1) >= 0]
        params = ptk.denoise_defaults(float(np.linalg.norm(p.max(axis=0) - p.min(axis=0))) if len(p) else 1.0, variance is not None)
    return ctx.denoise_planes(image, owner, np.ascontiguousarray(normals), pos, params, albedo=albedo, variance=variance,
                              want_variance=want_variance)
