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
