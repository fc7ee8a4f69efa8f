"""Ray sets for Context.trace_rays / PathTracer.TraceRays (include/ptk.h ptk_trace_rays): camera models the library's own
perspective camera does not cover, as plain (origins, directions) arrays.  Host only, no GPU."""
from __future__ import annotations

import numpy as np


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def equirect_rays(pos, dir, up, width: int, height: int):
    """(origins, dirs), float32 [height * width, 3] each, rows top-down: the rays through the pixel centres of a latitude-longitude
    panorama (2:1 for the full sphere) about the camera frame of ptk_set_camera - forward = normalize(dir), right =
    normalize(cross(up, dir)), and the up axis completed at right angles to both.  Column x looks longitude ((x + 1/2) / width -
    1/2) * 2 pi to the right of forward, row y latitude (1/2 - (y + 1/2) / height) * pi above the horizon: the centre of the image
    looks along dir, the top row towards up.  Computed in float64 and rounded once, so the directions are unit vectors to float32's
    last bit or so; every origin is pos."""
    f = _unit(dir)
    r = _unit(np.cross(_unit(up), f))
    u = np.cross(f, r)
    lon = ((np.arange(width, dtype=np.float64) + 0.5) / width - 0.5) * (2.0 * np.pi)
    lat = (0.5 - (np.arange(height, dtype=np.float64) + 0.5) / height) * np.pi
    cl, sl = np.cos(lat)[:, None, None], np.sin(lat)[:, None, None]
    d = cl * (np.cos(lon)[None, :, None] * f + np.sin(lon)[None, :, None] * r) + sl * u
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    dirs = np.ascontiguousarray(d.reshape(-1, 3), np.float32)
    origins = np.ascontiguousarray(np.broadcast_to(np.asarray(pos, np.float64), dirs.shape), np.float32)
    return origins, dirs
