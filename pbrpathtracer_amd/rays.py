"""Ray sets for Context.trace_rays / PathTracer.TraceRays (include/ptk.h ptk_trace_rays): camera models the library's own
perspective camera does not cover, as plain (origins, directions) arrays - and for Context.intersect_rays / occluded_rays
(ptk_intersect_rays, ptk_occluded_rays): segments between point pairs and ambient occlusion - and, over Context.multihit_rays
(ptk_multihit_rays), the length of a ray inside the geometry and the surfaces between two points - and, over
Context.surface_attributes (ptk_surface_attributes), the guide planes of a denoiser for any ray set.  Host only but for the
functions that take a context, which run their rays through it."""
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


def hit_guides(ctx, origins, dirs, sample: int = 0, seed: int = 0):
    """What the rays (origins[i], dirs[i]) see, as a perspective frame's first-hit feature planes give it for the one camera: dict of
    id [n] int32 (the triangle, -1 on a miss), depth [n] float32 (t, inf on a miss), position, normal, albedo, emission [n, 3] float32
    (0 on a miss) - one Context.intersect_rays call (the opacity draws of sample `sample` of `seed`) and one
    Context.surface_attributes call over its tri and bary with the rays' directions, so normal is the shading normal turned towards
    the ray's origin.  The guides of Context.denoise_planes for an image traced along these rays (mask = id): a panorama
    (equirect_rays), a fisheye, probes' views.  numpy arrays in and out."""
    from . import ptk
    tri, t, bary, _ = ctx.intersect_rays(origins, dirs, sample=sample, seed=seed)
    want = 1 << ptk.ATTR_POSITION | 1 << ptk.ATTR_NORMAL | 1 << ptk.ATTR_ALBEDO | 1 << ptk.ATTR_EMISSION
    at = ctx.surface_attributes(tri, bary, dirs, want)
    return dict(id=tri, depth=t, position=at["position"], normal=at["normal"], albedo=at["albedo"], emission=at["emission"])


def segment_rays(a, b):
    """(origins, dirs, tmax) for the segments from a[i] to b[i], [n, 3] each: origins = a, dirs = b - a in float32 (not
    normalised) and tmax = 1, so that Context.occluded_rays(origins, dirs, tmax) asks "is anything strictly between the two points"
    and the visibility between the pairs is 1 - occluded."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(b, np.float32).reshape(-1, 3)
    assert len(a) == len(b), "as many end points as start points"
    return a, np.ascontiguousarray(b - a), np.ones(len(a), np.float32)


def count_layers(ctx, a, b):
    """[n] int32: the number of surfaces crossed strictly between the points a[i] and b[i] - one Context.crossings_rays call over
    segment_rays(a, b), front + back (include/ptk.h ptk_crossings_rays: every triangle the segment passes through counts, whatever
    its material; a segment through a shared edge may count both neighbours).  "How many walls between A and B"; 0 = a clear line."""
    front, back = ctx.crossings_rays(*segment_rays(a, b))
    return front + back


def inside_length(count, t, side, max_hits: int):
    """(length [n] float32, complete [n] bool) from Context.multihit_rays' count [n], t [n, K] and side [n, K]: the length of each
    ray, in units of |dir|, that lies inside the geometry.  Each list is walked with a running sum of side that starts at 0 - the
    origin is taken to be outside - and t[j + 1] - t[j] is added, in float32 and in list order, for every j < count - 1 at which
    the running sum after crossing j is nonzero: between the two crossings the ray has entered more often than it has left, or
    the other way round, so the result does not depend on which way the mesh is wound, and a shared edge that both neighbours
    accept (+1, +1, -1, -1) is one interval.  complete = count < max_hits: the list was not cut, so the length is the whole
    ray's."""
    count = np.asarray(count, np.int32).reshape(-1)
    n = len(count)
    t = np.asarray(t, np.float32).reshape(n, -1) if n else np.zeros((0, 1), np.float32)
    side = np.asarray(side, np.int8).reshape(t.shape)
    length = np.zeros(n, np.float32)
    run = np.zeros(n, np.int32)
    for j in range(t.shape[1] - 1):
        run = run + side[:, j]
        add = (j + 1 < count) & (run != 0)
        with np.errstate(invalid="ignore"):                     # (inf - inf behind a list's end: not taken)
            length = np.where(add, length + (t[:, j + 1] - t[:, j]), length)
    return length, count < int(max_hits)


def thickness(ctx, origins, dirs, max_hits: int = 16, tmax=None):
    """(length [n] float32, complete [n] bool): inside_length of one Context.multihit_rays call - how much solid each ray passes
    through among its first max_hits crossings (before tmax).  numpy arrays in and out."""
    count, _, t, _, side = ctx.multihit_rays(origins, dirs, max_hits, tmax)
    return inside_length(count, t, side, max_hits)


def layers_between(ctx, a, b, max_hits: int):
    """Context.multihit_rays over segment_rays(a, b): (count, tri, t, bary, side) of the first max_hits surfaces strictly between the
    points a[i] and b[i], in order from a; t is the fraction of the segment.  "Which walls lie between A and B"."""
    origins, dirs, tmax = segment_rays(a, b)
    return ctx.multihit_rays(origins, dirs, max_hits, tmax)


def ambient_occlusion_rays(points, normals, dirs, offset):
    """The rays of ambient_occlusion: for point p with normal n the rays (p + n * offset, d_j) over the directions d_j with float32
    c_j = (n.x * d.x + n.y * d.y) + n.z * d.z > 0, point-major then in direction order - that order is a ray's global index.
    Returns (origins [m, 3], ray_dirs [m, 3], point [m] int64 - the point each ray belongs to -, cos [m] float32 - its c_j)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    assert len(n) == len(p), "one normal per point"
    c = (n[:, None, 0] * d[None, :, 0] + n[:, None, 1] * d[None, :, 1]) + n[:, None, 2] * d[None, :, 2]      # [points, dirs], float32
    pi, di = np.nonzero(c > 0)                                                                                # row-major: point-major
    origins = np.ascontiguousarray(p[pi] + n[pi] * np.float32(offset))
    return origins, np.ascontiguousarray(d[di]), pi, np.ascontiguousarray(c[pi, di])


def ambient_occlusion_fold(num_points: int, point, cos, occluded):
    """float32 [num_points] of sum c_j (1 - occluded_j) / sum c_j over each point's rays, summed in float64; 1 where a point has
    no ray."""
    w = np.asarray(cos, np.float64)
    open_ = np.bincount(point, weights=w * (1.0 - np.asarray(occluded, np.float64)), minlength=num_points)
    total = np.bincount(point, weights=w, minlength=num_points)
    return np.where(total > 0, open_ / np.where(total > 0, total, 1.0), 1.0).astype(np.float32)


def ambient_occlusion(ctx, points, normals, dirs, radius, offset, sample: int = 0, seed: int = 0):
    """Cosine-weighted openness of the surface points (points[i], normals[i]) over the direction set dirs (probes.fibonacci_dirs for
    instance): one Context.occluded_rays call over ambient_occlusion_rays with tmax = radius (in units of |d_j|), folded by
    ambient_occlusion_fold.  1 = nothing within radius, 0 = closed in.  numpy arrays in, float32 [len(points)] out."""
    origins, ray_dirs, point, cos = ambient_occlusion_rays(points, normals, dirs, offset)
    occ = ctx.occluded_rays(origins, ray_dirs, np.full(len(origins), radius, np.float32), sample=sample, seed=seed)
    return ambient_occlusion_fold(len(np.asarray(points).reshape(-1, 3)), point, cos, occ)
