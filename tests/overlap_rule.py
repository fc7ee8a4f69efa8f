"""numpy mirror of the overlap rules (include/ptk.h ptk_overlap_boxes, ptk_overlap_spheres): a vectorised
restatement, operation by operation in float32, over EVERY triangle of a scene - no tree -, with e1, e2 computed from
arrays["verts"] as float32 differences (the record packers' subtractions).  It gives accepted [n, m], and from it count and tris for
any k and tri_from.  Helper of tests/test_overlap_cpu.py, which holds it to an independent float64 separating-axis gap, and of
tests/test_gpu_overlap.py, which holds the kernel to it bit for bit.  Also the scenes those two share."""
import numpy as np

import closest_rule as CR

F32 = np.float32
MAX_K = 16                                     # PTK_OVERLAP_MAX_K
AXES = ("box x", "box y", "box z", "plane") + tuple(f"{f} x {j}" for f in ("e1", "e2-e1", "e2") for j in "xyz")
_NEXT = ((1, 2), (2, 0), (0, 1))               # j -> (k, l) = (j + 1, j + 2) mod 3


def _cross(x, y):
    """cross as ptk.h defines it: (xy*yz - yy*xz, xz*yx - yz*xx, xx*yy - yx*xy)"""
    return np.stack([x[..., 1] * y[..., 2] - y[..., 1] * x[..., 2], x[..., 2] * y[..., 0] - y[..., 2] * x[..., 0],
                     x[..., 0] * y[..., 1] - y[..., 0] * x[..., 1]], axis=-1)


def _min3(a, b, c):
    return np.fmin(np.fmin(a, b), c)           # (a NaN operand is ignored, as fminf)


def _max3(a, b, c):
    return np.fmax(np.fmax(a, b), c)


def _tri(verts):
    t = np.asarray(verts, F32).reshape(-1, 3, 3)
    return t[None, :, 0], (t[:, 1] - t[:, 0])[None], (t[:, 2] - t[:, 0])[None]


def box_axes(verts, lo, hi):
    """the box rule for every (box, triangle) pair: separated [13, n, m] bool, one plane per axis in the order of AXES, and
    valid [n] = the box has lo <= hi on every axis"""
    a, e1, e2 = _tri(verts)
    lo = np.asarray(lo, F32).reshape(-1, 1, 3); hi = np.asarray(hi, F32).reshape(-1, 1, 3)
    half = F32(0.5)
    with np.errstate(all="ignore"):
        valid = (lo <= hi).all(axis=(1, 2))
        c = (lo + hi) * half; h = (hi - lo) * half
        v0 = a - c; v1 = v0 + e1; v2 = v0 + e2
        assert c.dtype == F32 and h.dtype == F32 and v0.dtype == F32 and v1.dtype == F32 and v2.dtype == F32
        sep = []
        for j in range(3):
            sep.append((_min3(v0[..., j], v1[..., j], v2[..., j]) > h[..., j]) | (_max3(v0[..., j], v1[..., j], v2[..., j]) < -h[..., j]))
        n = _cross(e1, e2)
        d = [(n[..., 0] * v[..., 0] + n[..., 1] * v[..., 1]) + n[..., 2] * v[..., 2] for v in (v0, v1, v2)]
        r = (h[..., 0] * np.abs(n[..., 0]) + h[..., 1] * np.abs(n[..., 1])) + h[..., 2] * np.abs(n[..., 2])
        assert d[0].dtype == F32 and r.dtype == F32
        sep.append((_min3(*d) > r) | (_max3(*d) < -r))
        for f in (e1, e2 - e1, e2):
            for j in range(3):
                k, l = _NEXT[j]
                p = [v[..., l] * f[..., k] - v[..., k] * f[..., l] for v in (v0, v1, v2)]
                rr = h[..., k] * np.abs(f[..., l]) + h[..., l] * np.abs(f[..., k])
                assert p[0].dtype == F32 and rr.dtype == F32
                sep.append((_min3(*p) > rr) | (_max3(*p) < -rr))
    return np.stack([np.broadcast_to(s, sep[3].shape) for s in sep]), valid


def accepted_boxes(verts, lo, hi, chunk=64):
    """accepted [n, m] bool: no axis separates and the box is valid"""
    lo = np.asarray(lo, F32).reshape(-1, 3); hi = np.asarray(hi, F32).reshape(-1, 3)
    m = len(np.asarray(verts).reshape(-1, 9))
    out = np.zeros((len(lo), m), bool)
    for s in range(0, len(lo), chunk if m else len(lo) + 1):
        sep, valid = box_axes(verts, lo[s:s + chunk], hi[s:s + chunk])
        out[s:s + chunk] = ~sep.any(axis=0) & valid[:, None]
    return out


def accepted_spheres(verts, centers, radius, chunk=64):
    """accepted [n, m] bool: d2k of the closest rule finite and strictly below radius * radius; a NaN, zero or negative radius: none"""
    centers = np.asarray(centers, F32).reshape(-1, 3)
    n = len(centers)
    m = len(np.asarray(verts).reshape(-1, 9))
    r2 = CR._r2(np.asarray(radius, F32).reshape(n), n)
    assert r2.dtype == F32
    out = np.zeros((n, m), bool)
    for s in range(0, n, chunk if m else n + 1):
        d2k = CR.per_triangle(verts, centers[s:s + chunk])[0]
        with np.errstate(all="ignore"):
            out[s:s + chunk] = np.isfinite(d2k) & (d2k < r2[s:s + chunk, None])
    return out


def answer(accepted, k, tri_from=None):
    """(count [n] int32, tris [n, k] int32) of an accepted matrix: the considered triangles are those with index >= tri_from[i]
    (None or negative: 0)"""
    n, m = accepted.shape
    tf = np.zeros(n, np.int64) if tri_from is None else np.maximum(np.asarray(tri_from, np.int64).reshape(n), 0)
    ok = accepted & (np.arange(m)[None, :] >= tf[:, None])
    count = ok.sum(axis=1).astype(np.int32)
    tris = np.full((n, k), -1, np.int32)
    if k and m:
        # the rank of every accepted triangle among its query's accepted ones; the first k of them, in index order
        rank = np.cumsum(ok, axis=1) - 1
        q, t = np.nonzero(ok & (rank < k))
        tris[q, rank[q, t]] = t
    return count, tris


def mirror_boxes(arrays, lo, hi, k=0, tri_from=None):
    """what ptk_overlap_boxes must return"""
    return answer(accepted_boxes(arrays["verts"], lo, hi), k, tri_from)


def mirror_spheres(arrays, centers, radius, k=0, tri_from=None):
    """what ptk_overlap_spheres must return"""
    return answer(accepted_spheres(arrays["verts"], centers, radius), k, tri_from)


def csr(accepted):
    """(offsets [n + 1] int64, indices int32): every query's full list"""
    offsets = np.concatenate([[0], np.cumsum(accepted.sum(axis=1))]).astype(np.int64)
    return offsets, np.nonzero(accepted)[1].astype(np.int32)


# ---- an independent float64 computation ------------------------------------------------------------------------------------------------
def sat_gap64(verts, lo, hi, chunk=64):
    """[n, m] float64: the largest, over the 13 axes, of the separation of triangle and box along the axis divided by the axis'
    length - positive: apart by that distance at least; negative: they interpenetrate along every axis.  Zero axes are skipped.
    From the true vertices (float64 differences), not the records' e1, e2."""
    t = np.asarray(verts, np.float64).reshape(-1, 3, 3)
    lo = np.asarray(lo, np.float64).reshape(-1, 3); hi = np.asarray(hi, np.float64).reshape(-1, 3)
    edges = [t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 0] - t[:, 2]]
    unit = np.eye(3)
    axes = [np.broadcast_to(unit[j], (len(t), 3)) for j in range(3)] + [np.cross(edges[0], edges[1])]
    axes += [np.cross(unit[j][None], f) for f in edges for j in range(3)]
    out = np.empty((len(lo), len(t)))
    for s in range(0, len(lo), chunk):
        c = ((lo[s:s + chunk] + hi[s:s + chunk]) * 0.5)[:, None, None, :]          # [q, 1, 1, 3]
        h = ((hi[s:s + chunk] - lo[s:s + chunk]) * 0.5)[:, None, :]                # [q, 1, 3]
        v = t[None] - c                                                            # [q, m, 3 vertices, 3]
        gap = np.full((v.shape[0], len(t)), -np.inf)
        for L in axes:
            length = np.linalg.norm(L, axis=1)
            p = (v * L[None, :, None, :]).sum(axis=-1)                             # [q, m, 3]
            r = (h * np.abs(L)[None]).sum(axis=-1)                                 # [q, m]
            sep = np.maximum(p.min(axis=-1) - r, -p.max(axis=-1) - r)
            with np.errstate(all="ignore"):
                g = np.where(length > 0, sep / np.where(length > 0, length, 1.0), -np.inf)
            gap = np.maximum(gap, g)
        out[s:s + chunk] = gap
    return out


# ---- scenes the CPU and GPU tests share ----------------------------------------------------------------------------------------------
GENERATED = ((300, 0.15, 0), (4400, 0.08, 1), (6000, 0.03, 2))


def generated(n, sig, seed):
    """(verts [n, 9] float32, lo [400, 3], hi [400, 3] float32): random triangles around centres in the unit cube and 400 boxes"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 1, (n, 1, 3))
    verts = (c + rng.normal(0, sig, (n, 3, 3))).astype(F32).reshape(n, 9)
    centre = rng.uniform(-0.1, 1.1, (400, 3))
    half = rng.uniform(0.005, 0.15, (400, 3))
    return verts, (centre - half).astype(F32), (centre + half).astype(F32)


def spheres_of(lo, hi):
    """the spheres that go with a box set: centres = the box centres, radius = 1.5 x the first half extent"""
    lo = np.asarray(lo, np.float64); hi = np.asarray(hi, np.float64)
    return ((lo + hi) * 0.5).astype(F32), (1.5 * (hi[:, 0] - lo[:, 0]) * 0.5).astype(F32)


def boxes_in_bounds(arrays, n, seed, extent=(0.01, 0.2)):
    """(lo, hi) [n, 3] float32: boxes with centres in the vertex bounds grown by 10 % and half extents uniform in `extent` x the
    scene's extent"""
    rng = np.random.default_rng(seed)
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    vmin, vmax = v.min(axis=0), v.max(axis=0)
    size = float((vmax - vmin).max())
    centre = rng.uniform(vmin - 0.1 * size, vmax + 0.1 * size, (n, 3))
    half = rng.uniform(extent[0] * size, extent[1] * size, (n, 3))
    return (centre - half).astype(F32), (centre + half).astype(F32)


def grid_boxes():
    """(lo, hi) for closest_rule.grid_mesh: dyadic boxes whose faces lie ON grid lines - square cells and blocks of cells, flat
    (z = 0 exactly), above the plane (touching nothing) and touching it from above.  Exact arithmetic: the answer is a fixed table"""
    s = CR.GRID_STEP
    lo, hi = [], []
    for (i0, j0, ni, nj, z0, z1) in ((0, 0, 1, 1, -1, 1), (5, 7, 1, 1, 0, 0), (10, 3, 2, 3, -0.5, 0), (20, 20, 4, 4, 0, 0.5),
                                     (47, 47, 1, 1, -1, 1), (8, 8, 1, 1, 0.125, 1), (0, 0, 48, 48, -1, 1), (30, 2, 1, 2, -0.25, 0.25)):
        lo.append((i0 * s, j0 * s, z0)); hi.append(((i0 + ni) * s, (j0 + nj) * s, z1))
    return np.array(lo, F32), np.array(hi, F32)


def grid_expected(lo, hi):
    """the fixed table for grid_boxes, from the grid's construction alone.  Cell (i, j) holds the lower triangle 2 (i * 48 + j), with
    vertices (i, j), (i + 1, j), (i, j + 1), and the upper triangle 2 (i * 48 + j) + 1, with vertices (i + 1, j), (i + 1, j + 1),
    (i, j + 1).  A closed box whose z range holds 0 and whose sides lie on the grid lines i0, i1 and j0, j1 meets every triangle of
    the cells i0 - 1 .. i1, j0 - 1 .. j1 - each has a vertex or a side on the box - but two: the lower triangle of cell
    (i0 - 1, j0 - 1) and the upper triangle of cell (i1, j1), whose hypotenuses pass the box's corners (i0, j0) and (i1, j1) half a
    cell away."""
    n, s = CR.GRID_N, CR.GRID_STEP
    out = np.zeros((len(lo), 2 * n * n), bool)
    for q in range(len(lo)):
        if not (lo[q, 2] <= 0 <= hi[q, 2]):
            continue
        i0, j0, i1, j1 = (int(round(float(x) / s)) for x in (lo[q, 0], lo[q, 1], hi[q, 0], hi[q, 1]))
        for i in range(max(i0 - 1, 0), min(i1, n - 1) + 1):
            for j in range(max(j0 - 1, 0), min(j1, n - 1) + 1):
                out[q, 2 * (i * n + j)] = not (i == i0 - 1 and j == j0 - 1)
                out[q, 2 * (i * n + j) + 1] = not (i == i1 and j == j1)
    return out
