"""numpy mirror of the K-nearest rule (include/ptk.h ptk_nearest_triangles): closest_rule.per_triangle - the rule of
ptk_closest_points, operation by operation in float32 - over EVERY triangle of a scene, the accept mask, and one sort by the integer
(bits(d2k) << 32) | triangle index.  No tree.  Helper of tests/test_knearest_cpu.py, which holds it to the K smallest float64
distances, and of tests/test_gpu_knearest.py, which holds the kernel to it bit for bit."""
import numpy as np

import closest_rule as CR

F32 = np.float32
NAMES = ("count", "tri", "dist", "point", "bary")
FREE = np.uint64(0xffffffffffffffff)


def mirror_sets(arrays, points, sets, chunk=64):
    """mirror for each (k, max_dist) of the list `sets`, with the per-triangle rule evaluated once: a list of 5-tuples"""
    points = np.ascontiguousarray(points, F32).reshape(-1, 3)
    n = len(points)
    verts = np.asarray(arrays["verts"], F32).reshape(-1, 9)
    m = len(verts)
    outs = [(np.zeros(n, np.int32), np.full((n, k), -1, np.int32), np.full((n, k), np.inf, F32), np.zeros((n, k, 3), F32),
             np.zeros((n, k, 2), F32)) for k, _ in sets]
    if m == 0 or n == 0:
        return outs
    bounds = [CR._r2(md, n) for _, md in sets]
    index = np.arange(m, dtype=np.uint64)[None]
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        d2k, v, w, q, _ = CR.per_triangle(verts, points[s:e])
        rows = np.arange(e - s)[:, None]
        bits = d2k.view(np.uint32).astype(np.uint64) << np.uint64(32) | index
        for (k, _), r2, out in zip(sets, bounds, outs):
            with np.errstate(all="ignore"):
                ok = np.isfinite(d2k) & (d2k < r2[s:e, None])
            key = np.where(ok, bits, FREE)                                  # (an accepted d2k is finite and >= +0: its key is below FREE)
            kk = min(k, m)
            # the kk smallest keys in order (no two accepted keys are equal: the index is in them); the index is a key's low word
            first = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1)
            kept = first != FREE
            order = np.where(kept, first & np.uint64(0xffffffff), np.uint64(0)).astype(np.int64)
            count, tri, dist, point, bary = out
            count[s:e] = kept.sum(axis=1)
            tri[s:e, :kk] = np.where(kept, order, -1)
            with np.errstate(all="ignore"):
                dist[s:e, :kk] = np.where(kept, np.sqrt(d2k[rows, order]), F32(np.inf))
            point[s:e, :kk] = np.where(kept[..., None], q[rows, order], F32(0))
            bary[s:e, :kk, 0] = np.where(kept, v[rows, order], F32(0))
            bary[s:e, :kk, 1] = np.where(kept, w[rows, order], F32(0))
    return outs


def mirror(arrays, points, k, max_dist=None):
    """(count [n] int32, tri [n, k] int32, dist [n, k] float32, point [n, k, 3] float32, bary [n, k, 2] float32): what
    ptk_nearest_triangles must return"""
    return mirror_sets(arrays, points, [(k, max_dist)])[0]


def reference64(verts, points, k):
    """[n, min(k, triangles)] float64: the k smallest of closest_rule.distances64 per point, ascending"""
    d = CR.distances64(verts, points)
    return np.sort(d, axis=1)[:, :k]
