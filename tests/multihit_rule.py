"""numpy mirror of the multi-hit rule (include/ptk.h ptk_multihit_rays): the crossings rule's Moeller-Trumbore
over EVERY triangle of a scene - no tree - (crossings_rule.per_triangle, crossing_masks), and a stable sort of each ray's crossings
by t, which is the rule's (t, triangle index) order.  Helper of tests/test_multihit_cpu.py, which holds it to a float64 brute
force, and of tests/test_gpu_multihit.py, which holds the kernel to it bit for bit.  Also the two scenes those tests share."""
import numpy as np

import crossings_rule as XR

F32 = np.float32
MAX_HITS = 16                       # PTK_MULTIHIT_MAX
NAMES = ("count", "tri", "t", "bary", "side")


def multihit(arrays, ro, rd, max_hits, tmax=None, budget=1 << 22):
    """(count [n] int32, tri [n, K] int32, t [n, K] float32, bary [n, K, 2] float32, side [n, K] int8): what ptk_multihit_rays
    must return for K = max_hits.  tmax None: +inf for every ray"""
    K = int(max_hits)
    if not 1 <= K <= MAX_HITS:
        raise ValueError("max_hits must be in 1 .. 16")
    ro = np.ascontiguousarray(ro, F32).reshape(-1, 3); rd = np.ascontiguousarray(rd, F32).reshape(-1, 3)
    n = len(ro)
    verts = np.asarray(arrays["verts"], F32).reshape(-1, 9)
    count = np.zeros(n, np.int32); tri = np.full((n, K), -1, np.int32); t_out = np.full((n, K), np.inf, F32)
    bary = np.zeros((n, K, 2), F32); side = np.zeros((n, K), np.int8)
    if n == 0 or len(verts) == 0:
        return count, tri, t_out, bary, side
    tm = XR._tmax(tmax, n)
    chunk = max(1, budget // len(verts))
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        a, u, v, t = XR.per_triangle(verts, ro[s:e], rd[s:e])
        fr, bk = XR.crossing_masks(verts, ro[s:e], rd[s:e], tm[s:e])
        cross = fr | bk
        key = np.where(cross, t, F32(np.inf))                            # an accepted t is finite: +inf sorts behind every crossing
        order = np.argsort(key, axis=1, kind="stable")[:, :K]            # stable: equal t to the smaller index
        k = order.shape[1]                                               # (fewer triangles than K)
        rows = np.arange(e - s)[:, None]
        kept = cross[rows, order]
        count[s:e] = kept.sum(axis=1)
        tri[s:e, :k] = np.where(kept, order, -1)
        t_out[s:e, :k] = np.where(kept, t[rows, order], F32(np.inf))
        bary[s:e, :k, 0] = np.where(kept, u[rows, order], F32(0))
        bary[s:e, :k, 1] = np.where(kept, v[rows, order], F32(0))
        side[s:e, :k] = np.where(kept, np.where(a[rows, order] > 0, 1, -1), 0)
    return count, tri, t_out, bary, side


def cut(answer, k):
    """the first k columns of an answer for K >= k: the answer for k"""
    count, tri, t, bary, side = answer
    return (np.minimum(count, np.int32(k)), np.ascontiguousarray(tri[:, :k]), np.ascontiguousarray(t[:, :k]),
            np.ascontiguousarray(bary[:, :k]), np.ascontiguousarray(side[:, :k]))


def rows_of(answer, sel):
    return tuple(x[sel] for x in answer)


# ---- the two scenes ------------------------------------------------------------------------------------------------------------------
def soup(n, size, seed):
    """[n, 9] float32: n triangles, a centre uniform in [-1, 1]^3 plus three corners uniform within `size` of it - a ray through the
    soup crosses anything from none to dozens of them, in no order the tree knows"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    return (c + size * rng.uniform(-1, 1, (n, 3, 3))).astype(F32).reshape(n, 9)


def slabs(L):
    """[m, 9] float32: L squares [-1, 1]^2 at z = i / L, two triangles each, wound alternately; every fourth square is there twice,
    bit for bit - coincident triangles with equal t along any ray"""
    out = []
    for i in range(L):
        z = i / L
        q = [(-1, -1, z), (1, -1, z), (1, 1, z), (-1, 1, z)]
        if i % 2:
            q = q[::-1]
        two = [q[0] + q[1] + q[2], q[0] + q[2] + q[3]]
        out += two
        if i % 4 == 0:
            out += two
    return np.asarray(out, np.float64).astype(F32)
