"""numpy mirror of the closest-point rule (include/ptk.h ptk_closest_points): a vectorised restatement, operation
by operation in float32, over EVERY triangle of a scene - no tree -, with e1, e2 computed from arrays["verts"] as float32
differences (the record packers' subtractions).  Helper of tests/test_closest_cpu.py, which holds it to an independent float64
computation, and of tests/test_gpu_closest.py, which holds the kernel to it bit for bit.  Also the scenes those two share."""
import numpy as np

F32 = np.float32
K_SLACK, REL_SLACK = 2.0, 2.0 ** -19          # PTK_CLOSEST_K, PTK_CLOSEST_REL (pbrpathtracer_amd/csrc/ptk_closest.h)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def per_triangle(verts, points):
    """the rule for every (point, triangle) pair: (d2k [n, m], v, w, q [n, m, 3], region [n, m]), all float32 but the region"""
    t = np.asarray(verts, F32).reshape(-1, 3, 3)
    a, e1, e2 = t[None, :, 0], (t[:, 1] - t[:, 0])[None], (t[:, 2] - t[:, 0])[None]
    p = np.asarray(points, F32).reshape(-1, 1, 3)
    zero, one = F32(0), F32(1)
    with np.errstate(all="ignore"):
        ap = p - a; bp = ap - e1; cp = ap - e2
        d1, d2, d3, d4, d5, d6 = _dot(e1, ap), _dot(e2, ap), _dot(e1, bp), _dot(e2, bp), _dot(e1, cp), _dot(e2, cp)
        vc = d1 * d4 - d3 * d2; vb = d5 * d2 - d1 * d6; va = d3 * d6 - d5 * d4; e43 = d4 - d3; e56 = d5 - d6
        conds = ((d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0))
        region = np.select(conds, (0, 1, 3, 2, 4, 5), 7).astype(np.int8)
        den = (va + vb) + vc
        w5 = e43 / (e43 + e56)
        v = np.select([region == 0, region == 1, region == 3, region == 2, region == 4, region == 5],
                      [zero, one, d1 / (d1 - d3), zero, zero, one - w5], vb / den).astype(F32)
        w = np.select([region == 0, region == 1, region == 3, region == 2, region == 4, region == 5],
                      [zero, zero, zero, one, d2 / (d2 - d6), w5], vc / den).astype(F32)
        v = np.where(v > 0, v, zero); v = np.where(v < 1, v, one)
        w = np.where(w > 0, w, zero); top = one - v; w = np.where(w < top, w, top)
        q = (a + e1 * v[..., None]) + e2 * w[..., None]
        d = p - q
        d2k = _dot(d, d)
    assert d2k.dtype == F32 and q.dtype == F32 and v.dtype == F32 and w.dtype == F32
    return d2k, v, w, q, region


def _r2(max_dist, n):
    """the squared bound of each query: +inf without one; a NaN, zero or negative max_dist gives 0 (d2k < 0 accepts nothing)"""
    with np.errstate(all="ignore"):
        if max_dist is None:
            return np.full(n, np.inf, F32)
        md = np.asarray(max_dist, F32).reshape(n)
        return np.where(md > 0, md * md, F32(0)).astype(F32)


def mirror_radii(arrays, points, radii, chunk=64):
    """mirror_full for each max_dist of the list `radii` (None: no bound), with the per-triangle rule evaluated once: a list of dicts"""
    points = np.ascontiguousarray(points, F32).reshape(-1, 3)
    n = len(points)
    verts = np.asarray(arrays["verts"], F32).reshape(-1, 9)
    outs = [dict(tri=np.full(n, -1, np.int32), dist=np.full(n, np.inf, F32), point=np.zeros((n, 3), F32), bary=np.zeros((n, 2), F32),
                 region=np.full(n, -1, np.int8), ties=np.zeros(n, np.int32)) for _ in radii]
    if len(verts) == 0 or n == 0:
        return outs
    bounds = [_r2(md, n) for md in radii]
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        d2k, v, w, q, region = per_triangle(verts, points[s:e])
        for out, r2 in zip(outs, bounds):
            with np.errstate(all="ignore"):
                ok = np.isfinite(d2k) & (d2k < r2[s:e, None])
            key = np.where(ok, d2k, F32(np.inf))
            k = np.argmin(key, axis=1)                                      # (the first of equal minima: the smaller index)
            rows = np.arange(e - s)
            hit = ok[rows, k]
            i = s + rows[hit]
            kk = k[hit]
            out["tri"][i] = kk
            out["dist"][i] = np.sqrt(d2k[rows[hit], kk])
            out["point"][i] = q[rows[hit], kk]
            out["bary"][i, 0] = v[rows[hit], kk]; out["bary"][i, 1] = w[rows[hit], kk]
            out["region"][i] = region[rows[hit], kk]
            out["ties"][i] = (ok & (d2k == key[rows, k][:, None]))[rows[hit]].sum(axis=1)
    return outs


def mirror_full(arrays, points, max_dist=None, chunk=64):
    """the answer of the rule with what the tests ask about it: dict of tri, dist, point, bary (the outputs of ptk_closest_points),
    region (of the winner, -1 on a miss) and ties (accepted triangles that share the winning d2k, 0 on a miss)"""
    return mirror_radii(arrays, points, [max_dist], chunk)[0]


def mirror(arrays, points, max_dist=None):
    """(tri [n] int32, dist [n] float32, point [n, 3] float32, bary [n, 2] float32): what ptk_closest_points must return"""
    m = mirror_full(arrays, points, max_dist)
    return m["tri"], m["dist"], m["point"], m["bary"]


# ---- the slack of DESIGN §4.17 -----------------------------------------------------------------------------------------------------
def scene_bound(verts):
    """ptk_ctx::scene_bound: 3.1 x (1.01 x the largest |vertex coordinate| + 1e-3)"""
    return 3.1 * (1.01 * float(np.abs(np.asarray(verts, np.float64)).max()) + 1e-3)


def slack(verts, points):
    """E of each point: what a computed closest point and the triangle (and a decoded box) can disagree by, in position units"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return K_SLACK * 2.0 ** -21 * (np.abs(p).max(axis=1) + scene_bound(verts))


# ---- an independent float64 computation ------------------------------------------------------------------------------------------------
def _segment_dist(p, a, b):
    ab = b - a
    L = (ab * ab).sum(axis=-1)
    with np.errstate(all="ignore"):
        t = np.where(L > 0, ((p - a) * ab).sum(axis=-1) / np.where(L > 0, L, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    return np.linalg.norm(p - (a + ab * t[..., None]), axis=-1)


def distances64(verts, points):
    """[n, m] float64 distances from every point to every triangle: the minimum over the projection onto the triangle's plane, where
    that falls inside the triangle, and the distances to its three sides"""
    t = np.asarray(verts, np.float64).reshape(-1, 3, 3)
    p = np.asarray(points, np.float64).reshape(-1, 1, 3)
    a, b, c = t[None, :, 0], t[None, :, 1], t[None, :, 2]
    best = np.minimum(np.minimum(_segment_dist(p, a, b), _segment_dist(p, b, c)), _segment_dist(p, c, a))
    nrm = np.cross(b - a, c - a)
    nn = (nrm * nrm).sum(axis=-1)
    with np.errstate(all="ignore"):
        h = ((p - a) * nrm).sum(axis=-1) / np.where(nn > 0, nn, 1.0)            # signed height in units of |nrm|
        f = p - nrm * h[..., None]                                             # the foot of the perpendicular
        inside = np.broadcast_to(nn > 0, h.shape).copy()
        for u, v in ((a, b), (b, c), (c, a)):
            inside &= (np.cross(v - u, f - u) * nrm).sum(axis=-1) >= 0
        plane = np.abs(h) * np.sqrt(nn)
    return np.where(inside, np.minimum(best, plane), best)


# ---- scenes the CPU and GPU tests share ----------------------------------------------------------------------------------------------
def scene_of(verts):
    """a scene of the triangles verts [n, 9] under one plain material, no lights"""
    from pbrpathtracer_amd import ptk
    verts = np.ascontiguousarray(verts, F32).reshape(-1, 9)
    n = len(verts)
    mats = np.zeros(1, ptk.MATERIAL_DTYPE)
    mats["diffuse"] = 0.7; mats["specular"] = 1.0; mats["emissive_intensity"] = 1.0; mats["roughness"] = 1.0
    mats["translucency"] = 1.0; mats["ior"] = 1.5; mats["tex"] = -1
    e1 = verts[:, 3:6].astype(np.float64) - verts[:, 0:3]; e2 = verts[:, 6:9].astype(np.float64) - verts[:, 0:3]
    nrm = np.cross(e1, e2)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), np.array([0.0, 0.0, 1.0]))
    tbn = np.concatenate([nrm, np.zeros((n, 6))], axis=1).astype(F32)
    return dict(verts=verts, normals=np.tile(nrm, (1, 3)).astype(F32), uvs=np.zeros((n, 6), F32), tbn=tbn,
                smoothing=np.zeros(n, np.uint8), material=np.zeros(n, np.int32), materials=mats, lights=np.zeros(0, np.int32))


GRID_N, GRID_STEP, GRID_HEIGHT = 48, 0.125, 0.25


def grid_mesh():
    """(verts [4608, 9], points): a 48 x 48 grid of squares of side 1/8 in the plane z = 0, two triangles each, and query points 1/4
    above every third vertex and above the midpoints of the three sides of every third square's first triangle.  Every coordinate
    is dyadic with few bits, so the rule's arithmetic is exact and the triangles that share a vertex or a side tie exactly."""
    n, s = GRID_N, GRID_STEP
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x0, y0 = (i * s).ravel(), (j * s).ravel()
    z = np.zeros_like(x0)
    P = lambda dx, dy: np.stack([x0 + dx * s, y0 + dy * s, z], axis=1)
    lower = np.concatenate([P(0, 0), P(1, 0), P(0, 1)], axis=1)
    upper = np.concatenate([P(1, 0), P(1, 1), P(0, 1)], axis=1)
    verts = np.stack([lower, upper], axis=1).reshape(-1, 9).astype(F32)
    k = np.arange(0, n + 1, 3)
    vi, vj = np.meshgrid(k, k, indexing="ij")
    above_vertices = np.stack([vi.ravel() * s, vj.ravel() * s, np.full(vi.size, GRID_HEIGHT)], axis=1)
    c = np.arange(1, n, 3)
    ci, cj = np.meshgrid(c, c, indexing="ij")
    ci, cj = ci.ravel(), cj.ravel()
    h = np.full(ci.size, GRID_HEIGHT)
    mids = [np.stack([(ci + dx) * s, (cj + dy) * s, h], axis=1) for dx, dy in ((0.5, 0.0), (0.0, 0.5), (0.5, 0.5))]
    points = np.concatenate([above_vertices] + mids).astype(F32)
    return verts, points


def far_clusters(seed=3, per_cluster=2100):
    """(verts, points): two clusters of about 1e-3 at x = +-1e3 of triangles with legs of about 1e-4, and query points inside either
    cluster, between the two and about 1e5 scene sizes away - where box and triangle arithmetic carry rounding errors far larger than
    the clusters: the geometry that found the ray walk's slack (tests/test_gpu_bvh_limits.py)"""
    rng = np.random.default_rng(seed)
    tris = []
    for cx in (1e3, -1e3):
        c = np.array([cx, 0.5 * cx, -0.25 * cx]) + rng.uniform(-5e-4, 5e-4, (per_cluster, 1, 3))
        tris.append(c + rng.normal(0.0, 1e-4, (per_cluster, 3, 3)))
    verts = np.concatenate(tris).reshape(-1, 9).astype(F32)
    centre = np.array([1e3, 0.5e3, -0.25e3])
    sign = rng.choice([-1.0, 1.0], (200, 1))
    inside = sign[:100] * centre + rng.uniform(-1e-3, 1e-3, (100, 3))
    near = sign[100:] * centre + rng.normal(0.0, 1.0, (100, 3)) * np.array([[0.03], [1.0]]).repeat(50, axis=0)
    between = rng.uniform(-1.0, 1.0, (100, 1)) * centre * 0.9 + rng.normal(0.0, 30.0, (100, 3))
    d = rng.normal(0.0, 1.0, (150, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = d * rng.uniform(0.5e8, 3e8, (150, 1))
    axis_far = np.zeros((6, 3)); axis_far[np.arange(6), np.arange(6) % 3] = np.where(np.arange(6) < 3, 2e8, -2e8)
    points = np.concatenate([inside, near, between, far, axis_far]).astype(F32)
    return verts, points


def degenerate_mix(seed=4, n=4400):
    """(verts, points): ordinary random triangles in the unit cube with every fourth one degenerate - a == b, b == c, collinear
    vertices, all three equal - enough of them for the device builder, and 1000 points: in the cube grown by 10 %, near degenerate
    triangles and on their first vertices"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, (n, 1, 3))
    t = c + rng.normal(0.0, 0.08, (n, 3, 3))
    k = np.arange(0, n, 4)
    kind = (k // 4) % 4
    t[k[kind == 0], 1] = t[k[kind == 0], 0]
    t[k[kind == 1], 2] = t[k[kind == 1], 1]
    col = k[kind == 2]
    t[col, 2] = t[col, 0] + (t[col, 1] - t[col, 0]) * rng.uniform(-1.0, 2.0, (len(col), 1))
    t[k[kind == 3], 1] = t[k[kind == 3], 0]; t[k[kind == 3], 2] = t[k[kind == 3], 0]
    verts = t.reshape(n, 9).astype(F32)
    v = verts.reshape(n, 3, 3)
    col32 = v[col, 0] + (v[col, 1] - v[col, 0]) * F32(0.5)                      # (float32 collinear up to rounding is what is wanted)
    near_deg = np.concatenate([v[k, 0], col32]) + rng.normal(0.0, 0.01, (len(k) + len(col), 3)).astype(F32)
    points = np.concatenate([rng.uniform(-0.1, 1.1, (500, 3)), near_deg[rng.choice(len(near_deg), 250, replace=False)],
                             v[rng.choice(k, 250, replace=False), 0]]).astype(F32)
    return verts, points
