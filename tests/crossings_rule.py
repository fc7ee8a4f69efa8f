"""numpy mirror of the crossing rule (include/ptk.h ptk_crossings_rays, ptk_contains_points, ptk_signed_distance):
Moeller-Trumbore operation by operation in float32 over EVERY triangle of a scene - no tree -, with e1, e2 computed from
arrays["verts"] as float32 differences (the record packers' subtractions); the votes, the majority and the sign flip.  Helper of
tests/test_crossings_cpu.py, which holds it to the float64 solid-angle winding number, and of tests/test_gpu_crossings.py, which
holds the kernels to it bit for bit.  Also the small closed meshes those two share."""
import functools

import numpy as np

F32 = np.float32
EPS = F32(0.00001)
WINDING, PARITY = 0, 1            # PTK_INSIDE_WINDING, PTK_INSIDE_PARITY


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - by * az, az * bx - bz * ax, ax * by - bx * ay


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def per_triangle(verts, ro, rd):
    """Moeller-Trumbore of every (ray, triangle) pair as tri_test computes it: (a, u, v, t), float32 [n, m] each"""
    tr = np.asarray(verts, F32).reshape(-1, 3, 3)
    v0 = tr[:, 0]; e1 = tr[:, 1] - tr[:, 0]; e2 = tr[:, 2] - tr[:, 0]
    ro = np.asarray(ro, F32).reshape(-1, 1, 3); rd = np.asarray(rd, F32).reshape(-1, 1, 3)
    ox, oy, oz = ro[..., 0], ro[..., 1], ro[..., 2]
    dx, dy, dz = rd[..., 0], rd[..., 1], rd[..., 2]
    v0x, v0y, v0z = v0[None, :, 0], v0[None, :, 1], v0[None, :, 2]
    e1x, e1y, e1z = e1[None, :, 0], e1[None, :, 1], e1[None, :, 2]
    e2x, e2y, e2z = e2[None, :, 0], e2[None, :, 1], e2[None, :, 2]
    with np.errstate(all="ignore"):
        hx, hy, hz = _cross(dx, dy, dz, e2x, e2y, e2z)
        a = _dot(e1x, e1y, e1z, hx, hy, hz)
        f = F32(1.0) / a
        sx, sy, sz = ox - v0x, oy - v0y, oz - v0z
        u = f * _dot(sx, sy, sz, hx, hy, hz)
        qx, qy, qz = _cross(sx, sy, sz, e1x, e1y, e1z)
        v = f * _dot(dx, dy, dz, qx, qy, qz)
        t = f * _dot(e2x, e2y, e2z, qx, qy, qz)
    assert a.dtype == F32 and u.dtype == F32 and v.dtype == F32 and t.dtype == F32
    return a, u, v, t


def crossing_masks(verts, ro, rd, tmax):
    """(front, back) bool [n, m]: the triangles each ray crosses, by the sign of a; tmax float32 [n]"""
    a, u, v, t = per_triangle(verts, ro, rd)
    with np.errstate(all="ignore"):
        ok = ~(np.abs(a) < EPS) & ~(u < 0) & ~(v < 0) & ~(u + v > F32(1.0)) & (t > EPS) & (t < np.asarray(tmax, F32).reshape(-1, 1))
        return ok & (a > 0), ok & (a < 0)


def _tmax(tmax, n):
    return np.full(n, np.inf, F32) if tmax is None else np.ascontiguousarray(tmax, F32).reshape(n)


def crossings(arrays, ro, rd, tmax=None, budget=1 << 22):
    """(front [n] int32, back [n] int32): what ptk_crossings_rays must return.  tmax None: +inf for every ray"""
    ro = np.ascontiguousarray(ro, F32).reshape(-1, 3); rd = np.ascontiguousarray(rd, F32).reshape(-1, 3)
    n = len(ro)
    verts = np.asarray(arrays["verts"], F32).reshape(-1, 9)
    front = np.zeros(n, np.int32); back = np.zeros(n, np.int32)
    if n == 0 or len(verts) == 0:
        return front, back
    tm = _tmax(tmax, n)
    chunk = max(1, budget // len(verts))
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        fr, bk = crossing_masks(verts, ro[s:e], rd[s:e], tm[s:e])
        front[s:e] = fr.sum(axis=1); back[s:e] = bk.sum(axis=1)
    return front, back


def check_dirs(num_dirs, mode):
    """the refusals of ptk_contains_points that depend on D and the mode alone"""
    if not (1 <= num_dirs <= 31) or num_dirs % 2 == 0:
        raise ValueError("num_dirs must be odd and in 1 .. 31")
    if mode not in (WINDING, PARITY):
        raise ValueError("unknown mode")


def votes(front, back, mode):
    """the vote of each (point, direction): bool, the shape of front"""
    front = np.asarray(front, np.int32); back = np.asarray(back, np.int32)
    return back != front if mode == WINDING else ((front + back) & 1).astype(bool)


def contains(arrays, points, dirs, mode=WINDING):
    """(inside [n] uint8, winding [n, D] int32): what ptk_contains_points must return for the directions dirs [D, 3]"""
    points = np.ascontiguousarray(points, F32).reshape(-1, 3)
    dirs = np.ascontiguousarray(dirs, F32).reshape(-1, 3)
    D, n = len(dirs), len(points)
    check_dirs(D, mode)
    winding = np.zeros((n, D), np.int32); count = np.zeros(n, np.int32)
    for j in range(D):
        front, back = crossings(arrays, points, np.broadcast_to(dirs[j], (n, 3)))
        winding[:, j] = back - front
        count += votes(front, back, mode)
    return (2 * count > D).astype(np.uint8), winding


def flip_sign(dist, inside):
    """dist with its sign bit set where inside (+inf becomes -inf)"""
    bits = np.ascontiguousarray(dist, F32).view(np.uint32).copy()
    bits[np.asarray(inside).astype(bool)] |= np.uint32(0x80000000)
    return bits.view(F32)


def signed_distance(arrays, points, dirs, mode=WINDING, max_dist=None):
    """(tri, dist, point, bary): closest_rule's answer with the sign of dist from contains()"""
    import closest_rule as CR
    tri, dist, point, bary = CR.mirror(arrays, points, max_dist)
    return tri, flip_sign(dist, contains(arrays, points, dirs, mode)[0]), point, bary


# ---- the float64 reference: the solid-angle winding number ---------------------------------------------------------------------------
def winding_number64(verts, points, chunk=512):
    """[n] float64: the sum over the triangles of the signed solid angle seen from each point (Van Oosterom and Strackee), over
    4 pi: +-1 inside a closed mesh wound one way, 0 outside"""
    t = np.asarray(verts, np.float64).reshape(1, -1, 3, 3)
    p = np.asarray(points, np.float64).reshape(-1, 1, 1, 3)
    out = np.zeros(len(p))
    for s in range(0, len(p), chunk):
        r = t - p[s:s + chunk]
        a, b, c = r[:, :, 0], r[:, :, 1], r[:, :, 2]
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        det = (a * np.cross(b, c)).sum(axis=-1)
        den = la * lb * lc + (a * b).sum(axis=-1) * lc + (b * c).sum(axis=-1) * la + (c * a).sum(axis=-1) * lb
        out[s:s + chunk] = (2.0 * np.arctan2(det, den)).sum(axis=1) / (4.0 * np.pi)
    return out


# ---- the small closed meshes ---------------------------------------------------------------------------------------------------------
def _tris(v, f):
    return np.asarray(v, np.float64)[np.asarray(f)].reshape(-1, 9).astype(F32)


def cube(flipped=False):
    """[12, 9]: the cube [-1, 1]^3, two triangles per face, wound outward - or all of them the other way"""
    v = [[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    if flipped:
        f = [(a, c, b) for a, b, c in f]
    return _tris(v, f)


def icosphere(levels=2):
    """[20 x 4^levels, 9]: an icosahedron subdivided `levels` times, the vertices on the unit sphere"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [tuple(np.asarray(x) / np.linalg.norm(x)) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid = {}

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = (np.asarray(v[i]) + np.asarray(v[j])) / 2.0
                v.append(tuple(x / np.linalg.norm(x)))
                mid[key] = len(v) - 1
            return mid[key]
        f = [t for a, b, c in f for ab, bc, ca in [(m(a, b), m(b, c), m(c, a))] for t in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))]
    return _tris(v, f)


def torus(nu=16, nv=8, R=1.0, r=0.4):
    """[2 nu nv, 9]: a torus about the z axis, nu segments around it, nv around the tube"""
    u = 2.0 * np.pi * np.arange(nu) / nu; w = 2.0 * np.pi * np.arange(nv) / nv
    v = [((R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)) for a in u for b in w]
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            f += [(a, b, c), (a, c, d)]
    return _tris(v, f)


MESHES = ("cube", "cube flipped", "icosphere", "torus")


@functools.lru_cache(maxsize=None)
def mesh(name):
    """verts [m, 9] float32 of one of MESHES; shared, not to be modified"""
    return {"cube": cube, "cube flipped": lambda: cube(True), "icosphere": icosphere, "torus": torus}[name]()


def mesh_points(verts, n=4096, seed=7, lattice=9, pad=0.25):
    """float32 [n + lattice^3, 3]: n points uniform in the mesh's bounds enlarged by 20 % and a lattice over the bounds padded by
    `pad`"""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng(seed)
    uniform = rng.uniform(mid - 1.2 * half, mid + 1.2 * half, (n, 3))
    axes = [np.linspace(lo[k] - pad, hi[k] + pad, lattice) for k in range(3)]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.concatenate([uniform, grid]).astype(F32)


# ---- rays whose count no tree can promise ----------------------------------------------------------------------------------------------
def off_box(verts, ro, rd, tmax=None, budget=1 << 22):
    """bool [n]: rays one of whose crossings lies off its own triangle's box by more than the walk's slack (Walk::begin: 2^-21 x
    (max |ro| + scene bound) per axis) - walker_limit_cases._off_box for EVERY crossing, not only the nearest.  Moeller-Trumbore's
    acceptance error grows as 1 / cos of the incidence angle: a ray from 10^6 triangle sizes away that grazes a triangle's plane
    can "cross" it tens of triangle sizes off the triangle, where no box of the tree has to be.  From the rule alone."""
    verts = np.asarray(verts, F32).reshape(-1, 9)
    ro = np.ascontiguousarray(ro, F32).reshape(-1, 3); rd = np.ascontiguousarray(rd, F32).reshape(-1, 3)
    n = len(ro)
    out = np.zeros(n, bool)
    if n == 0 or len(verts) == 0:
        return out
    tm = _tmax(tmax, n)
    t3 = verts.reshape(-1, 3, 3).astype(np.float64)
    lo, hi = t3.min(axis=1), t3.max(axis=1)
    vmax = float(np.abs(verts).max())
    chunk = max(1, budget // len(verts))
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        a, u, v, t = per_triangle(verts, ro[s:e], rd[s:e])
        fr, bk = crossing_masks(verts, ro[s:e], rd[s:e], tm[s:e])
        i, k = np.nonzero(fr | bk)
        p = ro[s:e][i].astype(np.float64) + t[i, k].astype(np.float64)[:, None] * rd[s:e][i].astype(np.float64)
        slack = (np.abs(ro[s:e][i]).max(axis=1).astype(np.float64) + 3.1 * (1.01 * vmax + 1e-3)) * 2.0 ** -21
        off = np.maximum(lo[k] - p, p - hi[k]).max(axis=1)
        out[s + i[off > slack]] = True
    return out
