"""Helper of tests/test_gpu_bvh_limits.py, tests/test_gpu_walker_limits.py and tests/test_walker_limits_cpu.py - no tests of its
own: the scenes, rays and points that take a BVH walker to the trees' limits.  The nest (a tree whose traversal stack is full),
tools/soak_bvh.py's adversarial kinds, clusters at 2^20 .. 2^59 with rays from up to 2^22 triangle legs away, and for the
closest-point queries point sets on the same scenes.  Everything is seeded and drawn in float64, then cast once to float32."""
import functools

import numpy as np

from test_gpu_bvh_build import _scene, _soup          # noqa: F401  (_soup: for the importers)
from test_gpu_random_scenes import random_scene       # noqa: F401


def _glow(arrays, lights):
    """material 1 for the triangles `lights`: an emitter, so that a render of the scene is not black"""
    mats = np.concatenate([arrays["materials"], arrays["materials"]])
    mats[1]["emissive"] = (1.0, 0.8, 0.6); mats[1]["emissive_intensity"] = 4.0
    arrays["materials"] = mats
    arrays["material"] = arrays["material"].copy(); arrays["material"][lights] = 1
    arrays["lights"] = np.asarray(lights, np.int32)
    return arrays


def _aimed_rays(verts, m, seed, spread=1.5):
    rng = np.random.default_rng(seed)
    n = len(verts)
    ext = float(np.abs(verts).max())
    ro = (rng.uniform(-spread, spread, (m, 3)) * ext).astype(np.float32)
    tgt = verts.reshape(n, 3, 3)[rng.integers(0, n, m)].mean(axis=1)
    rd = tgt - ro
    rd /= np.maximum(np.linalg.norm(rd, axis=1, keepdims=True), 1e-30)
    rd = rd.astype(np.float32)
    rd[::23, 2] = 0.0
    return ro, rd


# ---- a traversal stack filled to its bound -----------------------------------------------------------------------------

_YZ = np.array([[-0.9, 1.1], [1.1, 1.1], [1.1, -0.9]])


def _nest(k=20, r=1.5, m=16384):
    """k triangles growing by r along +x and, at the near end, m identical ones.  Every triangle's box straddles the x axis and
    no triangle reaches it, so a ray along the axis enters every box and hits nothing: its walk defers whatever the tree lets
    it.  The big triangles glow (material 1) so that a render through the nest is not black."""
    s = r ** np.arange(1, k + 1)
    v = np.zeros((k + m, 3, 3))
    v[:k, :, 0] = 2 * s[:, None] + np.array([0.0, 0.5, 1.0]) * s[:, None]
    v[:k, :, 1:] = _YZ[None] * s[:, None, None]
    v[k:, :, 0] = np.array([0.0, 0.5, 1.0])
    v[k:, :, 1:] = _YZ[None]
    return _glow(_scene(v.astype(np.float32).reshape(-1, 9)), np.arange(k))


def nest_rays():
    """(ro, rd) [256, 3] float32: 128 rays along the nest's axis that miss everything, then 128 that hit the big triangles"""
    rng = np.random.default_rng(5)
    m = 256
    ro = np.zeros((m, 3)); ro[:, 0] = -1.0; ro[:, 1:] = rng.uniform(-0.05, 0.05, (m, 2))
    rd = np.zeros((m, 3)); rd[:, 0] = 1.0; rd[:, 1:] = rng.uniform(-1e-7, 1e-7, (m, 2))
    ro[m // 2:, 1:] = rng.uniform(-3.0, 3.0, (m - m // 2, 2))                  # and rays that hit the big triangles
    rd[m // 2:, 1:] = rng.uniform(-0.05, 0.05, (m - m // 2, 2))
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    return ro.astype(np.float32), rd.astype(np.float32)


# one trivial query behind each set: a ray from far outside that points away, and a point that is given a zero radius
NEST_TRIVIAL_RAY = (np.array([[-3e4, 2e4, 1e4]], np.float32), np.array([[-1.0, 0.0, 0.0]], np.float32))
NEST_TRIVIAL_POINT = np.array([[0.5, 0.1, 0.1]], np.float32)
NEST_CAMERA = dict(pos=np.array([-1.0, 0.0, 0.0], np.float32), dir=np.array([1.0, 0.0, 0.0], np.float32), up=np.array([0.0, 0.0, 1.0], np.float32),
                   focal=0.05, fovy=20.0, focal_dist=3.0, aperture=0.0)


def nest_points():
    """[600, 3] float32: 200 points in the box of the identical triangles (inside every box of the chain that leads to them: the
    closest-point walk defers every sibling on the way down), 200 along the axis the big triangles straddle, 200 around the near end"""
    rng = np.random.default_rng(1)
    inside = rng.uniform([0.0, -0.9, -0.9], [1.0, 1.1, 1.1], (200, 3))
    axis = np.concatenate([rng.uniform(-1.0, 7000.0, (200, 1)), rng.uniform(-0.05, 0.05, (200, 2))], axis=1)
    around = rng.uniform(-2.0, 2.0, (200, 3))
    return np.concatenate([inside, axis, around]).astype(np.float32)


# ---- adversarial geometry ----------------------------------------------------------------------------------------------

def _onion(n=60000, seed=5):
    """a soup scaled by 0.9995^i: boxes nest around the origin"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (n, 1, 3)) + 0.05 * rng.uniform(-1, 1, (n, 3, 3))
    return _glow(_scene((v * (0.9995 ** np.arange(n))[:, None, None]).astype(np.float32).reshape(n, 9)), np.arange(0, 200, 7))


SOAK_KINDS = ["line", "plane grid", "duplicates", "big coordinates", "slivers", "huge and tiny"]
SOAK_SEEDS = {k: 100 + i for i, k in enumerate(SOAK_KINDS)}


def _soak_scene(kind, seed):
    """tools/soak_bvh.py's adversarial kinds"""
    rng = np.random.default_rng(seed)
    n = int(rng.choice([4096, 5000, 12345]))
    c = rng.uniform(-1, 1, (n, 1, 3)); size = 0.02
    if kind == "line": c = c * np.array([1.0, 0.0, 0.0]) + np.array([0.0, 0.3, -0.2])
    elif kind == "plane grid":
        g = int(np.ceil(np.sqrt(n))); ij = np.stack(np.meshgrid(np.arange(g), np.arange(g)), -1).reshape(-1, 2)[:n]
        c = np.concatenate([ij / g * 2 - 1, np.zeros((n, 1))], axis=1)[:, None, :]
    elif kind == "big coordinates": c = c * 1e15; size = 1e13
    v = c + size * rng.uniform(-1, 1, (n, 3, 3))
    if kind == "huge and tiny": v[: n // 50] = c[: n // 50] + 1.5 * rng.uniform(-1, 1, (n // 50, 3, 3))
    if kind == "duplicates": v[n // 2:] = v[: n - n // 2]
    if kind == "slivers": v[:, 2] = v[:, 0] + (v[:, 1] - v[:, 0]) * rng.uniform(0, 1, (n, 1)) + 1e-7 * rng.normal(0, 1, (n, 3))
    return v.astype(np.float32).reshape(n, 9)


def soak_points(kind, verts, seed):
    """[800, 3] float32: the 400 ray origins of _aimed_rays(verts, 400, seed), 200 points on triangles (random barycentrics of
    random triangles, rounded to float32) and 200 points at N(0, size) around those - so that every kind's ties and degenerate
    triangles are on the winning side of a query, not only in its way"""
    rng = np.random.default_rng(seed + 1000)
    n = len(verts)
    size = 1e13 if kind == "big coordinates" else 0.02
    t = verts.reshape(n, 3, 3)[rng.integers(0, n, 200)].astype(np.float64)
    w = rng.dirichlet((1.0, 1.0, 1.0), 200)
    on = (t * w[:, :, None]).sum(axis=1)
    near = on + rng.normal(0.0, size, (200, 3))
    return np.concatenate([_aimed_rays(verts, 400, seed)[0].astype(np.float64), on, near]).astype(np.float32)


# ---- the far domain ----------------------------------------------------------------------------------------------------

TINY = [0.0, -0.0, 1e-40, 1e-30, 1e-19, 1e-17]           # the 1 / d clamp at +-1e18 engages below 1e-18, not above
FAR_EXPONENTS = (20, 40, 59)


def _off_box(verts, ro, rd, ref):
    """Rays whose brute-force hit lies off its own triangle's box by more than the walk's slack (Walk::begin: 2^-21 x (max |ro| +
    scene bound) per axis).  Moeller-Trumbore's acceptance error grows as 1 / cos of the incidence angle: a ray from 10^6 triangle
    sizes away that grazes a triangle's plane can be "hit" tens of triangle sizes off the triangle.  No box slack covers that, so
    for these rays the closest hit is not tree-independent - the oracle's own tree disagrees with its brute force too."""
    tri, tuv = ref
    h = np.nonzero(tri >= 0)[0]
    p = ro[h].astype(np.float64) + tuv[h, :1].astype(np.float64) * rd[h].astype(np.float64)
    t3 = verts[tri[h]].reshape(-1, 3, 3).astype(np.float64)
    vmax = float(np.abs(verts).max())
    slack = (np.abs(ro[h]).max(axis=1).astype(np.float64) + 3.1 * (1.01 * vmax + 1e-3)) * 2.0 ** -21
    off = np.maximum(t3.min(axis=1) - p, p - t3.max(axis=1)).max(axis=1)
    out = np.zeros(len(ro), bool)
    out[h] = off > slack
    return out


@functools.lru_cache(maxsize=None)
def far_case(e):
    """(shared, not to be modified) dict of a cluster of 4096 turned right isosceles triangles of legs 2^-17 x 2^e around 2^e x (1, -0.5, 0.25): verts [4096, 9],
    its 600 rays ro, rd (the first half from up to 2^22 legs away, the second half near enough for finite products), their
    distances dist and targets tgt (float64), the leg"""
    rng = np.random.default_rng(e)
    off = 2.0 ** e
    n = 4096
    c = rng.uniform(-1, 1, (n, 1, 3)) * 2.0 ** -12 * off + off * np.array([1.0, -0.5, 0.25])
    rot = np.linalg.qr(rng.normal(0, 1, (n, 3, 3)))[0]                          # a right isosceles triangle of legs 2^-17 x offset, turned
    v = c + 2.0 ** -17 * off * np.einsum("kj,nij->nki", np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), rot)
    if e == 59:
        v[0] = np.array([[2.0 ** 61 - 2.0 ** 37, 0, 0], [2.0 ** 60, 2.0 ** 58, 0], [2.0 ** 60, 0, 2.0 ** 58]])   # the largest accepted value
    verts = v.astype(np.float32).reshape(n, 9)
    e1 = verts[:, 3:6].astype(np.float64) - verts[:, 0:3]
    assert (np.linalg.norm(e1, axis=1)[1:] >= 2.0 ** -20 * off).all()
    m = 2 * 6 * 50
    tgt = verts.reshape(n, 3, 3)[rng.integers(1, n, m)].astype(np.float64).mean(axis=1)
    d = rng.normal(0, 1, (m, 3))
    axis = rng.integers(0, 3, m)
    tiny = np.tile(TINY, m // len(TINY)) * np.where((np.arange(m) // len(TINY)) % 2 == 0, 1.0, -1.0)
    d[np.arange(m), axis] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[np.arange(m), axis] = tiny
    leg = 2.0 ** -17 * off
    # far: up to 2^60 away, or 2^22 triangle legs; near: close enough that Moeller-Trumbore's products (legs^2 x distance) stay
    # finite - at 2^59 the far rays' products overflow and every one of them misses, in the reference's arithmetic as here
    far = np.minimum(2.0 ** 60 - np.abs(tgt).max(axis=1), 2.0 ** 22 * leg)
    dist = np.concatenate([far[: m // 2], np.minimum(far[m // 2:], 2.0 ** 118 / leg ** 2)]) * rng.uniform(0.5, 1.0, m)
    ro = (tgt - dist[:, None] * d).astype(np.float32)
    rd = d.astype(np.float32)
    assert (np.abs(ro) <= 2.0 ** 60).all()
    assert rd[np.arange(m), axis].tolist() == np.float32(tiny).tolist() and (np.signbit(rd[np.arange(m), axis]) == np.signbit(tiny)).all()
    return dict(verts=verts, ro=ro, rd=rd, dist=dist, tgt=tgt, leg=leg)


def far_cluster(e):
    """(verts, ro, rd) of far_case(e)"""
    c = far_case(e)
    return c["verts"], c["ro"], c["rd"]


def far_points(e):
    """[300, 3] float32: the first 150 ray origins of far_case(e) (up to 2^22 legs from the cluster) and 150 points at those rays'
    targets + N(0, 4 legs)"""
    c = far_case(e)
    rng = np.random.default_rng(e + 1000)
    near = c["tgt"][:150] + rng.normal(0.0, 4.0 * c["leg"], (150, 3))
    return np.concatenate([c["ro"][:150].astype(np.float64), near]).astype(np.float32)


# ---- references, computed once and shared by the tests of a run (not to be modified) -----------------------------------------

SEED, SAMPLE = (1 << 40) + 9, 3          # of the hit queries' opacity draws (they count on the textured scene only)
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def hits_reference(oracle_mod, key, arrays, ro, rd):
    """hit_rule.mirror of the rays at (SEED, SAMPLE, key_base 0): (tri, t, bary, material), every triangle, no tree"""
    import hit_rule as HR
    return cached(("hits", key), lambda: HR.mirror(oracle_mod, arrays, ro, rd, HR.ray_keys(SEED, 0, len(ro), SAMPLE)))


def occlusion_bounds(t, seed=11):
    """[(label, tmax)] for ptk_occluded_rays around the mirror's t: none, t itself (strict: not occluded), the next float up, a seeded
    uniform set, and tests/test_gpu_hits.py test_occlusion's mixture of NaN / inf / 0 / t with it"""
    hit = t < np.inf
    scale = float(np.median(t[hit])) if hit.any() else 1.0          # (no ray of "big coordinates" or "slivers" hits anything)
    uniform = np.random.default_rng(seed).uniform(0.0, 2.0 * scale, len(t)).astype(np.float32)
    mix = uniform.copy(); mix[0::5] = np.nan; mix[1::5] = np.inf; mix[2::5] = 0.0; mix[3::5] = t[3::5]
    return [("no bound", None), ("t", t), ("above t", np.nextafter(t, np.float32(np.inf))), ("uniform", uniform), ("mixture", mix)]


def closest_reference(key, arrays, pts, seed=11):
    """[(label, max_dist, (tri, dist, point, bary))] of closest_rule's mirror: without a radius, with max_dist = the distance (strict:
    a miss), the next float up, and a seeded uniform set"""
    import closest_rule as CR

    def make():
        free = CR.mirror_radii(arrays, pts, [None])[0]
        dist = free["dist"]
        uniform = np.random.default_rng(seed).uniform(0.0, 2.0 * float(np.median(dist)), len(pts)).astype(np.float32)
        radii = [dist, np.nextafter(dist, np.float32(np.inf)), uniform]
        rest = CR.mirror_radii(arrays, pts, radii)
        four = lambda m: (m["tri"], m["dist"], m["point"], m["bary"])
        return [("no radius", None, four(free))] + [(lb, md, four(m)) for lb, md, m in zip(("dist", "above dist", "uniform"), radii, rest)]
    return cached(("closest", key), make)
