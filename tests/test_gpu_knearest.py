"""K-nearest triangle queries (include/ptk.h ptk_nearest_triangles) against the numpy mirror of the rule
(tests/knearest_rule.py, which tests/test_knearest_cpu.py holds to the K smallest float64 distances), bit for bit: whatever K, the
point count, the cut of the point set, the radius, the builder, the leaf size, the "flat" option, the tile split and a refit, for
ties, full-stack trees, far points and degenerate triangles.  Every comparison is np.array_equal, with dtype and shape."""

import numpy as np
import pytest

import closest_rule as CR
import knearest_rule as KR
import ray_cases as RC
import walker_limit_cases as WC

pytestmark = pytest.mark.gpu

F32 = np.float32
NAMES = KR.NAMES
KS = (1, 2, 3, 5, 8, 13, 16)            # 1, 4, 16 are the kernel's list capacities; the others are not
CASES = ("s_cornell", "random16", "random300", "random6000")
N_POINTS = 300


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


@pytest.fixture
def tuning(ctx):
    """Builder tuning is process-wide: whatever a test sets is set back to the builders' own choices."""
    def set_(leaf_max, device_build=1):
        ctx.set_option("bvh_leaf_max", leaf_max)
        ctx.set_option("device_build", device_build)
    try:
        yield set_
    finally:
        ctx.set_option("bvh_leaf_max", 0); ctx.set_option("device_build", 1); ctx.set_option("flat", 1); ctx.set_tile(0, 1)
        ctx.set_option("contract", 0)


_cache = {}


def _radius_set(dist, seed=11):
    """max_dist uniform in [0, 2 x the median of the given distances]"""
    return np.random.default_rng(seed).uniform(0.0, 2.0 * float(np.median(dist)), len(dist)).astype(F32)


class Case:
    """a scene, its points, a radius set around the median 4th distance, and the mirror per (K, with radius), computed once each and
    not to be modified"""
    def __init__(self, arrays, pts):
        self.arrays, self.pts = arrays, np.ascontiguousarray(pts, F32)
        self.m = len(np.asarray(arrays["verts"]).reshape(-1, 9))
        self._want = {}
        d4 = self.want(4)[2]
        col = d4[:, min(3, self.m - 1)]
        self.md = _radius_set(np.where(np.isfinite(col), col, F32(1)))

    def want(self, k, radius=False, md=None):
        key = (k, radius)
        if md is not None:
            return KR.mirror(self.arrays, self.pts, k, md)
        if key not in self._want:
            ks = [k] if k not in KS else [x for x in KS if (x, radius) not in self._want]
            for x, w in zip(ks, KR.mirror_sets(self.arrays, self.pts, [(x, self.md if radius else None) for x in ks])):
                self._want[(x, radius)] = w
        return self._want[key]


def _case(case):
    if case not in _cache:
        arrays, _ = RC.scene(case)
        _cache[case] = Case(arrays, RC.rays_in_box(arrays, N_POINTS, 5)[0])
    return _cache[case]


def _built(name, make):
    if name not in _cache:
        verts, pts = make()
        _cache[name] = Case(CR.scene_of(verts), pts)
    return _cache[name]


def _check(got, want, what):
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = (g != w).reshape(len(g), -1).any(axis=1)
        assert np.array_equal(g, w), (what, name, int(bad.sum()), np.nonzero(bad)[0][:5].tolist())


def _rows(out, rows):
    return [o[rows] for o in out]


def _unused_slots_hold_the_miss_values(out):
    count, tri, dist, point, bary = out
    free = np.arange(tri.shape[1])[None] >= count[:, None]
    assert (tri[free] == -1).all() and np.isposinf(dist[free]).all() and (point[free] == 0).all() and (bary[free] == 0).all()
    assert (tri[~free] >= 0).all() and np.isfinite(dist[~free]).all()


# ---- 1. mirror equality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_equals_mirror(ctx, case):
    S = _case(case)
    ctx.upload_scene(S.arrays)
    assert ctx.upload_timing()["built_on_device"] == (case == "random6000")
    for k in KS:
        got = ctx.nearest_triangles(S.pts, k)
        _check(got, S.want(k), (case, k))
        _unused_slots_hold_the_miss_values(got)
        assert (got[0] == min(k, S.m)).all()
        got = ctx.nearest_triangles(S.pts, k, S.md)
        _check(got, S.want(k, True), (case, k, "radius"))
        _unused_slots_hold_the_miss_values(got)
    split = S.want(4, True)[0]
    assert (split == 0).any() or case == "s_cornell"
    assert (split < 4).mean() >= 0.15 and (split == 4).mean() >= 0.15, (float((split < 4).mean()), float((split == 4).mean()))
    if case == "s_cornell":                                                # 12 triangles: count < K without any radius
        assert S.m == 12 and (S.want(16)[0] == 12).all() and (S.want(13)[1][:, 12] == -1).all()
    assert ctx.last_nearest_ms() > 0


# ---- 2. K = 1 is closest_points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_k1_is_closest_points(ctx, case):
    S = _case(case)
    ctx.upload_scene(S.arrays)
    for md in (None, S.md):
        count, tri, dist, point, bary = ctx.nearest_triangles(S.pts, 1, md)
        c_tri, c_dist, c_point, c_bary = ctx.closest_points(S.pts, md)
        assert np.array_equal(tri[:, 0], c_tri) and np.array_equal(dist[:, 0], c_dist)
        assert np.array_equal(point[:, 0], c_point) and np.array_equal(bary[:, 0], c_bary)
        assert np.array_equal(count, (c_tri >= 0).astype(np.int32))
    assert (count == 0).any() and (count == 1).any()


# ---- 3. prefix property and the cross-check with overlap_spheres -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ("random300", "random6000"))
def test_prefix_property_and_overlap_cross_check(ctx, case):
    S = _case(case)
    ctx.upload_scene(S.arrays)
    for md in (None, S.md):
        full = ctx.nearest_triangles(S.pts, 16, md)
        for k in KS:
            got = ctx.nearest_triangles(S.pts, k, md)
            assert np.array_equal(got[0], np.minimum(full[0], k)), k
            for name, g, f in zip(NAMES[1:], got[1:], full[1:]):
                assert np.array_equal(g, f[:, :k]), (k, name)
    radius = S.md
    o_count, o_tris = ctx.overlap_spheres(S.pts, radius, 16)
    for k in (1, 5, 16):
        count, tri = ctx.nearest_triangles(S.pts, k, radius)[:2]
        assert np.array_equal(count, np.minimum(o_count, k)), k
        fits = o_count <= k
        assert fits.sum() >= 20
        assert np.array_equal(np.sort(np.where(tri[fits] < 0, np.iinfo(np.int32).max, tri[fits]), axis=1),
                              np.where(o_tris[fits, :k] < 0, np.iinfo(np.int32).max, o_tris[fits, :k])), k


# ---- 4. ragged sizes and cuts ------------------------------------------------------------------------------------------------------------
def test_ragged_counts_and_cuts(ctx):
    S = _case("random300")
    ctx.upload_scene(S.arrays)
    for k in (1, 5, 16):
        want, want_md = S.want(k), S.want(k, True)
        for n in (1, 63, 64, 65, 130):
            _check(ctx.nearest_triangles(S.pts[:n], k), _rows(want, slice(0, n)), (k, n))
            _check(ctx.nearest_triangles(S.pts[:n], k, S.md[:n]), _rows(want_md, slice(0, n)), (k, n, "radius"))
        for a, b in ((0, 100), (100, 300), (77, 141), (192, 193), (33, 64)):
            _check(ctx.nearest_triangles(S.pts[a:b], k, S.md[a:b]), _rows(want_md, slice(a, b)), (k, a, b))


# ---- 5. independence -----------------------------------------------------------------------------------------------------------------------
def test_independent_of_builder_leaf_size_flat_and_tiles(ctx, tuning):
    S = _case("random6000")
    for device_build in (0, 1):
        for leaf_max in (1, 8):
            tuning(leaf_max, device_build)
            ctx.upload_scene(S.arrays)
            assert ctx.upload_timing()["built_on_device"] == bool(device_build)
            for k in (1, 5, 16):
                _check(ctx.nearest_triangles(S.pts, k), S.want(k), (device_build, leaf_max, k))
                _check(ctx.nearest_triangles(S.pts, k, S.md), S.want(k, True), (device_build, leaf_max, k, "radius"))
    tuning(0, 1)
    S = _case("random16")
    ctx.upload_scene(S.arrays)
    for flat in (0, 1):
        ctx.set_option("flat", flat)
        _check(ctx.nearest_triangles(S.pts, 8), S.want(8), ("flat", flat))
    ctx.set_tile(1, 3)
    _check(ctx.nearest_triangles(S.pts, 8), S.want(8), "tile 1 of 3")
    for contract in (1, 2, 0):
        ctx.set_option("contract", contract)
        _check(ctx.nearest_triangles(S.pts, 8), S.want(8), ("contract", contract))


def test_independent_of_a_refit(ctx):
    from pbrpathtracer_amd import ptk
    S = _case("random300")
    arrays, pts = S.arrays, S.pts
    ctx.upload_scene(arrays)
    n = S.m
    a, b = n // 3, (2 * n) // 3
    verts = np.array(arrays["verts"], F32, copy=True).reshape(n, 9)
    ctx.update_geometry(a, verts[a:b])                                      # to the same positions: a refit that changes nothing
    for k in (5, 16):
        _check(ctx.nearest_triangles(pts, k), S.want(k), ("same positions", k))
    moved = dict(arrays); moved["verts"] = verts.copy()
    moved["verts"][a:b] = (verts[a:b].reshape(-1, 3, 3) + np.array([0.3, 0.15, -0.2], F32)).reshape(-1, 9)
    ctx.update_geometry(a, moved["verts"][a:b])
    fresh = ptk.Context(0)
    try:
        fresh.upload_scene(moved)
        for k in (5, 16):
            edited = ctx.nearest_triangles(pts, k)
            assert not np.array_equal(edited[1], S.want(k)[1])
            _check(edited, KR.mirror(moved, pts, k), ("after the update", k))
            _check(edited, fresh.nearest_triangles(pts, k), ("fresh upload", k))
    finally:
        fresh.close()


# ---- 6. ties ---------------------------------------------------------------------------------------------------------------------------------
def test_coincident_triangles_list_the_smaller_indices(ctx):
    tri0 = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    far = [0, 0, 9, 1, 0, 9, 0, 1, 9]
    pts = np.array([[0.25, 0.25, 1.0], [0.25, 0.25, -2.0], [0.25, 0.25, 0.0], [2.0, -1.0, 0.5], [0.5, 0.5, 0.25], [-1.0, 0.5, 0.0]], F32)
    arrays = CR.scene_of([tri0] * 5 + [far] + [tri0] * 3)
    ctx.upload_scene(arrays)
    for k, first in ((1, [0]), (3, [0, 1, 2]), (5, [0, 1, 2, 3, 4]), (8, [0, 1, 2, 3, 4, 6, 7, 8])):
        got = ctx.nearest_triangles(pts, k)
        assert (got[1] == np.array(first, np.int32)[None]).all(), k
        assert (got[2] == got[2][:, :1]).all() and got[2][:3, 0].tolist() == [1.0, 2.0, 0.0]
        _check(got, KR.mirror(arrays, pts, k), k)
    got = ctx.nearest_triangles(pts, 16)
    assert (got[0] == 9).all() and (got[1][:, 8] == 5).all() and (got[1][:, 9:] == -1).all()
    _check(got, KR.mirror(arrays, pts, 16), 16)


def test_grid_mesh_ties(ctx, tuning):
    S = _built("grid", lambda: (lambda v, p: (v, p[::4]))(*CR.grid_mesh()))
    d = S.want(16)[2]
    assert ((d == d[:, :1]).sum(axis=1) >= 2).mean() >= 0.25                # rows whose first entries tie exactly
    assert (d[:, 15] == d[:, 12]).mean() >= 0.25                            # ... and rows that are cut inside a run of ties
    for device_build, leaf_max in ((0, 1), (0, 8), (1, 4), (1, 8)):
        tuning(leaf_max, device_build)
        ctx.upload_scene(S.arrays)
        for k in (3, 16):
            _check(ctx.nearest_triangles(S.pts, k), S.want(k), (device_build, leaf_max, k))


def _nest_case():
    arrays = WC.cached("nest", WC._nest)
    return Case(arrays, WC.nest_points()[::3])


def test_full_stack_trees_keep_the_smallest_indices(ctx, tuning):
    """16 384 identical triangles behind a chain that fills the stack: the leaves arrive in tree order, the answer is by index"""
    S = _built_case("nest", _nest_case)
    want = S.want(16)
    n = len(S.pts)
    smallest = (want[1] == np.arange(20, 36, dtype=np.int32)[None]).all(axis=1)
    assert smallest.sum() >= 50, int(smallest.sum())                        # the identical triangles are the 16 nearest: indices 20 .. 35
    assert (want[2][smallest] == want[2][smallest][:, :1]).all()
    nan_odd = np.full(n, np.inf, F32); nan_odd[1::2] = np.nan
    for leaf_max in (1, 8):
        for device_build in (0, 1):
            tuning(leaf_max, device_build)
            ctx.upload_scene(S.arrays)
            assert ctx.bvh_layout()[2] == 32                                # PTK_MAX_BVH_DEPTH: these trees need the whole stack
            got = ctx.nearest_triangles(S.pts, 16)
            _check(got, want, ("nest", leaf_max, device_build))
            # live queries in the even lanes beside NaN radii in the odd ones: a list or a stack column that strayed would corrupt a neighbour
            got = ctx.nearest_triangles(S.pts, 16, nan_odd)
            _check(_rows(got, slice(0, None, 2)), _rows(want, slice(0, None, 2)), ("nest, even lanes", leaf_max, device_build))
            odd = _rows(got, slice(1, None, 2))
            assert (odd[0] == 0).all() and (odd[1] == -1).all() and np.isposinf(odd[2]).all() and (odd[3] == 0).all() and (odd[4] == 0).all()


def _built_case(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


# ---- 7. far clusters, degenerate triangles, far points ---------------------------------------------------------------------------------------
def test_far_clusters(ctx, tuning):
    S = _built("far", CR.far_clusters)
    rows = slice(0, None, 2)
    pts = S.pts[rows]
    for leaf_max, device_build in ((1, 0), (8, 0), (8, 1)):
        tuning(leaf_max, device_build)
        ctx.upload_scene(S.arrays)
        for k in (4, 16):
            _check(ctx.nearest_triangles(pts, k), _rows(S.want(k), rows), ("far clusters", leaf_max, device_build, k))
            _check(ctx.nearest_triangles(pts, k, S.md[rows]), _rows(S.want(k, True), rows), ("far clusters, radius", leaf_max, device_build, k))
    # a non-finite point affects neither its neighbours nor whether the call ends
    bad = pts.copy(); bad[7] = [np.nan, 0, 0]; bad[70] = [np.inf, 1, 2]; bad[130] = [1, -np.inf, np.nan]
    got = ctx.nearest_triangles(bad, 16)
    keep = np.ones(len(pts), bool); keep[[7, 70, 130]] = False
    _check(_rows(got, keep), _rows(_rows(S.want(16), rows), keep), "beside non-finite points")


def test_degenerate_triangles(ctx, tuning):
    S = _built("degenerate", lambda: (lambda v, p: (v, p[::3]))(*CR.degenerate_mix()))
    for device_build, leaf_max in ((0, 1), (0, 8), (1, 0), (1, 8)):
        tuning(leaf_max, device_build)
        ctx.upload_scene(S.arrays)
        for k in (4, 16):
            got = ctx.nearest_triangles(S.pts, k)
            assert (got[0] == k).all() and np.isfinite(got[2]).all() and np.isfinite(got[3]).all() and np.isfinite(got[4]).all()
            _check(got, S.want(k), (device_build, leaf_max, k))
    assert (S.want(16)[1] % 4 == 0).sum() >= 50                             # degenerate triangles are listed


@pytest.mark.parametrize("e", WC.FAR_EXPONENTS)
def test_far_points(ctx, tuning, e):
    S = _built_case(("farpoints", e), lambda: Case(CR.scene_of(WC.far_cluster(e)[0]), WC.far_points(e)[::2]))
    for leaf_max, device_build in ((1, 0), (8, 0), (8, 1)):
        tuning(leaf_max, device_build)
        ctx.upload_scene(S.arrays)
        for k in (4, 16):
            _check(ctx.nearest_triangles(S.pts, k), S.want(k), (e, leaf_max, device_build, k))


# ---- 8. special radii ------------------------------------------------------------------------------------------------------------------------
def test_special_radii(ctx):
    S = _case("random300")
    ctx.upload_scene(S.arrays)
    free = S.want(5)
    mix = S.md.copy(); mix[0] = np.nan; mix[1] = 0.0; mix[2] = -1.0; mix[3] = np.inf; mix[4] = -0.0; mix[5] = -np.inf
    got = ctx.nearest_triangles(S.pts, 5, mix)
    _check(got, S.want(5, md=mix), "mixed radii")
    none = [0, 1, 2, 4, 5]
    assert got[0][none].tolist() == [0] * 5 and (got[1][none] == -1).all() and np.isposinf(got[2][none]).all()
    assert (got[3][none] == 0).all() and (got[4][none] == 0).all()
    _check(_rows(got, slice(3, 4)), _rows(free, slice(3, 4)), "+inf")
    for bad in (np.nan, 0.0, -0.0, -1.0, -np.inf):
        g = ctx.nearest_triangles(S.pts[:70], 16, np.full(70, bad, F32))
        assert (g[0] == 0).all() and (g[1] == -1).all(), bad
    _check(ctx.nearest_triangles(S.pts, 5, np.full(len(S.pts), np.inf, F32)), free, "inf")
    # around the bound itself: max_dist = the 3rd distance and the next float up (strict in d2k < max_dist * max_dist)
    third = np.ascontiguousarray(free[2][:, 2])
    for md in (third, np.nextafter(third, F32(np.inf))):
        _check(ctx.nearest_triangles(S.pts, 5, md), S.want(5, md=md), "around the 3rd distance")


# ---- 9. the API surface ----------------------------------------------------------------------------------------------------------------------
def test_device_entries_and_caller_stream():
    import torch
    from pbrpathtracer_amd import ptk
    S = _case("random300")
    n = len(S.pts)
    dev = torch.device("cuda:0")
    c = ptk.Context(0)
    try:
        c.upload_scene(S.arrays)
        t_p, t_md = torch.from_numpy(S.pts).to(dev), torch.from_numpy(S.md).to(dev)
        torch.cuda.synchronize()
        out = c.nearest_triangles(t_p, 5)
        out_md = c.nearest_triangles(t_p, 16, t_md)
        c.synchronize()
        assert all(isinstance(o, torch.Tensor) and o.device == t_p.device for o in out + out_md)
        assert [tuple(o.shape) for o in out] == [(n,), (n, 5), (n, 5), (n, 5, 3), (n, 5, 2)]
        _check([o.cpu().numpy() for o in out], S.want(5), "device entry")
        _check([o.cpu().numpy() for o in out_md], S.want(16, True), "device entry, radius")
        for k in (1, 4, 16):
            nodes, tris = c.nearest_stats(t_p, k)
            assert nodes >= n and tris >= n * k                                # (every query fetches the root and tests at least k triangles)
        assert c.nearest_stats(t_p, 16)[1] >= c.nearest_stats(t_p, 1)[1]
        # on a caller's stream, with no host wait: the inputs are filled on that stream behind a long kernel, the result is read on it
        s = torch.cuda.Stream(device=dev)
        c.set_stream(s.cuda_stream)
        big = torch.randn(2048, 2048, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            f_p, f_md = torch.zeros_like(t_p), torch.zeros_like(t_md)
            for _ in range(8):
                big = big @ big * 1e-3
            f_p.copy_(t_p); f_md.copy_(t_md)
            res = [o.clone() for o in c.nearest_triangles(f_p, 16, f_md)]
        s.synchronize()
        _check([o.cpu().numpy() for o in res], S.want(16, True), "caller stream")
    finally:
        c.close()


def test_arguments(ctx):
    from pbrpathtracer_amd import ptk
    S = _case("s_cornell")
    L = ptk.load()
    n, K = 10, 3
    p = S.pts[:n].copy()
    want = _rows(S.want(K), slice(0, n))

    def blank():
        return (np.full(n, 77, np.int32), np.full((n, K), 77, np.int32), np.full((n, K), 7.0, F32), np.full((n, K, 3), 7.0, F32),
                np.full((n, K, 2), 7.0, F32))

    arr = blank()
    outs = tuple(a.ctypes.data for a in arr)
    none = (None,) * 5
    pp = p.ctypes.data
    BAD = -1
    fns = (L.ptk_nearest_triangles, L.ptk_nearest_triangles_device)

    def untouched():
        return all((a == (77 if a.dtype == np.int32 else 7)).all() for a in arr)

    fresh = ptk.Context(0)
    try:
        for fn in fns:
            assert fn(fresh.h, n, pp, None, K, *outs) == BAD                                # before ptk_upload_scene
    finally:
        fresh.close()
    ctx.upload_scene(S.arrays)
    for fn in fns:
        assert fn(None, n, pp, None, K, *outs) == BAD                                       # null context
        assert fn(ctx.h, -1, pp, None, K, *outs) == BAD                                     # negative count
        assert fn(ctx.h, n, None, None, K, *outs) == BAD                                    # null points
        assert fn(ctx.h, n, pp, None, K, *none) == BAD                                      # no output at all
        for k in (0, -1, 17, 1 << 20):
            assert fn(ctx.h, n, pp, None, k, *outs) == BAD, k                               # k out of range
            assert fn(ctx.h, 0, None, None, k, *outs) == BAD, k
        assert fn(ctx.h, 0, None, None, K, *none) == BAD
        assert fn(ctx.h, 0, None, None, K, *outs) == 0                                      # no points: nothing to do
    assert L.ptk_last_nearest_ms(None, None) == BAD
    assert L.ptk_nearest_stats(None, 0, None, None, 1, None, None) == BAD
    ctx.synchronize()
    assert untouched()                                                                      # a refused call leaves the outputs alone
    for bad_k in (0, 17):
        with pytest.raises(ptk.PtkError):
            ctx.nearest_triangles(p, bad_k)
    # every subset of the outputs but the empty one, through the host entry
    for m in range(1, 32):
        for a, b in zip(arr, blank()):
            a[...] = b
        sel = [o if m >> j & 1 else None for j, o in enumerate(outs)]
        assert L.ptk_nearest_triangles(ctx.h, n, pp, None, K, *sel) == 0, m
        for j, (g, w) in enumerate(zip(arr, want)):
            assert np.array_equal(g, w) if m >> j & 1 else (g == (77 if g.dtype == np.int32 else 7)).all(), (m, j)
    assert ctx.last_nearest_ms() > 0
    e = np.zeros((0, 3), F32)
    assert [x.shape for x in ctx.nearest_triangles(e, 4)] == [(0,), (0, 4), (0, 4), (0, 4, 3), (0, 4, 2)]
    # a scene without triangles: fills, without a kernel
    empty = {k: (np.asarray(v)[:0].copy() if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material") else np.asarray(v).copy())
             for k, v in S.arrays.items()}
    empty["lights"] = np.zeros(0, np.int32)
    ctx.upload_scene(empty)
    g = ctx.nearest_triangles(p, 16)
    assert (g[0] == 0).all() and (g[1] == -1).all() and np.isposinf(g[2]).all() and (g[3] == 0).all() and (g[4] == 0).all()
    _check(g, KR.mirror(empty, p, 16), "empty scene")
    assert ctx.last_nearest_ms() == 0                                                       # (no kernel ran)


def test_leaves_the_frame_state_alone(ctx):
    from pbrpathtracer_amd import ptk
    S = _case("random300")
    _, cam = RC.scene("random300")
    W, H = 40, 24
    ctx.upload_scene(S.arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, 4); ctx.set_tile(0, 1); ctx.reset()
    ctx.render_adaptive(0.05, 4, 2, 8, 3)
    ctx.render_features(ptk.FEAT_ALL, 0, 3)
    state = lambda: [ctx.read_accum(), np.array(ctx.samples()), ctx.read_sample_counts(), ctx.resolve_rgb8()] + \
        [ctx.read_feature(k) for k in range(len(ptk.FEAT_NAMES))]
    before = state()
    _check(ctx.nearest_triangles(S.pts, 8), S.want(8), "after render_adaptive")
    for b, a in zip(before, state()):
        assert np.array_equal(b, a, equal_nan=b.dtype.kind == "f")
    ctx.request_exit()                                                            # does not cut the query
    _check(ctx.nearest_triangles(S.pts, 8), S.want(8), "after request_exit")
    ctx.reset()


def test_needs_no_camera_and_no_frame():
    from pbrpathtracer_amd import ptk
    S = _case("s_cornell")
    c = ptk.Context(0)
    try:
        c.upload_scene(S.arrays)
        _check(c.nearest_triangles(S.pts, 13), S.want(13), "no camera")
        assert c.last_nearest_ms() > 0
    finally:
        c.close()


def test_host_class_transfer_and_distance_field_cli(tmp_path):
    from pbrpathtracer_amd import probes, render, scenes as S, surface
    from pbrpathtracer_amd.pathtracer import PathTracer
    pts_file, _, _ = S.build_config("C1", str(tmp_path), width=32, height=24, depth=4)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    arrays = pt.StagedScene()
    p = RC.rays_in_box(arrays, 200, 9)[0]
    want = KR.mirror(arrays, p, 5)
    _check(pt.nearest_triangles(p, 5), want, "PathTracer.nearest_triangles")      # no resolution work, no render before it
    assert pt.LastError() == ""
    md = _radius_set(want[2][:, 2], 16)
    _check(pt.nearest_triangles(p, 5, md), KR.mirror(arrays, p, 5, md), "PathTracer.nearest_triangles, radius")
    _check(pt.context().nearest_triangles(p, 5), want, "its context")
    with pytest.raises(Exception):
        pt.nearest_triangles(p, 17)
    # surface.transfer: the inverse-distance blend over the K nearest, in numpy on top of the call
    m = len(np.asarray(arrays["verts"]).reshape(-1, 9))
    values = np.random.default_rng(3).uniform(0.0, 1.0, (m, 3))
    blend = surface.transfer(pt, values, p, 4)
    count, tri, dist = KR.mirror(arrays, p, 4)[:3]
    wgt = 1.0 / np.maximum(dist.astype(np.float64), 1e-30) ** 2
    wgt = wgt * (tri >= 0)
    exp = (values[np.maximum(tri, 0)] * wgt[..., None]).sum(axis=1) / wgt.sum(axis=1, keepdims=True)
    assert blend.shape == (len(p), 3) and np.allclose(blend, exp, rtol=1e-12, atol=0)
    assert np.array_equal(surface.transfer(pt, values[:, 0], p, 1), values[:, 0][tri[:, 0]])          # K = 1: the nearest triangle's value
    on = np.asarray(arrays["verts"], F32).reshape(-1, 3, 3)[7].mean(axis=0, dtype=np.float64).astype(F32)[None]
    one = KR.mirror(arrays, on, 4)
    if one[2][0, 0] == 0:                                                         # a point on the surface takes that triangle's value
        assert np.array_equal(surface.transfer(pt, values, on, 4)[0], values[one[1][0, 0]])
    # a pending geometry edit applies, as for RenderFrame()
    M = np.eye(4, dtype=F32); M[3][0] = 0.05
    pt.SetObjectTransform(0, M)
    moved = pt.StagedScene()
    assert not np.array_equal(moved["verts"], arrays["verts"])
    _check(pt.nearest_triangles(p, 5), KR.mirror(moved, p, 5), "after SetObjectTransform")
    pt.close()
    # the CLI on a 4 x 4 x 4 grid: tri / dist with a trailing K axis
    npz = str(tmp_path / "field.npz")
    assert render.main([pts_file, "--distance-field", "4", "4", "4", "--nearest", "3", "-o", npz]) == 0
    z = np.load(npz)
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    origin, spacing = probes.grid_over_bounds(v.min(axis=0), v.max(axis=0), (4, 4, 4))
    pos = probes.grid_positions((4, 4, 4), origin, spacing)
    w = KR.mirror(arrays, pos, 3)
    assert z["tri"].shape == (4, 4, 4, 3) and z["dist"].shape == (4, 4, 4, 3) and z["count"].shape == (4, 4, 4)
    assert np.array_equal(z["tri"], w[1].reshape(4, 4, 4, 3)) and np.array_equal(z["dist"], w[2].reshape(4, 4, 4, 3))
    assert np.array_equal(z["count"], w[0].reshape(4, 4, 4))
    assert np.array_equal(z["origin"], origin) and np.array_equal(z["spacing"], spacing)
    assert render.main([pts_file, "--distance-field", "4", "4", "4", "--nearest", "17", "-o", npz]) == 1
    assert render.main([pts_file, "--nearest", "3", "-o", npz]) == 1                # --nearest goes with --distance-field
