"""Overlap queries (include/ptk.h ptk_overlap_boxes, ptk_overlap_spheres) against the numpy mirror of the two rules
(tests/overlap_rule.py, which tests/test_overlap_cpu.py holds to float64 computations), bit for bit: whatever k, tri_from, the query
count, the cut of the query set, the builder, the leaf size, the "flat" option and the tile split, for touching boxes, coincident
and degenerate triangles, far geometry, trees that fill the traversal stack and edited geometry.  Every comparison is
np.array_equal, with dtype and shape."""

import numpy as np
import pytest

import closest_rule as CR
import overlap_rule as OR
import ray_cases as RC
import walker_limit_cases as WC

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = ("boxes", "spheres")
KS = (0, 1, 4, 5, 16)
SCENES = ("s_cornell", "random16", "random300", "random6000") + OR.GENERATED


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


class Queries:
    """a scene with a query set of either shape and the mirror's accepted matrix, from which any (k, tri_from) answer follows"""

    def __init__(self, arrays, lo, hi, spheres=None):
        self.arrays = arrays
        self.m = len(np.asarray(arrays["verts"]).reshape(-1, 9))
        self.q = {"boxes": (np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32)), "spheres": spheres if spheres is not None else OR.spheres_of(lo, hi)}
        self._acc = {}

    def acc(self, shape):
        if shape not in self._acc:
            fn = OR.accepted_boxes if shape == "boxes" else OR.accepted_spheres
            self._acc[shape] = fn(self.arrays["verts"], *self.q[shape])
        return self._acc[shape]

    def want(self, shape, k, tri_from=None, rows=slice(None)):
        return OR.answer(self.acc(shape)[rows], k, None if tri_from is None else tri_from)

    def ask(self, c, shape, k, tri_from=None, rows=slice(None)):
        a, b = self.q[shape]
        fn = c.overlap_boxes if shape == "boxes" else c.overlap_spheres
        return fn(a[rows], b[rows], k, tri_from)


_cache = {}


def _scene(name):
    """Queries of a parity case or of a generated scene; computed once, not to be modified"""
    if name not in _cache:
        if isinstance(name, tuple):
            verts, lo, hi = OR.generated(*name)
            _cache[name] = Queries(CR.scene_of(verts), lo, hi)
        else:
            arrays, _ = RC.scene(name)
            _cache[name] = Queries(arrays, *OR.boxes_in_bounds(arrays, 1000 if name == "random300" else 400, 7))
    return _cache[name]


def _built(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def _check(got, want, what):
    for name, g, w in zip(("count", "tris"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        assert np.array_equal(g, w), (what, name, len(bad), bad[:5].tolist())


def _tri_from(n, m, seed=5):
    return np.random.default_rng(seed).integers(-3, max(m, 1), n).astype(np.int32)


def _raw(c, shape, a, b, tri_from, k, want_count, want_tris):
    """the host entry through ctypes with only the outputs asked for; the others stay sentinel-filled"""
    from pbrpathtracer_amd import ptk
    n = len(a)
    count = np.full(n, 77, np.int32); tris = np.full((n, max(k, 1)), 77, np.int32)
    fn = ptk.load().ptk_overlap_boxes if shape == "boxes" else ptk.load().ptk_overlap_spheres
    rc = fn(c.h, n, a.ctypes.data, b.ctypes.data, tri_from.ctypes.data if tri_from is not None else None, k,
            count.ctypes.data if want_count else None, tris.ctypes.data if want_tris else None)
    return rc, count, tris


# ---- 1. mirror equality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES, ids=str)
def test_equals_mirror(ctx, name):
    S = _scene(name)
    n = len(S.q["boxes"][0])
    ctx.upload_scene(S.arrays)
    tf = _tri_from(n, S.m)
    beyond = np.full(n, S.m, np.int32)
    for shape in SHAPES:
        for k in KS:
            _check(S.ask(ctx, shape, k), S.want(shape, k), (name, shape, k))
            _check(S.ask(ctx, shape, k, tf), S.want(shape, k, tf), (name, shape, k, "tri_from"))
        got = S.ask(ctx, shape, 4, beyond)
        assert (got[0] == 0).all() and (got[1] == -1).all()
        _check(got, S.want(shape, 4, beyond), (name, shape, "beyond the scene"))
        # each output alone
        a, b = S.q[shape]
        rc, count, tris = _raw(ctx, shape, a, b, tf, 5, True, False)
        assert rc != 0 and (count == 77).all()                              # k > 0 needs tris
        rc, count, tris = _raw(ctx, shape, a, b, tf, 5, False, True)
        assert rc == 0 and (count == 77).all() and np.array_equal(tris, S.want(shape, 5, tf)[1])
        rc, count, tris = _raw(ctx, shape, a, b, tf, 0, True, True)
        assert rc == 0 and np.array_equal(count, S.want(shape, 0, tf)[0]) and (tris == 77).all()
        assert ctx.last_overlap_ms() > 0
        assert (S.acc(shape).sum(axis=1) > 0).any()
    per = S.acc("boxes").sum(axis=1)
    if name == OR.GENERATED[0]:
        for k in (4, 16):
            assert (per > k).any() and (per < k).any() and (per == 0).any()


# ---- 2. ragged counts and cuts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_ragged_counts_and_cuts(ctx, shape):
    S = _scene("random300")
    n = len(S.q[shape][0])
    assert n == 1000
    ctx.upload_scene(S.arrays)
    tf = _tri_from(n, S.m)
    for cnt in (1, 63, 64, 65, 1000):
        rows = slice(0, cnt)
        for k in (0, 5, 16):
            _check(S.ask(ctx, shape, k, tf[rows], rows), S.want(shape, k, tf[rows], rows), (shape, cnt, k))
    whole = S.ask(ctx, shape, 5, tf)
    for a, b in ((0, 300), (300, 1000), (77, 141), (640, 641)):
        _check(S.ask(ctx, shape, 5, tf[a:b], slice(a, b)), [w[a:b] for w in whole], (shape, a, b))


# ---- 3. independence -------------------------------------------------------------------------------------------------------------------
def test_independent_of_builder_leaf_size_flat_tiles_and_contract(ctx, tuning):
    S = _scene("random6000")
    n = len(S.q["boxes"][0])
    tf = _tri_from(n, S.m)
    for device_build in (0, 1):
        for leaf_max in (1, 8):
            tuning(leaf_max, device_build)
            ctx.upload_scene(S.arrays)
            assert ctx.upload_timing()["built_on_device"] == bool(device_build)
            for shape in SHAPES:
                _check(S.ask(ctx, shape, 16), S.want(shape, 16), (shape, device_build, leaf_max))
                _check(S.ask(ctx, shape, 4, tf), S.want(shape, 4, tf), (shape, device_build, leaf_max, "tri_from"))
    tuning(0, 1)
    S = _scene("random16")
    ctx.upload_scene(S.arrays)
    for shape in SHAPES:
        want = S.want(shape, 16)
        for flat in (0, 1):
            ctx.set_option("flat", flat)
            _check(S.ask(ctx, shape, 16), want, (shape, "flat", flat))
        ctx.set_tile(1, 3)
        _check(S.ask(ctx, shape, 16), want, (shape, "tile 1 of 3"))
        ctx.set_tile(0, 1)
        for contract in (1, 2, 0):
            ctx.set_option("contract", contract)
            _check(S.ask(ctx, shape, 16), want, (shape, "contract", contract))


# ---- 4. limit geometry -------------------------------------------------------------------------------------------------------------------
def _grid_queries():
    verts, pts = CR.grid_mesh()
    lo, hi = OR.grid_boxes()
    # and flat boxes and spheres around the query points of the closest tests: above the plane, touching it, through it
    half = np.array([CR.GRID_STEP, CR.GRID_STEP, CR.GRID_HEIGHT], F32)
    return Queries(CR.scene_of(verts), np.concatenate([lo, pts - half]), np.concatenate([hi, pts + half]),
                   (pts, np.resize(np.array([CR.GRID_HEIGHT, CR.GRID_HEIGHT * 0.5, CR.GRID_HEIGHT * 1.5, 0.28125], F32), len(pts))))


def test_grid_mesh_with_faces_on_grid_lines(ctx, tuning):
    S = _built("grid", _grid_queries)
    nb = len(OR.grid_boxes()[0])
    assert np.array_equal(S.acc("boxes")[:nb], OR.grid_expected(*OR.grid_boxes()))
    at = S.acc("spheres")[0::4].sum(axis=1)
    assert (at == 0).all()                                                  # radius = the height itself: strict, nothing
    for device_build in (0, 1):
        for leaf_max in (1, 8):
            tuning(leaf_max, device_build)
            ctx.upload_scene(S.arrays)
            for shape in SHAPES:
                _check(S.ask(ctx, shape, 16), S.want(shape, 16), (shape, device_build, leaf_max))
                _check(S.ask(ctx, shape, 0), S.want(shape, 0), (shape, device_build, leaf_max, "count"))
    got = S.ask(ctx, "boxes", 16)
    assert got[0][:nb].tolist() == [7, 16, 38, 70, 7, 0, 4608, 22] and got[1][6].tolist() == list(range(16))


def test_coincident_triangles_each_count(ctx):
    tri0 = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    arrays = CR.scene_of([tri0, [5, 5, 5, 6, 5, 5, 5, 6, 5], tri0, tri0])
    ctx.upload_scene(arrays)
    lo = np.array([[0.2, 0.2, -1], [0.2, 0.2, 0], [1, 1, 0], [0.5, 0.5, 0], [4, 4, 4], [-1, -1, -1]], F32)
    hi = np.array([[0.3, 0.3, 1], [0.2, 0.2, 0], [2, 2, 1], [2, 2, 1], [7, 7, 7], [9, 9, 9]], F32)
    count, tris = ctx.overlap_boxes(lo, hi, 4)
    assert count.tolist() == [3, 3, 0, 3, 1, 4]
    assert tris.tolist() == [[0, 2, 3, -1], [0, 2, 3, -1], [-1] * 4, [0, 2, 3, -1], [1, -1, -1, -1], [0, 1, 2, 3]]
    _check((count, tris), OR.mirror_boxes(arrays, lo, hi, 4), "coincident")
    count, tris = ctx.overlap_boxes(lo, hi, 2, np.array([1, 2, 0, 3, 2, -7], np.int32))
    assert count.tolist() == [2, 2, 0, 1, 0, 4] and tris.tolist() == [[2, 3], [2, 3], [-1, -1], [3, -1], [-1, -1], [0, 1]]
    c = np.array([[0.25, 0.25, 0.5], [0.25, 0.25, 0.5], [5, 5, 5.25]], F32); r = np.array([0.5, 0.75, 0.5], F32)
    count, tris = ctx.overlap_spheres(c, r, 4)
    assert count.tolist() == [0, 3, 1] and tris.tolist() == [[-1] * 4, [0, 2, 3, -1], [1, -1, -1, -1]]


def _degenerate_queries():
    verts, pts = CR.degenerate_mix()
    half = np.random.default_rng(8).uniform(0.005, 0.1, (len(pts), 3))
    return Queries(CR.scene_of(verts), (pts - half).astype(F32), (pts + half).astype(F32))


def test_degenerate_triangles(ctx, tuning):
    S = _built("degenerate", _degenerate_queries)
    assert S.m >= 4096 and S.acc("boxes")[:, ::4].sum() >= 50
    for device_build, leaf_max in ((0, 0), (0, 1), (1, 0), (1, 8)):
        tuning(leaf_max, device_build)
        ctx.upload_scene(S.arrays)
        assert ctx.upload_timing()["built_on_device"] == bool(device_build), (device_build, leaf_max)
        for shape in SHAPES:
            _check(S.ask(ctx, shape, 16), S.want(shape, 16), (shape, device_build, leaf_max))


def _far_queries():
    verts, pts = CR.far_clusters()
    # boxes and spheres of a few triangle legs around the near points, of the distance itself and more around the far ones
    d = CR.mirror(CR.scene_of(verts), pts)[1].astype(np.float64)
    half = np.where(np.arange(len(pts)) % 2 == 0, np.maximum(d * 1.5, 3e-4), 3e-4)[:, None] * np.ones((1, 3))
    p = pts.astype(np.float64)
    return Queries(CR.scene_of(verts), (p - half).astype(F32), (p + half).astype(F32), (pts, half[:, 0].astype(F32)))


def test_far_clusters_and_non_finite_queries(ctx, tuning):
    S = _built("far", _far_queries)
    assert (S.acc("boxes").sum(axis=1) > 0).sum() >= 150 and (S.acc("spheres").sum(axis=1) > 0).sum() >= 150
    for leaf_max in (1, 8):
        for device_build in (0, 1):
            tuning(leaf_max, device_build)
            ctx.upload_scene(S.arrays)
            for shape in SHAPES:
                _check(S.ask(ctx, shape, 16), S.want(shape, 16), (shape, leaf_max, device_build))
    # a non-finite query affects neither its neighbours nor whether the call ends
    keep = np.ones(len(S.q["boxes"][0]), bool); keep[[7, 70, 130]] = False
    lo, hi = (x.copy() for x in S.q["boxes"])
    lo[7] = -np.inf; hi[7] = np.inf; hi[70, 1] = np.inf; lo[130] = [-np.inf, 0, 0]; hi[130] = [0, np.inf, 3e38]
    got = ctx.overlap_boxes(lo, hi, 16)
    _check([g[keep] for g in got], [w[keep] for w in S.want("boxes", 16)], "beside non-finite boxes")
    c, r = (x.copy() for x in S.q["spheres"])
    c[7] = [np.nan, 0, 0]; c[70] = [np.inf, 1, 2]; c[130] = [1, -np.inf, np.nan]
    got = ctx.overlap_spheres(c, r, 16)
    _check([g[keep] for g in got], [w[keep] for w in S.want("spheres", 16)], "beside non-finite spheres")


def _far_domain_queries(e):
    verts = WC.far_cluster(e)[0]
    pts = WC.far_points(e).astype(np.float64)
    leg = 2.0 ** (e - 17)
    half = np.random.default_rng(e).uniform(0.5 * leg, 4.0 * leg, (len(pts), 3))
    return Queries(CR.scene_of(verts), (pts - half).astype(F32), (pts + half).astype(F32), (pts.astype(F32), half[:, 0].astype(F32)))


@pytest.mark.parametrize("e", WC.FAR_EXPONENTS)
def test_far_domain(ctx, tuning, e):
    S = _built(("far", e), lambda: _far_domain_queries(e))
    assert (S.acc("boxes").sum(axis=1) > 0).sum() >= 50 and (S.acc("boxes").sum(axis=1) == 0).sum() >= 50
    for leaf_max, device_build in ((1, 0), (8, 0), (8, 1)):
        tuning(leaf_max, device_build)
        ctx.upload_scene(S.arrays)
        for shape in SHAPES:
            _check(S.ask(ctx, shape, 16), S.want(shape, 16), (e, shape, leaf_max, device_build))


def _nest_queries():
    arrays = WC.cached("nest", WC._nest)
    pts = WC.nest_points().astype(np.float64)
    half = np.random.default_rng(2).uniform(0.02, 0.6, (len(pts), 3)) * np.maximum(1.0, np.abs(pts[:, :1]) * 0.05)
    return Queries(arrays, (pts - half).astype(F32), (pts + half).astype(F32))


def test_full_stack_trees(ctx, tuning):
    S = _built("nest", _nest_queries)
    per = S.acc("boxes").sum(axis=1)
    assert (per >= 16384).sum() >= 50 and (per == 0).sum() >= 50
    lo, hi = S.q["boxes"]
    for leaf_max in (1, 8):
        for device_build in (0, 1):
            tuning(leaf_max, device_build)
            ctx.upload_scene(S.arrays)
            assert ctx.bvh_layout()[2] == 32                                # PTK_MAX_BVH_DEPTH: these trees need the whole stack
            _check(S.ask(ctx, "boxes", 16), S.want("boxes", 16), ("nest", leaf_max, device_build))
            # live queries in the even lanes beside reversed boxes in the odd ones: a column that spilled would corrupt a neighbour
            rl, rh = lo.copy(), hi.copy()
            rl[1::2], rh[1::2] = hi[1::2], lo[1::2]
            count, tris = ctx.overlap_boxes(rl, rh, 16)
            want = S.want("boxes", 16)
            assert np.array_equal(count[0::2], want[0][0::2]) and np.array_equal(tris[0::2], want[1][0::2]), (leaf_max, device_build)
            assert (count[1::2] == 0).all() and (tris[1::2] == -1).all()
    tuning(8, 1)
    ctx.upload_scene(S.arrays)
    rows = slice(0, 600, 3)
    _check(S.ask(ctx, "spheres", 4, None, rows), S.want("spheres", 4, None, rows), "nest spheres")


# ---- 5. radii and boxes ----------------------------------------------------------------------------------------------------------------
def test_special_radii_and_boxes(ctx):
    S = _scene("random300")
    ctx.upload_scene(S.arrays)
    c, r = (x[:400].copy() for x in S.q["spheres"])
    r[0] = np.nan; r[1] = 0.0; r[2] = -1.0; r[3] = np.inf; r[4] = -0.0; r[5] = -np.inf
    got = ctx.overlap_spheres(c, r, 16)
    _check(got, OR.mirror_spheres(S.arrays, c, r, 16), "mixed radii")
    assert got[0][[0, 1, 2, 4, 5]].tolist() == [0] * 5 and (got[1][[0, 1, 2, 4, 5]] == -1).all()
    assert got[0][3] == S.m and got[1][3].tolist() == list(range(16))
    lo, hi = (x[:400].copy() for x in S.q["boxes"])
    lo[0], hi[0] = hi[0].copy(), lo[0].copy()                               # reversed on every axis
    lo[1, 1], hi[1, 1] = hi[1, 1], lo[1, 1]                                 # ... on one
    lo[2, 0] = np.nan; hi[3, 2] = np.nan; lo[4] = np.nan; hi[4] = np.nan
    v = np.asarray(S.arrays["verts"], np.float64).reshape(-1, 3)
    lo[5], hi[5] = v.min(axis=0) - 1, v.max(axis=0) + 1                      # the box around the whole scene
    a = np.asarray(S.arrays["verts"], F32).reshape(-1, 9)[17, :3]
    lo[6] = a; hi[6] = a                                                    # a point box on a first vertex
    got = ctx.overlap_boxes(lo, hi, 16)
    _check(got, OR.mirror_boxes(S.arrays, lo, hi, 16), "special boxes")
    assert got[0][:5].tolist() == [0] * 5 and (got[1][:5] == -1).all()
    assert got[0][5] == S.m and got[1][5].tolist() == list(range(16))
    assert 17 in got[1][6].tolist()


# ---- 6. state and entry points ---------------------------------------------------------------------------------------------------------
def test_geometry_edits_are_seen(ctx):
    from pbrpathtracer_amd import ptk
    S = _scene("random300")
    arrays = S.arrays
    ctx.upload_scene(arrays)
    rows = slice(0, 400)
    for shape in SHAPES:
        _check(S.ask(ctx, shape, 16, None, rows), S.want(shape, 16, None, rows), (shape, "before"))
    n = S.m
    a, b = n // 3, (2 * n) // 3
    moved = dict(arrays); moved["verts"] = np.array(arrays["verts"], F32, copy=True).reshape(n, 9)
    moved["verts"][a:b] = (moved["verts"][a:b].reshape(-1, 3, 3) + np.array([0.3, 0.15, -0.2], F32)).reshape(-1, 9)
    ctx.update_geometry(a, moved["verts"][a:b])
    fresh = ptk.Context(0)
    try:
        fresh.upload_scene(moved)
        for shape in SHAPES:
            qa, qb = (x[rows] for x in S.q[shape])
            edited = S.ask(ctx, shape, 16, None, rows)
            assert not np.array_equal(edited[0], S.want(shape, 16, None, rows)[0])
            mirror = (OR.mirror_boxes if shape == "boxes" else OR.mirror_spheres)(moved, qa, qb, 16)
            _check(edited, mirror, (shape, "after the update"))
            _check(edited, S.ask(fresh, shape, 16, None, rows), (shape, "fresh upload"))
    finally:
        fresh.close()


def test_leaves_the_frame_state_alone(ctx):
    from pbrpathtracer_amd import ptk
    S = _scene("random300")
    _, cam = RC.scene("random300")
    W, H = 40, 24
    ctx.upload_scene(S.arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, 4); ctx.set_tile(0, 1); ctx.reset()
    ctx.render_adaptive(0.05, 4, 2, 8, 3)
    ctx.render_features(ptk.FEAT_ALL, 0, 3)
    state = lambda: [ctx.read_accum(), np.array(ctx.samples()), ctx.read_sample_counts(), ctx.resolve_rgb8()] + \
        [ctx.read_feature(k) for k in range(len(ptk.FEAT_NAMES))]
    before = state()
    for shape in SHAPES:
        _check(S.ask(ctx, shape, 5), S.want(shape, 5), (shape, "after render_adaptive"))
    for b, a in zip(before, state()):
        assert np.array_equal(b, a, equal_nan=b.dtype.kind == "f")
    ctx.request_exit()                                                            # does not cut the query
    for shape in SHAPES:
        _check(S.ask(ctx, shape, 5), S.want(shape, 5), (shape, "after request_exit"))
    ctx.reset()


def test_device_entries_and_caller_stream():
    import torch
    from pbrpathtracer_amd import ptk
    S = _scene("random300")
    n = len(S.q["boxes"][0])
    tf = _tri_from(n, S.m)
    dev = torch.device("cuda:0")
    c = ptk.Context(0)
    try:
        c.upload_scene(S.arrays)
        t_tf = torch.from_numpy(tf).to(dev)
        for shape in SHAPES:
            t_a, t_b = (torch.from_numpy(x).to(dev) for x in S.q[shape])
            torch.cuda.synchronize()
            fn = c.overlap_boxes if shape == "boxes" else c.overlap_spheres
            out = fn(t_a, t_b, 16)
            out_tf = fn(t_a, t_b, 5, t_tf)
            out_0 = fn(t_a, t_b, 0)
            c.synchronize()
            assert all(isinstance(o, torch.Tensor) and o.device == t_a.device for o in out + out_tf + out_0)
            assert [tuple(o.shape) for o in out] == [(n,), (n, 16)] and tuple(out_0[1].shape) == (n, 0)
            _check([o.cpu().numpy() for o in out], S.want(shape, 16), (shape, "device entry"))
            _check([o.cpu().numpy() for o in out_tf], S.want(shape, 5, tf), (shape, "device entry, tri_from"))
            _check([o.cpu().numpy() for o in out_0], S.want(shape, 0), (shape, "device entry, count only"))
            nodes, tris, accepted, past = c.overlap_stats(ptk.OVERLAP_BOX if shape == "boxes" else ptk.OVERLAP_SPHERE, t_a, t_b)
            assert accepted == int(S.acc(shape).sum()) and tris >= accepted and nodes >= 1
            assert (past >= accepted and past <= tris) if shape == "boxes" else past == 0
            # on a caller's stream, with no host wait: the inputs are filled on that stream behind a long kernel
            s = torch.cuda.Stream(device=dev)
            c.set_stream(s.cuda_stream)
            big = torch.randn(2048, 2048, device=dev)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                f_a, f_b, f_tf = torch.zeros_like(t_a), torch.zeros_like(t_b), torch.zeros_like(t_tf)
                for _ in range(8):
                    big = big @ big * 1e-3
                f_a.copy_(t_a); f_b.copy_(t_b); f_tf.copy_(t_tf)
                res = [o.clone() for o in fn(f_a, f_b, 5, f_tf)]
            s.synchronize()
            _check([o.cpu().numpy() for o in res], S.want(shape, 5, tf), (shape, "caller stream"))
            c.set_stream(0)
    finally:
        c.close()


def test_arguments(ctx):
    from pbrpathtracer_amd import ptk
    S = _scene("s_cornell")
    L = ptk.load()
    n, k = 10, 4
    BAD = -1
    count = np.full(n, 77, np.int32); tris = np.full((n, k), 77, np.int32)
    pc, pt = count.ctypes.data, tris.ctypes.data
    fresh = ptk.Context(0)
    for shape, fns in (("boxes", (L.ptk_overlap_boxes, L.ptk_overlap_boxes_device)), ("spheres", (L.ptk_overlap_spheres, L.ptk_overlap_spheres_device))):
        a, b = (np.ascontiguousarray(x[:n]) for x in S.q[shape])
        pa, pb = a.ctypes.data, b.ctypes.data
        for fn in fns:
            assert fn(fresh.h, n, pa, pb, None, k, pc, pt) == BAD                                # before ptk_upload_scene
        ctx.upload_scene(S.arrays)
        for fn in fns:
            assert fn(None, n, pa, pb, None, k, pc, pt) == BAD                                   # null context
            assert fn(ctx.h, -1, pa, pb, None, k, pc, pt) == BAD                                 # negative count
            assert fn(ctx.h, n, None, pb, None, k, pc, pt) == BAD                                # null inputs
            assert fn(ctx.h, n, pa, None, None, k, pc, pt) == BAD
            assert fn(ctx.h, n, pa, pb, None, -1, pc, pt) == BAD                                 # k outside 0 .. 16
            assert fn(ctx.h, n, pa, pb, None, 17, pc, pt) == BAD
            assert fn(ctx.h, n, pa, pb, None, k, pc, None) == BAD                                # k > 0 without tris
            assert fn(ctx.h, n, pa, pb, None, 0, None, pt) == BAD                                # k == 0 without count
            assert fn(ctx.h, 0, None, None, None, 0, None, None) == BAD
            assert fn(ctx.h, 0, None, None, None, k, pc, pt) == 0                                # no queries: nothing to do
        ctx.synchronize()
        assert (count == 77).all() and (tris == 77).all()                                        # a refused call leaves the outputs alone
        assert fns[0](ctx.h, n, pa, pb, None, k, None, pt) == 0                                  # tris alone
        assert (count == 77).all() and np.array_equal(tris, S.want(shape, k, None, slice(0, n))[1])
        tris[:] = 77
        assert fns[0](ctx.h, n, pa, pb, None, 0, pc, None) == 0                                  # count alone
        assert (tris == 77).all() and np.array_equal(count, S.want(shape, 0, None, slice(0, n))[0])
        count[:] = 77
        with pytest.raises(ptk.PtkError):
            S.ask(ctx, shape, 17)
    fresh.close()
    assert L.ptk_last_overlap_ms(None, None) == BAD
    assert ctx.last_overlap_ms() > 0
    e = np.zeros((0, 3), F32)
    assert [x.shape for x in ctx.overlap_boxes(e, e, 3)] == [(0,), (0, 3)]
    # a scene without triangles: zeros and -1s, by fills
    arrays = S.arrays
    empty = {k_: (np.asarray(v)[:0].copy() if k_ in ("verts", "normals", "uvs", "tbn", "smoothing", "material") else np.asarray(v).copy())
             for k_, v in arrays.items()}
    empty["lights"] = np.zeros(0, np.int32)
    ctx.upload_scene(empty)
    for shape in SHAPES:
        a, b = (x[:n] for x in S.q[shape])
        got = (ctx.overlap_boxes if shape == "boxes" else ctx.overlap_spheres)(a, b, 3)
        assert got[0].tolist() == [0] * n and (got[1] == -1).all() and got[1].shape == (n, 3)
    assert ctx.last_overlap_ms() == 0                                                            # (no kernel ran)


# ---- 7. cross-checks and worked uses ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("random300", "random6000"))
def test_sphere_finds_exactly_what_closest_points_finds(ctx, case):
    from pbrpathtracer_amd import overlap
    S = _scene(case)
    ctx.upload_scene(S.arrays)
    n = 100 if case == "random6000" else 400                                # (spheres there hold hundreds of triangles: many pages each)
    c, r = (x[:n] for x in S.q["spheres"])
    tri = ctx.closest_points(c, r)[0]
    offsets, indices = overlap.all_in_spheres(ctx, c, r)
    count = np.diff(offsets)
    assert np.array_equal(count > 0, tri >= 0) and 0.05 <= (tri >= 0).mean() <= 0.95
    want = OR.csr(S.acc("spheres")[:n])
    assert np.array_equal(offsets, want[0]) and np.array_equal(indices, want[1])
    hit = np.nonzero(tri >= 0)[0]
    assert S.acc("spheres")[hit, tri[hit]].all()                            # closest_points' triangle is in the list (the lists are the mirror's)


def test_all_in_boxes_and_voxel_occupancy(ctx):
    from pbrpathtracer_amd import overlap, probes
    S = _scene(OR.GENERATED[1])
    ctx.upload_scene(S.arrays)
    lo, hi = S.q["boxes"]
    offsets, indices = overlap.all_in_boxes(ctx, lo, hi)
    want = OR.csr(S.acc("boxes"))
    assert offsets.dtype == np.int64 and indices.dtype == np.int32 and np.diff(offsets).max() > 3 * 16
    assert np.array_equal(offsets, want[0]) and np.array_equal(indices, want[1])
    v = np.asarray(S.arrays["verts"], np.float64).reshape(-1, 3)
    dims = (9, 8, 7)
    origin, spacing = probes.grid_over_bounds(v.min(axis=0), v.max(axis=0), dims)
    occ = overlap.voxel_occupancy(ctx, origin, spacing, dims)
    vlo, vhi, centres = overlap.voxel_boxes(origin, spacing, dims)
    mirror = OR.accepted_boxes(S.arrays["verts"], vlo, vhi).any(axis=1).reshape(7, 8, 9)
    assert occ.dtype == bool and occ.shape == (7, 8, 9) and np.array_equal(occ, mirror) and 0 < occ.sum() < occ.size
    solid = overlap.voxel_occupancy(ctx, origin, spacing, dims, solid=True)
    assert np.array_equal(solid, mirror | (ctx.contains_points(centres) != 0).reshape(7, 8, 9))


def test_host_class_and_voxelize_cli(tmp_path):
    from pbrpathtracer_amd import overlap, probes, render, scenes as Sc
    from pbrpathtracer_amd.pathtracer import PathTracer
    pts_file, _, _ = Sc.build_config("C1", str(tmp_path), width=32, height=24, depth=4)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    arrays = pt.StagedScene()
    lo, hi = OR.boxes_in_bounds(arrays, 200, 9)
    c, r = OR.spheres_of(lo, hi)
    tf = _tri_from(200, len(arrays["verts"]))
    _check(pt.overlap_boxes(lo, hi, 16), OR.mirror_boxes(arrays, lo, hi, 16), "PathTracer.overlap_boxes")     # no resolution work, no render
    assert pt.LastError() == ""
    _check(pt.overlap_boxes(lo, hi, 3, tf), OR.mirror_boxes(arrays, lo, hi, 3, tf), "PathTracer.overlap_boxes, tri_from")
    _check(pt.overlap_spheres(c, r, 5), OR.mirror_spheres(arrays, c, r, 5), "PathTracer.overlap_spheres")
    _check(pt.context().overlap_boxes(lo, hi, 0), OR.mirror_boxes(arrays, lo, hi, 0), "its context")
    with pytest.raises(Exception):
        pt.overlap_boxes(lo, hi, 17)
    # a pending geometry edit applies, as for RenderFrame(): object 0 staged again under another matrix ([column][row])
    M = np.eye(4, dtype=F32); M[3][0] = 0.05
    pt.SetObjectTransform(0, M)
    moved = pt.StagedScene()
    assert not np.array_equal(moved["verts"], arrays["verts"])
    _check(pt.overlap_boxes(lo, hi, 16), OR.mirror_boxes(moved, lo, hi, 16), "after SetObjectTransform")
    pt.close()
    # the CLI on a 5 x 4 x 3 grid against the mirror of the same voxels
    for solid in (False, True):
        npz = str(tmp_path / ("solid.npz" if solid else "grid.npz"))
        assert render.main([pts_file, "--voxelize", "5", "4", "3"] + (["--solid"] if solid else []) + ["-o", npz]) == 0
        z = np.load(npz)
        assert sorted(z.files) == ["occupancy", "origin", "spacing"]
        v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
        origin, spacing = probes.grid_over_bounds(v.min(axis=0), v.max(axis=0), (5, 4, 3))
        assert np.array_equal(z["origin"], origin) and np.array_equal(z["spacing"], spacing)
        vlo, vhi, centres = overlap.voxel_boxes(origin, spacing, (5, 4, 3))
        surface = OR.accepted_boxes(arrays["verts"], vlo, vhi).any(axis=1).reshape(3, 4, 5)
        occ = z["occupancy"]
        assert occ.dtype == bool and occ.shape == (3, 4, 5)
        if not solid:
            assert np.array_equal(occ, surface) and occ.any()
        else:
            pt = PathTracer(0)
            pt.LoadSceneFile(pts_file)
            assert np.array_equal(occ, surface | (pt.contains_points(centres) != 0).reshape(3, 4, 5))
            pt.close()
    assert render.main([pts_file, "--solid", "-o", str(tmp_path / "x.png")]) == 1
