"""Closest-point queries (include/ptk.h ptk_closest_points) against the numpy mirror of the rule
(tests/closest_rule.py, which tests/test_closest_cpu.py holds to a float64 computation), bit for bit: whatever the point count, the
cut of the point set, the radius, the builder, the leaf size, the "flat" option and the tile split, for ties, far points,
degenerate triangles and edited geometry.  Every comparison is np.array_equal, with dtype and shape."""

import numpy as np
import pytest

import closest_rule as CR
import ray_cases as RC

pytestmark = pytest.mark.gpu

F32 = np.float32
NAMES = ("tri", "dist", "point", "bary")


def n_points(case):
    return 400 if case == "random6000" else 1000


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


_mirror = {}


def _case(case):
    """(arrays, points, (tri, dist, point, bary) of the mirror) of a case; computed once, not to be modified"""
    if case not in _mirror:
        arrays, _ = RC.scene(case)
        pts = RC.rays_in_box(arrays, n_points(case), 5)[0]
        _mirror[case] = (arrays, pts, CR.mirror(arrays, pts))
    return _mirror[case]


def _built(name, make):
    """(arrays, points, mirror) of one of closest_rule's scenes; computed once, not to be modified"""
    if name not in _mirror:
        verts, pts = make()
        arrays = CR.scene_of(verts)
        _mirror[name] = (arrays, pts, CR.mirror(arrays, pts))
    return _mirror[name]


def _check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, w), (what, name, int((g != w).reshape(len(g), -1).any(axis=1).sum()),
                                      np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0][:5].tolist())


def _radius_set(dist, n, seed=11):
    return np.random.default_rng(seed).uniform(0.0, 2.0 * float(np.median(dist)), n).astype(F32)


def _raw(ctx, pts, md, which):
    """the host entry through ctypes with only the outputs `which` (a set of names) requested"""
    from pbrpathtracer_amd import ptk
    n = len(pts)
    out = dict(tri=np.full(n, 77, np.int32), dist=np.full(n, 7.0, F32), point=np.full((n, 3), 7.0, F32), bary=np.full((n, 2), 7.0, F32))
    p = np.ascontiguousarray(pts, F32)
    rc = ptk.load().ptk_closest_points(ctx.h, n, p.ctypes.data, md.ctypes.data if md is not None else None,
                                       *(out[k].ctypes.data if k in which else None for k in NAMES))
    return rc, out


# ---- 1. mirror equality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("s_cornell", "random16", "random300", "random6000"))
def test_equals_mirror(ctx, case):
    arrays, pts, want = _case(case)
    ctx.upload_scene(arrays)
    assert ctx.upload_timing()["built_on_device"] == (case == "random6000")
    _check(ctx.closest_points(pts), want, case)
    assert (want[0] >= 0).all()
    for k, name in enumerate(NAMES):                                        # each output requested alone
        rc, out = _raw(ctx, pts, None, {name})
        assert rc == 0
        for j, other in enumerate(NAMES):
            if j == k:
                assert np.array_equal(out[other], want[j]), (case, name)
            else:
                assert (out[other] == (77 if other == "tri" else 7)).all(), (case, name, other)
    assert ctx.last_closest_ms() > 0


# ---- 2. radius -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("random16", "random300", "random6000"))
def test_radius(ctx, case):
    arrays, pts, free = _case(case)
    n = len(pts)
    ctx.upload_scene(arrays)
    md = _radius_set(free[1], n)
    want = CR.mirror(arrays, pts, md)
    _check(ctx.closest_points(pts, md), want, case)
    assert 0.15 <= (want[0] >= 0).mean() <= 0.85
    # around the bound itself: max_dist = the distance and the next float up (strict in d2k < max_dist * max_dist)
    _check(ctx.closest_points(pts, free[1]), CR.mirror(arrays, pts, free[1]), case + " at dist")
    up = np.nextafter(free[1], F32(np.inf))
    _check(ctx.closest_points(pts, up), CR.mirror(arrays, pts, up), case + " above dist")
    # one query each with NaN, 0, negative and +inf, among ordinary radii
    mix = md.copy(); mix[0] = np.nan; mix[1] = 0.0; mix[2] = -1.0; mix[3] = np.inf; mix[4] = -0.0; mix[5] = -np.inf
    got = ctx.closest_points(pts, mix)
    _check(got, CR.mirror(arrays, pts, mix), case + " mixed")
    assert got[0][[0, 1, 2, 4, 5]].tolist() == [-1] * 5 and np.isposinf(got[1][[0, 1, 2, 4, 5]]).all()
    assert (got[2][[0, 1, 2, 4, 5]] == 0).all() and (got[3][[0, 1, 2, 4, 5]] == 0).all()
    assert got[0][3] == free[0][3] and got[1][3] == free[1][3]
    for bad in (np.nan, 0.0, -1.0):
        assert (ctx.closest_points(pts[:70], np.full(70, bad, F32))[0] == -1).all(), bad
    _check(ctx.closest_points(pts, np.full(n, np.inf, F32)), free, case + " inf")


# ---- 3. ragged counts and cuts ---------------------------------------------------------------------------------------------------------
def test_ragged_counts_and_cuts(ctx):
    arrays, pts, want = _case("random300")
    ctx.upload_scene(arrays)
    md = _radius_set(want[1], len(pts))
    want_md = CR.mirror(arrays, pts, md)
    for n in (1, 63, 64, 65, 129):
        _check(ctx.closest_points(pts[:n]), [w[:n] for w in want], n)
        _check(ctx.closest_points(pts[:n], md[:n]), [w[:n] for w in want_md], n)
    whole = ctx.closest_points(pts, md)
    for a, b in ((0, 300), (300, 1000), (77, 141), (640, 641)):
        _check(ctx.closest_points(pts[a:b], md[a:b]), [w[a:b] for w in whole], (a, b))


# ---- 4. independence -------------------------------------------------------------------------------------------------------------------
def test_independent_of_builder_leaf_size_flat_and_tiles(ctx, tuning):
    arrays, pts, want = _case("random6000")
    md = _radius_set(want[1], len(pts))
    want_md = CR.mirror(arrays, pts, md)
    for device_build in (0, 1):
        for leaf_max in (1, 8):
            tuning(leaf_max, device_build)
            ctx.upload_scene(arrays)
            assert ctx.upload_timing()["built_on_device"] == bool(device_build)
            _check(ctx.closest_points(pts), want, (device_build, leaf_max))
            _check(ctx.closest_points(pts, md), want_md, (device_build, leaf_max, "radius"))
    tuning(0, 1)
    arrays, pts, want = _case("random16")
    ctx.upload_scene(arrays)
    for flat in (0, 1):
        ctx.set_option("flat", flat)
        _check(ctx.closest_points(pts), want, ("flat", flat))
    ctx.set_tile(1, 3)
    _check(ctx.closest_points(pts), want, "tile 1 of 3")
    for contract in (1, 2, 0):
        ctx.set_option("contract", contract)
        _check(ctx.closest_points(pts), want, ("contract", contract))


# ---- 5. ties ---------------------------------------------------------------------------------------------------------------------------
def test_coincident_triangles_give_the_smaller_index(ctx):
    tri0 = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    pts = np.array([[0.25, 0.25, 1.0], [0.25, 0.25, -2.0], [0.25, 0.25, 0.0], [2.0, -1.0, 0.5], [0.5, 0.5, 0.25], [-1.0, 0.5, 0.0]], F32)
    full, _ = RC.scene("s_cornell")
    for order in ((0, 1), (1, 0)):                                          # two distinct materials, in either upload order
        arrays = CR.scene_of([tri0, tri0])
        arrays["materials"] = np.asarray(full["materials"])[:2].copy()
        arrays["material"] = np.array(order, np.int32)
        ctx.upload_scene(arrays)
        tri, dist, point, bary = ctx.closest_points(pts)
        assert tri.tolist() == [0] * len(pts), order
        assert dist[:3].tolist() == [1.0, 2.0, 0.0] and np.array_equal(point[0], [0.25, 0.25, 0.0]) and np.array_equal(bary[0], [0.25, 0.25])
        _check((tri, dist, point, bary), CR.mirror(arrays, pts), order)
    # the second one alone is triangle 1 once the first moves away
    ctx.upload_scene(CR.scene_of([[0, 0, 9, 1, 0, 9, 0, 1, 9], tri0]))
    assert ctx.closest_points(pts[:1])[0].tolist() == [1]


def test_grid_mesh_ties(ctx, tuning):
    arrays, pts, want = _built("grid", CR.grid_mesh)
    for device_build in (0, 1):
        for leaf_max in (1, 4, 8):
            tuning(leaf_max, device_build)
            ctx.upload_scene(arrays)
            # (with one triangle per leaf the device builder hands this mesh to the host builder: the tree it makes of a regular
            # planar grid would defer more than the traversal stack holds)
            assert ctx.upload_timing()["built_on_device"] == bool(device_build and leaf_max != 1)
            _check(ctx.closest_points(pts), want, (device_build, leaf_max))


# ---- 6. far clusters and far points ----------------------------------------------------------------------------------------------------
def test_far_clusters_and_far_points(ctx, tuning):
    arrays, pts, want = _built("far", CR.far_clusters)
    md = np.where(np.arange(len(pts)) % 2 == 0, want[1] * F32(1.5), want[1] * F32(0.75)).astype(F32)
    want_md = CR.mirror(arrays, pts, md)
    for leaf_max in (1, 8):
        for device_build in (0, 1):
            tuning(leaf_max, device_build)
            ctx.upload_scene(arrays)
            # (clusters this small in a scene this large share their Morton codes: with one triangle per leaf the device builder's
            # tree would defer more than the traversal stack holds and it hands the scene to the host builder; with leaves of up
            # to 8 it builds the tree itself, and that tree is walked here)
            assert ctx.upload_timing()["built_on_device"] == bool(device_build and leaf_max == 8), (leaf_max, device_build)
            _check(ctx.closest_points(pts), want, (leaf_max, device_build))
            _check(ctx.closest_points(pts, md), want_md, (leaf_max, device_build, "radius"))
    # a non-finite point affects neither its neighbours nor whether the call ends
    bad = pts.copy(); bad[7] = [np.nan, 0, 0]; bad[70] = [np.inf, 1, 2]; bad[130] = [1, -np.inf, np.nan]
    got = ctx.closest_points(bad)
    keep = np.ones(len(pts), bool); keep[[7, 70, 130]] = False
    _check([g[keep] for g in got], [w[keep] for w in want], "beside non-finite points")


# ---- 7. degenerate triangles -----------------------------------------------------------------------------------------------------------
def test_degenerate_triangles(ctx, tuning):
    arrays, pts, want = _built("degenerate", CR.degenerate_mix)
    assert len(arrays["verts"]) >= 4096 and len(pts) <= 1000
    for device_build, leaf_max in ((0, 0), (0, 1), (0, 8), (1, 0), (1, 8)):
        tuning(leaf_max, device_build)
        ctx.upload_scene(arrays)
        assert ctx.upload_timing()["built_on_device"] == bool(device_build), (device_build, leaf_max)
        got = ctx.closest_points(pts)
        assert (got[0] >= 0).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all() and np.isfinite(got[3]).all()
        _check(got, want, (device_build, leaf_max))
    assert (want[0] % 4 == 0).sum() >= 50


# ---- 8. geometry edits are seen --------------------------------------------------------------------------------------------------------
def test_geometry_edits_are_seen(ctx):
    from pbrpathtracer_amd import ptk
    arrays, pts, want = _case("random300")
    ctx.upload_scene(arrays)
    _check(ctx.closest_points(pts), want, "before")
    n = len(arrays["verts"])
    a, b = n // 3, (2 * n) // 3
    moved = dict(arrays); moved["verts"] = np.array(arrays["verts"], F32, copy=True).reshape(n, 9)
    moved["verts"][a:b] = (moved["verts"][a:b].reshape(-1, 3, 3) + np.array([0.3, 0.15, -0.2], F32)).reshape(-1, 9)
    ctx.update_geometry(a, moved["verts"][a:b])
    edited = ctx.closest_points(pts)
    assert not np.array_equal(edited[0], want[0])
    _check(edited, CR.mirror(moved, pts), "after the update")
    fresh = ptk.Context(0)
    try:
        fresh.upload_scene(moved)
        _check(edited, fresh.closest_points(pts), "fresh upload")
    finally:
        fresh.close()


# ---- 9. no camera, no frame, frame state untouched -------------------------------------------------------------------------------------
def test_leaves_the_frame_state_alone(ctx):
    from pbrpathtracer_amd import ptk
    arrays, pts, want = _case("random300")
    _, cam = RC.scene("random300")
    W, H = 40, 24
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, 4); ctx.set_tile(0, 1); ctx.reset()
    ctx.render_adaptive(0.05, 4, 2, 8, 3)
    ctx.render_features(ptk.FEAT_ALL, 0, 3)
    state = lambda: [ctx.read_accum(), np.array(ctx.samples()), ctx.read_sample_counts(), ctx.resolve_rgb8()] + \
        [ctx.read_feature(k) for k in range(len(ptk.FEAT_NAMES))]
    before = state()
    _check(ctx.closest_points(pts), want, "after render_adaptive")
    for b, a in zip(before, state()):
        assert np.array_equal(b, a, equal_nan=b.dtype.kind == "f")
    ctx.request_exit()                                                            # does not cut the query
    _check(ctx.closest_points(pts), want, "after request_exit")
    ctx.reset()


def test_needs_no_camera_and_no_frame():
    from pbrpathtracer_amd import ptk
    arrays, pts, want = _case("s_cornell")
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays)
        _check(c.closest_points(pts), want, "no camera")
        assert c.last_closest_ms() > 0
    finally:
        c.close()


# ---- 10. device and host entries -------------------------------------------------------------------------------------------------------
def test_device_entries_and_caller_stream():
    import torch
    from pbrpathtracer_amd import ptk
    arrays, pts, want = _case("random300")
    n = len(pts)
    md = _radius_set(want[1], n)
    want_md = CR.mirror(arrays, pts, md)
    dev = torch.device("cuda:0")
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays)
        t_p, t_md = torch.from_numpy(pts).to(dev), torch.from_numpy(md).to(dev)
        torch.cuda.synchronize()
        out = c.closest_points(t_p)
        out_md = c.closest_points(t_p, t_md)
        c.synchronize()
        assert all(isinstance(o, torch.Tensor) and o.device == t_p.device for o in out + out_md)
        assert [tuple(o.shape) for o in out] == [(n,), (n,), (n, 3), (n, 2)]
        _check([o.cpu().numpy() for o in out], want, "device entry")
        _check([o.cpu().numpy() for o in out_md], want_md, "device entry, radius")
        nodes, tris = c.closest_stats(t_p)
        assert nodes >= n and tris >= n                                        # (every query fetches the root and tests a triangle)
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
            res = [o.clone() for o in c.closest_points(f_p, f_md)]
        s.synchronize()
        _check([o.cpu().numpy() for o in res], want_md, "caller stream")
    finally:
        c.close()


# ---- 11. arguments ---------------------------------------------------------------------------------------------------------------------
def test_arguments(ctx):
    from pbrpathtracer_amd import ptk
    arrays, pts, want = _case("s_cornell")
    L = ptk.load()
    n = 10
    p = pts[:n].copy()
    tri = np.full(n, 77, np.int32); dist = np.full(n, 7.0, F32); point = np.full((n, 3), 7.0, F32); bary = np.full((n, 2), 7.0, F32)
    pp = p.ctypes.data
    outs = (tri.ctypes.data, dist.ctypes.data, point.ctypes.data, bary.ctypes.data)
    BAD = -1
    fns = (L.ptk_closest_points, L.ptk_closest_points_device)

    def untouched():
        return (tri == 77).all() and (dist == 7).all() and (point == 7).all() and (bary == 7).all()

    fresh = ptk.Context(0)
    try:
        for fn in fns:
            assert fn(fresh.h, n, pp, None, *outs) == BAD                                   # before ptk_upload_scene
    finally:
        fresh.close()
    ctx.upload_scene(arrays)
    for fn in fns:
        assert fn(None, n, pp, None, *outs) == BAD                                          # null context
        assert fn(ctx.h, -1, pp, None, *outs) == BAD                                        # negative count
        assert fn(ctx.h, n, None, None, *outs) == BAD                                       # null points
        assert fn(ctx.h, n, pp, None, None, None, None, None) == BAD                        # no output at all
        assert fn(ctx.h, 0, None, None, None, None, None, None) == BAD
        assert fn(ctx.h, 0, None, None, *outs) == 0                                         # no points: nothing to do
    assert L.ptk_last_closest_ms(None, None) == BAD
    ctx.synchronize()
    assert untouched()                                                                      # a refused call leaves the outputs alone
    # every subset of the outputs but the empty one, through the host entry
    for m in range(1, 16):
        tri[:] = 77; dist[:] = 7; point[:] = 7; bary[:] = 7
        sel = [o if m >> k & 1 else None for k, o in enumerate(outs)]
        assert L.ptk_closest_points(ctx.h, n, pp, None, *sel) == 0, m
        for k, (g, w, keep) in enumerate(zip((tri, dist, point, bary), want, (77, 7, 7, 7))):
            assert np.array_equal(g, w[:n]) if m >> k & 1 else (g == keep).all(), (m, k)
    assert ctx.last_closest_ms() > 0
    e = np.zeros((0, 3), F32)
    assert [x.shape for x in ctx.closest_points(e)] == [(0,), (0,), (0, 3), (0, 2)]
    # a scene without triangles: misses
    empty = {k: (np.asarray(v)[:0].copy() if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material") else np.asarray(v).copy())
             for k, v in arrays.items()}
    empty["lights"] = np.zeros(0, np.int32)
    ctx.upload_scene(empty)
    g = ctx.closest_points(p)
    assert (g[0] == -1).all() and np.isposinf(g[1]).all() and (g[2] == 0).all() and (g[3] == 0).all()
    _check(g, CR.mirror(empty, p), "empty scene")
    assert L.ptk_closest_points(ctx.h, n, pp, None, None, dist.ctypes.data, None, None) == 0 and np.isposinf(dist).all()
    assert ctx.last_closest_ms() == 0                                                       # (no kernel ran)


# ---- 12. worked uses -------------------------------------------------------------------------------------------------------------------
def test_relocate_above_the_cornell_floor(ctx):
    from pbrpathtracer_amd import probes
    arrays, _, _ = _case("s_cornell")
    ctx.upload_scene(arrays)
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    extent = float((hi - lo).max())
    mid = 0.5 * (lo + hi)
    # a 6 x 6 patch over the middle of the floor (y up), at heights from 1 % to 30 % of the room
    gx, gz, gh = np.meshgrid(np.linspace(-0.15, 0.15, 6), np.linspace(-0.15, 0.15, 6), np.linspace(0.01, 0.30, 8), indexing="ij")
    pos = np.stack([mid[0] + gx.ravel() * extent, lo[1] + gh.ravel() * (hi[1] - lo[1]), mid[2] + gz.ravel() * extent], axis=1).astype(F32)
    min_dist = F32(0.15 * (hi[1] - lo[1]))
    dist, point, tri = probes.clearance(ctx, pos)
    _check((tri, dist, point), CR.mirror(arrays, pos)[:3], "clearance")
    near = dist < min_dist
    assert near.sum() >= 36 and (~near).sum() >= 36 and (dist > 0).all()
    new, moved = probes.relocate(ctx, pos, min_dist)
    assert new.dtype == F32 and new.shape == pos.shape
    assert np.array_equal(moved, near)
    assert np.array_equal(new[~moved], pos[~moved])                               # the others stay bit for bit
    scale = (min_dist / dist[moved]).astype(F32)
    assert np.array_equal(new[moved], point[moved] + (pos[moved] - point[moved]) * scale[:, None])
    after, _, _ = probes.clearance(ctx, new)
    ulp = float(np.spacing(F32(extent)))
    assert (np.abs(after[moved].astype(np.float64) - float(min_dist)) <= 4 * ulp).all()
    assert (after[~moved] >= min_dist).all()


def test_host_class_and_distance_field_cli(tmp_path):
    from pbrpathtracer_amd import probes, render, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    pts_file, _, _ = S.build_config("C1", str(tmp_path), width=32, height=24, depth=4)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    arrays = pt.StagedScene()
    p = RC.rays_in_box(arrays, 200, 9)[0]
    want = CR.mirror(arrays, p)
    _check(pt.closest_points(p), want, "PathTracer.closest_points")               # no resolution work, no render before it
    assert pt.LastError() == ""
    md = _radius_set(want[1], len(p), 16)
    _check(pt.closest_points(p, md), CR.mirror(arrays, p, md), "PathTracer.closest_points, radius")
    _check(pt.context().closest_points(p), want, "its context")
    # a pending geometry edit applies, as for RenderFrame(): object 0 staged again under another matrix ([column][row])
    M = np.eye(4, dtype=F32); M[3][0] = 0.05
    pt.SetObjectTransform(0, M)
    moved = pt.StagedScene()
    assert not np.array_equal(moved["verts"], arrays["verts"])
    _check(pt.closest_points(p), CR.mirror(moved, p), "after SetObjectTransform")
    pt.close()
    # the CLI on a 4 x 4 x 4 grid against Context.closest_points on the same positions
    npz = str(tmp_path / "field.npz")
    assert render.main([pts_file, "--distance-field", "4", "4", "4", "-o", npz]) == 0
    z = np.load(npz)
    assert sorted(z.files) == ["dist", "origin", "point", "side", "spacing", "tri"]
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    origin, spacing = probes.grid_over_bounds(v.min(axis=0), v.max(axis=0), (4, 4, 4))
    assert np.array_equal(z["origin"], origin) and np.array_equal(z["spacing"], spacing)
    pos = probes.grid_positions((4, 4, 4), origin, spacing)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    pt.closest_points(pos[:1])                                                    # (the scene is on the GPU from here on)
    tri, dist, point, _ = pt.context().closest_points(pos)
    pt.close()
    assert np.array_equal(z["tri"], tri.reshape(4, 4, 4)) and np.array_equal(z["dist"], dist.reshape(4, 4, 4))
    assert np.array_equal(z["point"], point.reshape(4, 4, 4, 3))
    _check((tri, dist, point), CR.mirror(arrays, pos)[:3], "the grid")
    assert z["side"].dtype == np.int8 and z["side"].shape == (4, 4, 4) and set(np.unique(z["side"]).tolist()) <= {-1, 0, 1}
    assert np.array_equal(z["side"], render.face_side(arrays["verts"], pos, point, tri).reshape(4, 4, 4))
    npz2 = str(tmp_path / "field_near.npz")
    reach = 0.5 * float(dist.max())                                               # (most of the grid lies on the room's walls)
    assert render.main([pts_file, "--distance-field", "4", "4", "4", "--df-max-dist", repr(reach), "-o", npz2]) == 0
    z2 = np.load(npz2)
    want2 = CR.mirror(arrays, pos, np.full(len(pos), reach, F32))
    assert np.array_equal(z2["tri"].ravel(), want2[0]) and np.array_equal(z2["dist"].ravel(), want2[1])
    assert (z2["side"].ravel()[want2[0] < 0] == 0).all() and (want2[0] < 0).any() and (want2[0] >= 0).any()
