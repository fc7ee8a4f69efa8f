"""Crossing counts, point containment and the signed distance (include/ptk.h ptk_crossings_rays, ptk_contains_points,
ptk_signed_distance) against the numpy restatement of the rule (tests/crossings_rule.py, which
tests/test_crossings_cpu.py holds to the float64 winding number), bit for bit: whatever the count, the cut of the query set, tmax,
the builder, the leaf size, the "flat" and "contract" options and the tile split, on closed meshes, on the trees at their limits
(tests/walker_limit_cases.py) and on edited geometry.  Every comparison is np.array_equal, with dtype and shape; the references are
computed once per case and never from a kernel."""
import numpy as np
import pytest

import closest_rule as CR
import crossings_rule as XR
import hit_rule as HR
import ray_cases as RC
import walker_limit_cases as WC

pytestmark = pytest.mark.gpu

F32 = np.float32
CLOSEST_NAMES = ("tri", "dist", "point", "bary")
COUNTS = (1, 63, 64, 65, 129)     # a partial wave, a full wave, a second workgroup with one lane, a third


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


def DIRS():
    from pbrpathtracer_amd import ptk
    return ptk.inside_default_dirs()


def DIRS5():
    """five directions of the caller's own: the built-in three and two more, not normalised"""
    return np.concatenate([DIRS(), np.array([[-0.41, -0.83, 0.57], [1.3, 0.29, -2.1]], F32)])


_ref = {}


def cached(key, make):
    """a reference, computed once; shared, not to be modified"""
    if key not in _ref:
        _ref[key] = make()
    return _ref[key]


def _same(got, want, names, what):
    assert len(got) == len(want)
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w, equal_nan=False):
            bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
            raise AssertionError(f"{what}: {name} differs from the rule in {len(bad)} of {len(g)} queries, first {bad[:5].tolist()}: "
                                 f"{g[bad[:3]].tolist()} != {w[bad[:3]].tolist()}")


def _check_rays(c, arrays, ro, rd, tmax, what, key=None):
    want = cached(("rays", key, what), lambda: XR.crossings(arrays, ro, rd, tmax)) if key is not None else XR.crossings(arrays, ro, rd, tmax)
    _same(c.crossings_rays(ro, rd, tmax), want, ("front", "back"), what)
    return want


def _check_points(c, arrays, pts, what, key, dirs=None, modes=(XR.WINDING, XR.PARITY), max_dist=None, signed=True):
    """contains_points with winding, and signed_distance, in both modes against the rule"""
    d = DIRS() if dirs is None else dirs
    closest = cached(("closest", key, max_dist is not None), lambda: CR.mirror(arrays, pts, max_dist)) if signed else None
    for mode in modes:
        inside, winding = cached(("contains", key, len(d), mode), lambda: XR.contains(arrays, pts, d, mode))
        _same(c.contains_points(pts, dirs, mode, want_winding=True), (inside, winding), ("inside", "winding"), f"{what}, mode {mode}")
        got = c.contains_points(pts, dirs, mode)
        assert isinstance(got, np.ndarray) and np.array_equal(got, inside)
        if not signed:
            continue
        want = (closest[0], XR.flip_sign(closest[1], inside), closest[2], closest[3])
        _same(c.signed_distance(pts, max_dist, dirs, mode), want, CLOSEST_NAMES, f"{what}, signed distance, mode {mode}")
    return inside


def _box_rays(verts, n, seed, grow=0.3):
    return RC.rays_in_box(dict(verts=verts), n, seed)


# ---- 1. the smallest shapes --------------------------------------------------------------------------------------------------------
def test_smallest_shapes(ctx):
    one = CR.scene_of([[0, 0, 0, 1, 0, 0, 0, 1, 0]])
    cube = CR.scene_of(XR.mesh("cube"))
    rng = np.random.default_rng(3)
    for name, arrays in (("one triangle", one), ("cube", cube)):
        ctx.upload_scene(arrays)
        ro = rng.uniform(-2, 2, (129, 3)).astype(F32)
        aim = rng.uniform(-0.9, 0.9, (129, 3)) if name == "cube" else np.c_[rng.uniform(0, 0.5, (129, 2)), np.zeros(129)]
        rd = (aim - ro).astype(F32)
        pts = rng.uniform(-1.5, 1.5, (129, 3)).astype(F32)
        front, back = XR.crossings(arrays, ro, rd)
        assert (front + back > 0).mean() > 0.8
        for n in COUNTS:
            _same(ctx.crossings_rays(ro[:n], rd[:n]), (front[:n], back[:n]), ("front", "back"), (name, n))
            _check_points(ctx, arrays, pts[:n], f"{name}, {n} points", (name, n))
        assert ctx.last_crossings_ms() > 0
    inside = XR.contains(cube, pts, DIRS())[0]
    assert 0.1 < inside.mean() < 0.9
    # no queries
    e3 = np.zeros((0, 3), F32)
    assert [(x.shape, x.dtype) for x in ctx.crossings_rays(e3, e3)] == [((0,), np.int32)] * 2
    got = ctx.contains_points(e3, want_winding=True)
    assert (got[0].shape, got[0].dtype, got[1].shape, got[1].dtype) == ((0,), np.uint8, (0, 3), np.int32)
    assert [x.shape for x in ctx.signed_distance(e3)] == [(0,), (0,), (0, 3), (0, 2)]
    # a scene without triangles: zeros, and the closest-point misses
    empty = {k: (np.asarray(v)[:0].copy() if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material") else np.asarray(v).copy())
             for k, v in cube.items()}
    ctx.upload_scene(empty)
    front, back = ctx.crossings_rays(ro, rd)
    assert front.dtype == np.int32 and (front == 0).all() and (back == 0).all()
    inside, winding = ctx.contains_points(pts, want_winding=True)
    assert inside.dtype == np.uint8 and (inside == 0).all() and winding.shape == (129, 3) and (winding == 0).all()
    _same(ctx.signed_distance(pts), CR.mirror(empty, pts), CLOSEST_NAMES, "empty scene")
    assert ctx.last_crossings_ms() == 0                                                     # (no kernel ran)


# ---- 2. the closed meshes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", XR.MESHES)
def test_closed_meshes(ctx, name):
    verts = XR.mesh(name)
    arrays = cached(("scene", name), lambda: CR.scene_of(verts))
    pts = XR.mesh_points(verts)
    ro, rd = _box_rays(verts, 1000, 5)
    ctx.upload_scene(arrays)
    front, back = _check_rays(ctx, arrays, ro, rd, None, name, key=name)
    assert (front + back > 0).mean() > 0.4 and (front + back >= 2).mean() > 0.1
    t_mid = np.random.default_rng(11).uniform(0.0, 2.0, len(ro)).astype(F32)
    _check_rays(ctx, arrays, ro, rd, t_mid, name + " tmax", key=name)
    inside = _check_points(ctx, arrays, pts, name, name)
    w = cached(("winding number", name), lambda: np.abs(XR.winding_number64(verts, pts)) > 0.5)
    assert np.array_equal(inside.astype(bool), w)                                           # ... and that is containment
    _check_points(ctx, arrays, pts[:600], name + " five directions", (name, 5), dirs=DIRS5())
    md = np.random.default_rng(12).uniform(0.0, 0.5, 600).astype(F32)
    _check_points(ctx, arrays, pts[:600], name + " radius", (name, "md"), max_dist=md)


# ---- 3. a scene with opacity maps, glass and lights: geometry only -----------------------------------------------------------------
@pytest.mark.parametrize("case", ("s_cornell", "s_opacity", "random300"))
def test_ray_case_scenes(ctx, case):
    arrays, _ = RC.scene(case)
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    ctx.upload_scene(arrays)
    front, back = _check_rays(ctx, arrays, ro, rd, None, case, key=case)
    assert (front + back > 0).mean() > 0.25 and (front + back >= 2).mean() > 0.05
    _check_points(ctx, arrays, ro[:300], case, case)
    for k, name in enumerate(("front", "back")):                            # each output requested alone
        from pbrpathtracer_amd import ptk
        out = [np.full(len(ro), 77, np.int32), np.full(len(ro), 77, np.int32)]
        sel = [o.ctypes.data if j == k else None for j, o in enumerate(out)]
        assert ptk.load().ptk_crossings_rays(ctx.h, len(ro), ro.ctypes.data, rd.ctypes.data, None, *sel) == 0
        assert np.array_equal(out[k], (front, back)[k]) and (out[1 - k] == 77).all()


# ---- 4. the trees at their limits --------------------------------------------------------------------------------------------------
def _upload(c, arrays, device_build, strict=True):
    c.set_option("device_build", device_build)
    c.upload_scene(arrays)
    if strict:
        assert c.upload_timing()["built_on_device"] == bool(device_build)


def test_full_stack_nest(ctx, tuning):
    from test_gpu_bvh_limits import PTK_MAX_BVH_DEPTH
    arrays = WC.cached("nest", WC._nest)
    ro, rd = (np.concatenate(x) for x in zip(WC.nest_rays(), WC.NEST_TRIVIAL_RAY))
    pts = np.concatenate([WC.nest_points()[::5], WC.NEST_TRIVIAL_POINT])
    assert not XR.off_box(arrays["verts"], ro, rd).any()
    for L in (1, 8):
        for dev in (0, 1):
            ctx.set_option("bvh_leaf_max", L); ctx.set_option("bvh_trav_cost", 0)
            _upload(ctx, arrays, dev, strict=False)
            assert ctx.bvh_layout()[2] == PTK_MAX_BVH_DEPTH
            what = f"nest L{L} dev{dev}"
            front, back = _check_rays(ctx, arrays, ro, rd, None, "nest", key="nest")
            assert (front + back).max() == len(arrays["verts"])                             # a ray through every triangle of the nest
            _check_points(ctx, arrays, pts, what, "nest", modes=(XR.WINDING,), signed=L == 8 and dev == 1)
            # the deepest walks in the even lanes, the trivial ray in the odd ones: a column that spilled would corrupt a neighbour
            rows = np.full(129, len(ro) - 1); rows[0::2] = np.resize(np.arange(128), 65)
            _same(ctx.crossings_rays(ro[rows], rd[rows]), (front[rows], back[rows]), ("front", "back"), what + " interleaved")
    ctx.set_option("bvh_trav_cost", 0)


LIMIT_CASES = ["onion", "far 20", "far 59", "huge and tiny", "duplicates"]


def _limit_case(name):
    def make():
        if name == "onion":
            arrays = WC._onion()
            ro, rd = WC._aimed_rays(arrays["verts"], 200, 5)
        elif name.startswith("far"):
            verts, ro, rd = WC.far_cluster(int(name.split()[1]))
            arrays = WC._scene(verts)
        else:
            verts = WC._soak_scene(name, WC.SOAK_SEEDS[name])
            arrays = WC._scene(verts)
            ro, rd = WC._aimed_rays(verts, 400, WC.SOAK_SEEDS[name])
        # the rays whose count no tree can promise, from the rule alone (crossings_rule.off_box)
        ill = XR.off_box(arrays["verts"], ro, rd)
        return arrays, ro[~ill], rd[~ill], int(ill.sum()), len(ro)
    return cached(("limit", name), make)


@pytest.mark.parametrize("name", LIMIT_CASES)
def test_trees_at_their_limits(ctx, tuning, name):
    arrays, ro, rd, ill, m = _limit_case(name)
    print(f"{name}: {ill} of {m} rays cross a triangle off its box by more than the slack (left out)")
    assert ill <= m // 50 and (ill == 0 or name.startswith("far"))
    builders = {"huge and tiny": (1,), "duplicates": (0,)}.get(name, (0, 1))                # one soak scene per builder
    want = cached(("limit rays", name), lambda: XR.crossings(arrays, ro, rd))
    assert (want[0] + want[1] > 0).mean() > 0.3
    t_one = cached(("limit tmax", name), lambda: _tmax_at_a_crossing(arrays["verts"], ro, rd))
    want_t = cached(("limit rays t", name), lambda: XR.crossings(arrays, ro, rd, t_one))
    pts = ro[:100]
    for L in (1, 8):
        for dev in builders:
            tuning(L, dev)
            ctx.upload_scene(arrays)
            what = f"{name} L{L} dev{dev}"
            _same(ctx.crossings_rays(ro, rd), want, ("front", "back"), what)
            _same(ctx.crossings_rays(ro, rd, t_one), want_t, ("front", "back"), what + " tmax")
            if name in ("huge and tiny", "duplicates"):
                _check_points(ctx, arrays, pts, what, ("limit", name), modes=(XR.WINDING,))


def _tmax_at_a_crossing(verts, ro, rd):
    """float32 [n]: the t of each ray's farthest crossing (strict: that one is then not counted), 1 for a ray that crosses nothing"""
    out = np.ones(len(ro), F32)
    step = max(1, (1 << 22) // len(verts))
    for s in range(0, len(ro), step):
        _, _, _, t = XR.per_triangle(verts, ro[s:s + step], rd[s:s + step])
        fr, bk = XR.crossing_masks(verts, ro[s:s + step], rd[s:s + step], np.full(len(t), np.inf, F32))
        tt = np.where(fr | bk, t, F32(-np.inf)).max(axis=1)
        out[s:s + step] = np.where(tt > 0, tt, F32(1))
    return out


# ---- 5. independence ---------------------------------------------------------------------------------------------------------------
def test_independent_of_builder_leaf_size_flat_contract_tiles_and_cuts(ctx, tuning):
    arrays, _ = RC.scene("random6000")
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    pts = ro[:300]
    tm = np.random.default_rng(11).uniform(0.0, 2.0, len(ro)).astype(F32)
    for device_build in (0, 1):
        for leaf_max in (1, 8):
            tuning(leaf_max, device_build)
            ctx.upload_scene(arrays)
            assert ctx.upload_timing()["built_on_device"] == bool(device_build)
            _check_rays(ctx, arrays, ro, rd, None, "random6000", key="random6000")
            _check_rays(ctx, arrays, ro, rd, tm, "random6000 tmax", key="random6000")
            _check_points(ctx, arrays, pts, f"random6000 {device_build} {leaf_max}", "random6000")
    tuning(0, 1)
    arrays, _ = RC.scene("random16")
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    pts = ro[:300]
    ctx.upload_scene(arrays)
    for flat in (0, 1):
        ctx.set_option("flat", flat)
        _check_rays(ctx, arrays, ro, rd, None, "random16", key="random16")
        _check_points(ctx, arrays, pts, f"random16 flat {flat}", "random16")
    ctx.set_tile(1, 3)
    _check_rays(ctx, arrays, ro, rd, None, "random16", key="random16")
    for contract in (1, 2, 0):
        ctx.set_option("contract", contract)
        _check_rays(ctx, arrays, ro, rd, None, "random16", key="random16")
        _check_points(ctx, arrays, pts, f"random16 contract {contract}", "random16")
    # the query set cut into calls at non-multiples of 64
    whole = ctx.crossings_rays(ro, rd, tm)
    whole_p = ctx.contains_points(pts, want_winding=True)
    whole_s = ctx.signed_distance(pts)
    for a, b in ((0, 300), (77, 141), (299, 300)):
        _same(ctx.crossings_rays(ro[a:b], rd[a:b], tm[a:b]), [w[a:b] for w in whole], ("front", "back"), (a, b))
        _same(ctx.contains_points(pts[a:b], want_winding=True), [w[a:b] for w in whole_p], ("inside", "winding"), (a, b))
        _same(ctx.signed_distance(pts[a:b]), [w[a:b] for w in whole_s], CLOSEST_NAMES, (a, b))


def test_after_update_geometry_with_a_refit(ctx):
    arrays, _ = RC.scene("random300")
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    pts = ro[:300]
    ctx.upload_scene(arrays)
    before = _check_rays(ctx, arrays, ro, rd, None, "random300", key="random300")
    n = len(arrays["verts"])
    a, b = n // 3, (2 * n) // 3
    moved = dict(arrays); moved["verts"] = np.array(arrays["verts"], F32, copy=True).reshape(n, 9)
    moved["verts"][a:b] = (moved["verts"][a:b].reshape(-1, 3, 3) + np.array([0.3, 0.15, -0.2], F32)).reshape(-1, 9)
    ctx.update_geometry(a, moved["verts"][a:b])
    info = ctx.geometry_info()
    assert info["updates"] == 1 and info["refitted"]
    after = _check_rays(ctx, moved, ro, rd, None, "random300 moved", key="random300 moved")
    assert not np.array_equal(after[0] + after[1], before[0] + before[1])
    _check_points(ctx, moved, pts, "random300 moved", "random300 moved")


def test_device_entries(ctx):
    import torch
    from pbrpathtracer_amd import ptk
    verts = XR.mesh("torus")
    arrays = cached(("scene", "torus"), lambda: CR.scene_of(verts))
    ro, rd = _box_rays(verts, 1000, 5)
    pts = XR.mesh_points(verts)[:1000]
    tm = np.random.default_rng(11).uniform(0.0, 2.0, len(ro)).astype(F32)
    md = np.random.default_rng(12).uniform(0.0, 0.5, len(pts)).astype(F32)
    dev = torch.device("cuda:0")
    ctx.upload_scene(arrays)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t_ro, t_rd, t_tm, t_p, t_md, t_d5 = to(ro), to(rd), to(tm), to(pts), to(md), to(DIRS5())
    torch.cuda.synchronize()
    host = [ctx.crossings_rays(ro, rd), ctx.crossings_rays(ro, rd, tm), ctx.contains_points(pts, None, XR.PARITY, want_winding=True),
            ctx.contains_points(pts, DIRS5(), XR.WINDING, want_winding=True), ctx.signed_distance(pts, md), ctx.signed_distance(pts, None, DIRS5(), "parity")]
    got = [ctx.crossings_rays(t_ro, t_rd), ctx.crossings_rays(t_ro, t_rd, t_tm), ctx.contains_points(t_p, None, XR.PARITY, want_winding=True),
           ctx.contains_points(t_p, t_d5, XR.WINDING, want_winding=True), ctx.signed_distance(t_p, t_md), ctx.signed_distance(t_p, None, t_d5, "parity")]
    ctx.synchronize()
    names = [("front", "back")] * 2 + [("inside", "winding")] * 2 + [CLOSEST_NAMES] * 2
    for h, g, nm in zip(host, got, names):
        assert all(isinstance(x, torch.Tensor) and x.device == t_p.device for x in g)
        _same([x.cpu().numpy() for x in g], h, nm, "device entry")
    _same(host[0], XR.crossings(arrays, ro, rd), ("front", "back"), "host entry")
    _same(host[3], XR.contains(arrays, pts, DIRS5(), XR.WINDING), ("inside", "winding"), "host entry, five directions")
    assert ctx.last_crossings_ms() > 0
    # the device form of the signed distance is the closest-point call with the sign set in place
    closest = ctx.closest_points(t_p, t_md)
    ctx.synchronize()
    c_tri, c_dist, c_point, c_bary = (x.cpu().numpy() for x in closest)
    s = [x.cpu().numpy() for x in got[4]]
    assert np.array_equal(s[0], c_tri) and np.array_equal(np.abs(s[1]), c_dist) and np.array_equal(s[2], c_point) and np.array_equal(s[3], c_bary)


# ---- 6. tmax -----------------------------------------------------------------------------------------------------------------------
def test_tmax(ctx, oracle_mod):
    arrays, _ = RC.scene("s_cornell")
    assert (oracle_mod.normalise_arrays(arrays)["materials"]["tex"][:, HR.OPACITY_SLOT] < 0).all(), "an opaque scene"
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    ctx.upload_scene(arrays)
    free = _check_rays(ctx, arrays, ro, rd, None, "s_cornell", key="s_cornell")
    n = len(ro)
    # a bound equal to one crossing's own t: strict, that crossing is not counted
    t_far = cached("cornell t_far", lambda: _tmax_at_a_crossing(arrays["verts"], ro, rd))
    at = _check_rays(ctx, arrays, ro, rd, t_far, "s_cornell tmax = t", key="s_cornell")
    crosses = free[0] + free[1] > 0
    assert crosses.mean() > 0.5 and ((at[0] + at[1])[crosses] == (free[0] + free[1])[crosses] - 1).mean() > 0.9
    above = _check_rays(ctx, arrays, ro, rd, np.nextafter(t_far, F32(np.inf)), "s_cornell tmax above t", key="s_cornell")
    assert np.array_equal((above[0] + above[1])[crosses], (free[0] + free[1])[crosses])
    mix = np.random.default_rng(11).uniform(0.0, 2.0, n).astype(F32)
    mix[0::7] = np.nan; mix[1::7] = 0.0; mix[2::7] = -1.0; mix[3::7] = np.inf; mix[4::7] = -0.0; mix[5::7] = -np.inf
    got = _check_rays(ctx, arrays, ro, rd, mix, "s_cornell mixture", key="s_cornell")
    for k in (0, 1, 2, 4, 5):
        assert (got[0][k::7] == 0).all() and (got[1][k::7] == 0).all(), k
    assert np.array_equal(got[0][3::7], free[0][3::7]) and np.array_equal(got[1][3::7], free[1][3::7])
    for bad in (np.nan, 0.0, -1.0):
        f, b = ctx.crossings_rays(ro[:70], rd[:70], np.full(70, bad, F32))
        assert (f == 0).all() and (b == 0).all(), bad
    # against the occlusion query the product already has, on this opaque scene: occluded == (front + back > 0)
    t_hit = HR.mirror(oracle_mod, arrays, ro, rd, HR.PROBE_KEY)[1]
    for label, tmax in WC.occlusion_bounds(t_hit):
        f, b = ctx.crossings_rays(ro, rd, tmax)
        assert np.array_equal(ctx.occluded_rays(ro, rd, tmax), (f + b > 0).astype(np.uint8)), label


# ---- 7. the signed distance --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("icosphere", "cube flipped"))
def test_signed_distance(ctx, name):
    verts = XR.mesh(name)
    arrays = cached(("scene", name), lambda: CR.scene_of(verts))
    pts = XR.mesh_points(verts)[3500:]
    ctx.upload_scene(arrays)
    for md in (None, np.full(len(pts), 0.25, F32)):
        tri, dist, point, bary = ctx.closest_points(pts, md)
        inside = ctx.contains_points(pts)
        s = ctx.signed_distance(pts, md)
        assert np.array_equal(s[0], tri) and np.array_equal(s[2], point) and np.array_equal(s[3], bary)
        assert np.array_equal(np.abs(s[1]), dist) and np.array_equal(np.signbit(s[1]), inside.astype(bool))
        assert np.array_equal(s[1], XR.flip_sign(dist, inside))
        assert 0.1 < inside.mean() < 0.9
        if md is not None:
            deep = inside.astype(bool) & (tri < 0)                          # inside and beyond max_dist
            assert deep.sum() >= 10 and np.isneginf(s[1][deep]).all() and np.isposinf(s[1][~inside.astype(bool) & (tri < 0)]).all()
    # the centre, with a reach that ends short of the surface
    s = ctx.signed_distance(np.zeros((1, 3), F32), np.array([0.1], F32))
    assert s[0][0] == -1 and np.isneginf(s[1][0]) and (s[2] == 0).all() and (s[3] == 0).all()
    # each output alone through the host entry
    from pbrpathtracer_amd import ptk
    want = ctx.signed_distance(pts)
    for k, name_k in enumerate(CLOSEST_NAMES):
        out = [np.full(len(pts), 77, np.int32), np.full(len(pts), 7.0, F32), np.full((len(pts), 3), 7.0, F32), np.full((len(pts), 2), 7.0, F32)]
        sel = [o.ctypes.data if j == k else None for j, o in enumerate(out)]
        assert ptk.load().ptk_signed_distance(ctx.h, len(pts), pts.ctypes.data, None, 3, None, 0, *sel) == 0
        for j in range(4):
            assert np.array_equal(out[j], want[j]) if j == k else (out[j] == (77 if j == 0 else 7)).all(), (name_k, j)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    from pbrpathtracer_amd import ptk
    L = ptk.load()
    arrays = cached(("scene", "cube"), lambda: CR.scene_of(XR.mesh("cube")))
    n = 10
    o = np.random.default_rng(1).uniform(-1, 1, (n, 3)).astype(F32)
    d5 = DIRS5(); d4 = np.ascontiguousarray(d5[:4])
    front = np.full(n, 77, np.int32); back = np.full(n, 77, np.int32); inside = np.full(n, 77, np.uint8); winding = np.full((n, 5), 77, np.int32)
    tri = np.full(n, 77, np.int32); dist = np.full(n, 7.0, F32); point = np.full((n, 3), 7.0, F32); bary = np.full((n, 2), 7.0, F32)
    op, fp, bp, ip, wp = o.ctypes.data, front.ctypes.data, back.ctypes.data, inside.ctypes.data, winding.ctypes.data
    sd = (tri.ctypes.data, dist.ctypes.data, point.ctypes.data, bary.ctypes.data)
    BAD = -1

    def untouched():
        return all((x == 77).all() for x in (front, back, inside, winding, tri)) and all((x == 7).all() for x in (dist, point, bary))

    fresh = ptk.Context(0)
    try:                                                                                    # before ptk_upload_scene
        for fn in (L.ptk_crossings_rays, L.ptk_crossings_rays_device):
            assert fn(fresh.h, n, op, op, None, fp, bp) == BAD
        for fn in (L.ptk_contains_points, L.ptk_contains_points_device):
            assert fn(fresh.h, n, op, 3, None, 0, ip, None) == BAD
        for fn in (L.ptk_signed_distance, L.ptk_signed_distance_device):
            assert fn(fresh.h, n, op, None, 3, None, 0, *sd) == BAD
    finally:
        fresh.close()
    ctx.upload_scene(arrays)
    for fn in (L.ptk_crossings_rays, L.ptk_crossings_rays_device):
        assert fn(None, n, op, op, None, fp, bp) == BAD                                     # null context
        assert fn(ctx.h, -1, op, op, None, fp, bp) == BAD                                   # negative count
        assert fn(ctx.h, n, None, op, None, fp, bp) == BAD and fn(ctx.h, n, op, None, None, fp, bp) == BAD
        assert fn(ctx.h, n, op, op, None, None, None) == BAD                                # both outputs NULL
        assert fn(ctx.h, 0, None, None, None, fp, bp) == 0                                  # no rays: nothing to do
    for fn in (L.ptk_contains_points, L.ptk_contains_points_device):
        assert fn(None, n, op, 3, None, 0, ip, wp) == BAD
        assert fn(ctx.h, -1, op, 3, None, 0, ip, wp) == BAD
        assert fn(ctx.h, n, None, 3, None, 0, ip, wp) == BAD
        assert fn(ctx.h, n, op, 3, None, 0, None, None) == BAD                              # no output
        assert fn(ctx.h, n, op, 4, d4.ctypes.data, 0, ip, wp) == BAD                        # an even D
        for D in (0, -1, 33):
            assert fn(ctx.h, n, op, D, d5.ctypes.data, 0, ip, wp) == BAD, D                 # D outside 1 .. 31
        assert fn(ctx.h, n, op, 5, None, 0, ip, wp) == BAD and fn(ctx.h, n, op, 1, None, 0, ip, wp) == BAD      # the built-in set has three
        assert fn(ctx.h, n, op, 3, None, 2, ip, wp) == BAD and fn(ctx.h, n, op, 3, None, -1, ip, wp) == BAD     # an unknown mode
        assert fn(ctx.h, 0, None, 3, None, 0, ip, wp) == 0
    for fn in (L.ptk_signed_distance, L.ptk_signed_distance_device):
        assert fn(None, n, op, None, 3, None, 0, *sd) == BAD
        assert fn(ctx.h, n, None, None, 3, None, 0, *sd) == BAD
        assert fn(ctx.h, n, op, None, 3, None, 0, None, None, None, None) == BAD
        assert fn(ctx.h, n, op, None, 4, d4.ctypes.data, 0, *sd) == BAD
        assert fn(ctx.h, n, op, None, 5, None, 0, *sd) == BAD
        assert fn(ctx.h, n, op, None, 3, None, 7, *sd) == BAD
    ctx.synchronize()
    assert untouched()
    assert "num_dirs" in L.ptk_last_error(ctx.h).decode() or "mode" in L.ptk_last_error(ctx.h).decode()
    with pytest.raises(ptk.PtkError):
        ctx.contains_points(o, d4)
    with pytest.raises(ptk.PtkError):
        ctx.signed_distance(o, None, None, "sideways")
    # and the host entries do work with these arrays
    assert L.ptk_contains_points(ctx.h, n, op, 5, d5.ctypes.data, 1, ip, wp) == 0
    _same((inside, winding), XR.contains(arrays, o, d5, XR.PARITY), ("inside", "winding"), "after the refusals")


# ---- 9. order: no camera, no frame, frame state untouched --------------------------------------------------------------------------
def test_leaves_the_frame_state_alone(ctx):
    from pbrpathtracer_amd import ptk
    arrays, cam = RC.scene("random300")
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    pts = ro[:300]
    W, H = 40, 24
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, 4); ctx.set_tile(0, 1); ctx.reset()
    ctx.render(0, 2, 3)
    plain = ctx.read_accum().copy()
    _check_rays(ctx, arrays, ro, rd, None, "random300", key="random300")
    _check_points(ctx, arrays, pts, "between renders", "random300")
    ctx.reset(); ctx.render(0, 2, 3)
    assert np.array_equal(ctx.read_accum(), plain)                                          # a render before and after a query is unchanged
    ctx.reset()
    ctx.render_adaptive(0.05, 4, 2, 8, 3)
    ctx.render_features(ptk.FEAT_ALL, 0, 3)
    state = lambda: [ctx.read_accum(), np.array(ctx.samples()), ctx.read_sample_counts(), ctx.resolve_rgb8()] + \
        [ctx.read_feature(k) for k in range(len(ptk.FEAT_NAMES))]
    before = state()
    _check_rays(ctx, arrays, ro, rd, None, "random300", key="random300")                   # legal after render_adaptive
    _check_points(ctx, arrays, pts, "after render_adaptive", "random300")
    for b, a in zip(before, state()):
        assert np.array_equal(b, a, equal_nan=b.dtype.kind == "f")
    ctx.request_exit()                                                                      # does not cut the query
    _check_rays(ctx, arrays, ro, rd, None, "random300", key="random300")
    ctx.reset()


def test_needs_no_camera_and_no_frame():
    from pbrpathtracer_amd import ptk
    verts = XR.mesh("icosphere")
    arrays = cached(("scene", "icosphere"), lambda: CR.scene_of(verts))
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays)
        ro, rd = _box_rays(verts, 1000, 5)
        _check_rays(c, arrays, ro, rd, None, "icosphere", key="icosphere")
        assert c.last_crossings_ms() > 0
    finally:
        c.close()


# ---- 10. worked uses and the upper layers ------------------------------------------------------------------------------------------
def test_probes_and_layers(ctx):
    from pbrpathtracer_amd import probes, rays
    verts = XR.mesh("torus")
    arrays = cached(("scene", "torus"), lambda: CR.scene_of(verts))
    pts = XR.mesh_points(verts)[4096:]
    ctx.upload_scene(arrays)
    want = XR.contains(arrays, pts, DIRS())[0].astype(bool)
    got = probes.inside(ctx, pts)
    assert got.dtype == bool and np.array_equal(got, want) and 0.05 < want.mean() < 0.9
    new0, moved0 = probes.relocate(ctx, pts, 0.1)
    new, moved, keep = probes.relocate(ctx, pts, 0.1, drop_inside=True)
    assert np.array_equal(keep, ~want) and np.array_equal(moved, moved0 & keep) and (moved0 & ~keep).any()
    assert np.array_equal(new[moved], new0[moved]) and np.array_equal(new[~moved], pts[~moved])
    # walls between point pairs: through the tube once, across the whole torus, and clear of it
    a = np.array([[1.0, 0, 0], [-2.0, 0.0, 0.05], [-2.0, 0.0, 1.0]], F32); b = np.array([[2.0, 0.1, 0.05], [2.0, 0.1, 0.0], [2.0, 0.0, 1.0]], F32)
    layers = rays.count_layers(ctx, a, b)
    f, bk = XR.crossings(arrays, *rays.segment_rays(a, b))
    assert layers.dtype == np.int32 and np.array_equal(layers, f + bk) and layers.tolist() == [1, 4, 0]


def test_host_class_and_signed_distance_field_cli(tmp_path):
    from pbrpathtracer_amd import render, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    pts_file, _, _ = S.build_config("C1", str(tmp_path), width=32, height=24, depth=4)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    arrays = pt.StagedScene()
    ro, rd = RC.rays_in_box(arrays, 300, 9)
    _same(pt.crossings_rays(ro, rd), XR.crossings(arrays, ro, rd), ("front", "back"), "PathTracer.crossings_rays")   # no render before it
    assert pt.LastError() == ""
    tm = np.random.default_rng(2).uniform(0, 3, len(ro)).astype(F32)
    _same(pt.crossings_rays(ro, rd, tm), XR.crossings(arrays, ro, rd, tm), ("front", "back"), "PathTracer.crossings_rays, tmax")
    _same(pt.contains_points(ro, DIRS5(), "parity", want_winding=True), XR.contains(arrays, ro, DIRS5(), XR.PARITY), ("inside", "winding"),
          "PathTracer.contains_points")
    assert np.array_equal(pt.contains_points(ro), XR.contains(arrays, ro, DIRS())[0])
    _same(pt.signed_distance(ro), XR.signed_distance(arrays, ro, DIRS()), CLOSEST_NAMES, "PathTracer.signed_distance")
    from pbrpathtracer_amd import ptk
    with pytest.raises(ptk.PtkError):
        pt.contains_points(ro, DIRS5()[:4])
    assert "num_dirs" in pt.LastError()
    # a pending geometry edit applies, as for RenderFrame()
    M = np.eye(4, dtype=F32); M[3][0] = 0.05
    pt.SetObjectTransform(0, M)
    moved = pt.StagedScene()
    assert not np.array_equal(moved["verts"], arrays["verts"])
    _same(pt.crossings_rays(ro, rd), XR.crossings(moved, ro, rd), ("front", "back"), "after SetObjectTransform")
    pt.close()
    # the CLI: every array of the unsigned field stays byte for byte, inside and sdf are added
    plain, signed, parity = (str(tmp_path / f) for f in ("field.npz", "field_signed.npz", "field_parity.npz"))
    assert render.main([pts_file, "--distance-field", "5", "4", "6", "-o", plain]) == 0
    assert render.main([pts_file, "--distance-field", "5", "4", "6", "--signed", "-o", signed]) == 0
    assert render.main([pts_file, "--distance-field", "5", "4", "6", "--signed", "--inside-mode", "parity", "--df-max-dist", "0.3", "-o", parity]) == 0
    z0, z1, z2 = np.load(plain), np.load(signed), np.load(parity)
    assert sorted(z0.files) == ["dist", "origin", "point", "side", "spacing", "tri"]
    assert sorted(z1.files) == sorted(z0.files + ["inside", "sdf"])
    for k in z0.files:
        assert z1[k].dtype == z0[k].dtype and z1[k].tobytes() == z0[k].tobytes(), k
    from pbrpathtracer_amd import probes
    pos = probes.grid_positions((5, 4, 6), z0["origin"], z0["spacing"])
    inside, _ = XR.contains(arrays, pos, DIRS())
    assert z1["inside"].dtype == np.uint8 and z1["inside"].shape == (6, 4, 5) and np.array_equal(z1["inside"].ravel(), inside)
    assert np.array_equal(z1["sdf"].ravel(), XR.flip_sign(z0["dist"].ravel(), inside))
    want2 = XR.signed_distance(arrays, pos, DIRS(), XR.PARITY, np.full(len(pos), 0.3, F32))
    assert np.array_equal(z2["sdf"].ravel(), want2[1]) and np.array_equal(z2["tri"].ravel(), want2[0])
    assert np.array_equal(z2["inside"].ravel(), XR.contains(arrays, pos, DIRS(), XR.PARITY)[0])
