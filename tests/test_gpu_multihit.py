"""Ordered multi-hit ray queries (include/ptk.h ptk_multihit_rays) against the numpy restatement of the rule
(tests/multihit_rule.py, which tests/test_multihit_cpu.py holds to a float64 brute force), bit for bit: whatever the count, the list
length, tmax, the builder, the leaf size, the "flat" and "contract" options, the tile split and the cut of the ray set; on scenes
made to evict from a full list, to tie exactly and to leave lists short, on the trees at their limits (tests/walker_limit_cases.py)
and on edited geometry.  Every comparison is np.array_equal, with dtype and shape; the references are computed once per case, at
K = 16 and cut to the K of a call (the prefix property, which test_multihit_cpu.py holds within the mirror), and never from a
kernel."""
import numpy as np
import pytest

import closest_rule as CR
import crossings_rule as XR
import multihit_rule as MR
import ray_cases as RC
import walker_limit_cases as WC

pytestmark = pytest.mark.gpu

F32 = np.float32
COUNTS = (1, 63, 64, 65, 129)     # a partial wave, a full wave, a second workgroup with one lane, a third
NAMES = MR.NAMES


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


_ref = {}


def cached(key, make):
    """a reference, computed once; shared, not to be modified"""
    if key not in _ref:
        _ref[key] = make()
    return _ref[key]


def _same(got, want, what):
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w, equal_nan=False):
            bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
            raise AssertionError(f"{what}: {name} differs from the rule in {len(bad)} of {len(g)} rays, first {bad[:5].tolist()}: "
                                 f"{g[bad[:3]].tolist()} != {w[bad[:3]].tolist()}")


def _full(key, arrays, ro, rd, tmax=None):
    """the rule's answer at K = 16, once per key"""
    return cached(("full", key), lambda: MR.multihit(arrays, ro, rd, 16, tmax))


def _check(c, full, ro, rd, K, tmax, what):
    _same(c.multihit_rays(ro, rd, K, tmax), MR.cut(full, K), f"{what}, K = {K}")


def _tmax_at_a_crossing(verts, ro, rd):
    """float32 [n]: the t of each ray's farthest crossing (strict: that one is then not listed), 1 for a ray that crosses nothing"""
    out = np.ones(len(ro), F32)
    step = max(1, (1 << 22) // len(verts))
    for s in range(0, len(ro), step):
        _, _, _, t = XR.per_triangle(verts, ro[s:s + step], rd[s:s + step])
        fr, bk = XR.crossing_masks(verts, ro[s:s + step], rd[s:s + step], np.full(len(t), np.inf, F32))
        tt = np.where(fr | bk, t, F32(-np.inf)).max(axis=1)
        out[s:s + step] = np.where(tt > 0, tt, F32(1))
    return out


def _raw(c, ro, rd, K, outs, tmax=None):
    """the C entry itself: outs = five arrays or None"""
    from pbrpathtracer_amd import ptk
    L = ptk.load()
    return L.ptk_multihit_rays(c.h, len(ro), ro.ctypes.data, rd.ctypes.data, tmax.ctypes.data if tmax is not None else None, K,
                               *(o.ctypes.data if o is not None else None for o in outs))


def _sentinels(n, K):
    return [np.full(n, 77, np.int32), np.full((n, K), 77, np.int32), np.full((n, K), 7.0, F32), np.full((n, K, 2), 7.0, F32), np.full((n, K), 77, np.int8)]


def _untouched(outs):
    return all((o == (7 if o.dtype == F32 else 77)).all() for o in outs)


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
        full = MR.multihit(arrays, ro, rd, 16)
        assert (full[0] > 0).mean() > 0.8
        for n in COUNTS:
            for K in (1, 2, 3, 16):
                _same(ctx.multihit_rays(ro[:n], rd[:n], K), MR.cut(MR.rows_of(full, slice(0, n)), K), (name, n, K))
        assert ctx.last_multihit_ms() > 0
    # every output requested alone: the others are not touched
    want = MR.cut(full, 3)
    for k in range(5):
        outs = _sentinels(129, 3)
        assert _raw(ctx, ro, rd, 3, [o if j == k else None for j, o in enumerate(outs)]) == 0
        assert np.array_equal(outs[k], want[k]), NAMES[k]
        assert _untouched([o for j, o in enumerate(outs) if j != k]), NAMES[k]
    # K = 0 and K = 17 are refused and the outputs left alone; so is a call without an output
    from pbrpathtracer_amd import ptk
    outs = _sentinels(129, 16)
    for K in (0, 17, -1):
        assert _raw(ctx, ro, rd, K, outs) == -1, K
        with pytest.raises(ptk.PtkError):
            ctx.multihit_rays(ro, rd, K)
    assert "max_hits" in ptk.load().ptk_last_error(ctx.h).decode()
    assert _raw(ctx, ro, rd, 3, [None] * 5) == -1
    ctx.synchronize()
    assert _untouched(outs)
    # no rays
    e3 = np.zeros((0, 3), F32)
    assert [(x.shape, x.dtype) for x in ctx.multihit_rays(e3, e3, 5)] == \
        [((0,), np.int32), ((0, 5), np.int32), ((0, 5), F32), ((0, 5, 2), F32), ((0, 5), np.int8)]
    assert ptk.load().ptk_multihit_rays(ctx.h, 0, None, None, None, 3, *(o.ctypes.data for o in outs)) == 0 and _untouched(outs)
    # a scene without triangles: the unused-slot values everywhere, by fills
    empty = {k: (np.asarray(v)[:0].copy() if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material") else np.asarray(v).copy())
             for k, v in cube.items()}
    ctx.upload_scene(empty)
    _same(ctx.multihit_rays(ro, rd, 5), MR.multihit(empty, ro, rd, 5), "empty scene")
    assert ctx.last_multihit_ms() == 0                                                      # (no kernel ran)


# ---- 2. eviction, ties and short lists ---------------------------------------------------------------------------------------------
KS = (1, 2, 3, 4, 8, 16)


@pytest.mark.parametrize("size,device_build", ((4000, 0), (6000, 1)))
def test_soup(ctx, tuning, size, device_build):
    arrays = cached(("soup", size), lambda: CR.scene_of(MR.soup(size, 0.5, 7)))
    ro, rd = RC.rays_in_box(arrays, 512, 11)
    verts = np.asarray(arrays["verts"], F32).reshape(-1, 9)
    front, back = cached(("soup crossings", size), lambda: XR.crossings(arrays, ro, rd))
    total = front + back
    for K in KS:
        more, short = (total > K).mean(), ((total > 0) & (total < K)).mean()
        print(f"soup {size}, K = {K}: {more:.3f} of the rays cross more than K triangles, {short:.3f} between 1 and K - 1")
        # (the 6000-triangle soup is denser: only 0.037 of its rays cross exactly one triangle, so the K = 2 share of short lists is
        # held on the 4000-triangle soup, 0.082 there, and from K = 3 on both)
        assert more >= 0.2 and (K < 2 or (K == 2 and size == 6000) or short >= 0.05), (K, more, short)
    bounds = {"no tmax": None,
              "tmax at the farthest crossing": cached(("soup far", size), lambda: _tmax_at_a_crossing(verts, ro, rd)),
              "random tmax": np.random.default_rng(12).uniform(0.0, 2.0, len(ro)).astype(F32)}
    for L in (1, 8):
        tuning(L, device_build)
        ctx.upload_scene(arrays)
        assert ctx.upload_timing()["built_on_device"] == bool(device_build)
        for label, tmax in bounds.items():
            full = _full(("soup", size, label), arrays, ro, rd, tmax)
            for K in KS:
                _check(ctx, full, ro, rd, K, tmax, f"soup {size} L{L}, {label}")
    # the farthest crossing is the one a strict bound at its t leaves out
    free, at = _full(("soup", size, "no tmax"), arrays, ro, rd), _full(("soup", size, "tmax at the farthest crossing"), arrays, ro, rd)
    few = (total > 0) & (total <= 16)
    assert few.mean() > 0.15 and np.array_equal(at[0][few], free[0][few] - 1)


def _slab_rays(n=512, seed=4):
    """half from z = -0.5, half from z = 1.5, aimed at U(-0.9, 0.9)^2 on the plane z = 0.5 from within 0.05 of the aim in x and y:
    every ray passes through all the squares"""
    rng = np.random.default_rng(seed)
    aim = np.c_[rng.uniform(-0.9, 0.9, (n, 2)), np.full(n, 0.5)]
    ro = np.c_[aim[:, :2] + rng.uniform(-0.05, 0.05, (n, 2)), np.where(np.arange(n) < n // 2, -0.5, 1.5)]
    return ro.astype(F32), (aim - ro).astype(F32)


def test_slabs(ctx, tuning):
    arrays = cached("slabs", lambda: CR.scene_of(MR.slabs(24)))
    verts = np.asarray(arrays["verts"], F32).reshape(-1, 9)
    ro, rd = _slab_rays()
    front, back = XR.crossings(arrays, ro, rd)
    assert (front + back == 30).all()                                                       # more than K for every K
    bounds = {"no tmax": None, "tmax at the farthest crossing": _tmax_at_a_crossing(verts, ro, rd),
              "random tmax": np.random.default_rng(12).uniform(0.0, 2.0, len(ro)).astype(F32)}
    eight = MR.cut(_full(("slabs", "no tmax"), arrays, ro, rd), 8)
    assert (eight[0] == 8).all() and (np.diff(eight[2], axis=1) == 0).any(axis=1).all()     # every kept list holds an exact tie
    tie = np.diff(eight[2], axis=1) == 0
    assert (np.diff(eight[1], axis=1)[tie] > 0).all()                                       # ... the smaller index first
    for L in (1, 8):
        for dev in (0, 1):
            tuning(L, dev)
            ctx.upload_scene(arrays)
            for label, tmax in bounds.items():
                full = _full(("slabs", label), arrays, ro, rd, tmax)
                for K in (1, 4, 8, 16):
                    _check(ctx, full, ro, rd, K, tmax, f"slabs L{L} dev{dev}, {label}")


# ---- 3. cross-checks on the GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("s_cornell", "s_opacity", "random300"))
def test_ray_case_scenes(ctx, case):
    arrays, _ = RC.scene(case)
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    ctx.upload_scene(arrays)
    full = _full(case, arrays, ro, rd)
    assert (full[0] > 0).mean() > 0.25 and (full[0] >= 2).mean() > 0.05
    got16 = ctx.multihit_rays(ro, rd, 16)
    _same(got16, full, case)
    front, back = ctx.crossings_rays(ro, rd)
    for K in (1, 3, 16):
        got = ctx.multihit_rays(ro, rd, K)
        _same(got, MR.cut(full, K), f"{case}, K = {K}")
        assert np.array_equal(got[0], np.minimum(K, front + back).astype(np.int32)), K
        _same(got, MR.cut(got16, K), f"{case}: the first {K} columns of K = 16")
    if case == "s_cornell":                                                                 # no opacity maps: K = 1 is the closest hit
        _one_hit_is_intersect_rays(ctx, ro, rd)


def _one_hit_is_intersect_rays(c, ro, rd):
    count, tri, t, bary, side = c.multihit_rays(ro, rd, 1)
    h_tri, h_t, h_bary, _ = c.intersect_rays(ro, rd)
    assert (h_tri >= 0).mean() > 0.3
    assert np.array_equal(tri[:, 0], h_tri) and np.array_equal(t[:, 0], h_t) and np.array_equal(bary[:, 0], h_bary)
    assert np.array_equal(count, (h_tri >= 0).astype(np.int32))


def test_one_hit_is_the_closest_hit_on_the_cube(ctx):
    arrays = CR.scene_of(XR.mesh("cube"))
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    ctx.upload_scene(arrays)
    _one_hit_is_intersect_rays(ctx, ro, rd)


# ---- 4. the trees at their limits --------------------------------------------------------------------------------------------------
def _upload(c, arrays, device_build):
    c.set_option("device_build", device_build)
    c.upload_scene(arrays)


def test_full_stack_nest(ctx, tuning):
    from test_gpu_bvh_limits import PTK_MAX_BVH_DEPTH
    arrays = WC.cached("nest", WC._nest)
    ro, rd = (np.concatenate(x) for x in zip(WC.nest_rays(), WC.NEST_TRIVIAL_RAY))
    assert not XR.off_box(arrays["verts"], ro, rd).any()
    full = _full("nest", arrays, ro, rd)
    assert (full[0] == 16).any()
    # the deepest walks in the even lanes, the trivial ray in the odd ones: a column that spilled would corrupt a neighbour
    rows = np.full(129, len(ro) - 1); rows[0::2] = np.resize(np.arange(128), 65)
    for L in (1, 8):
        for dev in (0, 1):
            ctx.set_option("bvh_leaf_max", L); ctx.set_option("bvh_trav_cost", 0)
            _upload(ctx, arrays, dev)
            assert ctx.bvh_layout()[2] == PTK_MAX_BVH_DEPTH
            for K in (16, 1):
                _check(ctx, full, ro, rd, K, None, f"nest L{L} dev{dev}")
                _same(ctx.multihit_rays(ro[rows], rd[rows], K), MR.cut(MR.rows_of(full, rows), K), f"nest L{L} dev{dev} interleaved, K = {K}")
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
        # the rays whose crossings no tree can promise, from the rule alone (crossings_rule.off_box)
        ill = XR.off_box(arrays["verts"], ro, rd)
        return arrays, ro[~ill], rd[~ill], int(ill.sum()), len(ro)
    return cached(("limit", name), make)


@pytest.mark.parametrize("name", LIMIT_CASES)
def test_trees_at_their_limits(ctx, tuning, name):
    arrays, ro, rd, ill, m = _limit_case(name)
    print(f"{name}: {ill} of {m} rays cross a triangle off its box by more than the slack (left out)")
    assert ill <= m // 50 and (ill == 0 or name.startswith("far"))
    builders = {"huge and tiny": (1,), "duplicates": (0,)}.get(name, (0, 1))                # one soak scene per builder
    full = _full(("limit", name), arrays, ro, rd)
    assert (full[0] > 0).mean() > 0.3
    for L in (1, 8):
        for dev in builders:
            tuning(L, dev)
            ctx.upload_scene(arrays)
            for K in (1, 16):
                _check(ctx, full, ro, rd, K, None, f"{name} L{L} dev{dev}")


# ---- 5. independence ---------------------------------------------------------------------------------------------------------------
def test_independent_of_builder_leaf_size_flat_contract_tiles_and_cuts(ctx, tuning):
    arrays, _ = RC.scene("random6000")
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    tm = np.random.default_rng(11).uniform(0.0, 2.0, len(ro)).astype(F32)
    full, full_t = _full("random6000", arrays, ro, rd), _full("random6000 tmax", arrays, ro, rd, tm)
    for device_build in (0, 1):
        for leaf_max in (1, 8):
            tuning(leaf_max, device_build)
            ctx.upload_scene(arrays)
            assert ctx.upload_timing()["built_on_device"] == bool(device_build)
            for K in (1, 5, 16):
                _check(ctx, full, ro, rd, K, None, f"random6000 {device_build} {leaf_max}")
                _check(ctx, full_t, ro, rd, K, tm, f"random6000 {device_build} {leaf_max} tmax")
    tuning(0, 1)
    arrays, _ = RC.scene("random16")
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    full = _full("random16", arrays, ro, rd)
    ctx.upload_scene(arrays)
    for flat in (0, 1):
        ctx.set_option("flat", flat)
        _check(ctx, full, ro, rd, 4, None, f"random16 flat {flat}")
    ctx.set_tile(1, 3)
    _check(ctx, full, ro, rd, 4, None, "random16 tile 1 of 3")
    for contract in (1, 2, 0):
        ctx.set_option("contract", contract)
        _check(ctx, full, ro, rd, 4, None, f"random16 contract {contract}")
    # the ray set cut into calls at non-multiples of 64
    whole = ctx.multihit_rays(ro, rd, 6, tm)
    for a, b in ((0, 300), (77, 141), (299, 300)):
        _same(ctx.multihit_rays(ro[a:b], rd[a:b], 6, tm[a:b]), MR.rows_of(whole, slice(a, b)), (a, b))


def test_after_update_geometry_with_a_refit(ctx):
    arrays, _ = RC.scene("random300")
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    ctx.upload_scene(arrays)
    before = _full("random300", arrays, ro, rd)
    _check(ctx, before, ro, rd, 16, None, "random300")
    n = len(arrays["verts"])
    a, b = n // 3, (2 * n) // 3
    moved = dict(arrays); moved["verts"] = np.array(arrays["verts"], F32, copy=True).reshape(n, 9)
    moved["verts"][a:b] = (moved["verts"][a:b].reshape(-1, 3, 3) + np.array([0.3, 0.15, -0.2], F32)).reshape(-1, 9)
    ctx.update_geometry(a, moved["verts"][a:b])
    info = ctx.geometry_info()
    assert info["updates"] == 1 and info["refitted"]
    after = _full("random300 moved", moved, ro, rd)
    assert not np.array_equal(after[1], before[1])
    refit = ctx.multihit_rays(ro, rd, 16)
    _same(refit, after, "random300 after a refit")
    ctx.upload_scene(moved)
    _same(ctx.multihit_rays(ro, rd, 16), refit, "a fresh upload of the moved scene")


def test_device_entry(ctx):
    import torch
    verts = XR.mesh("torus")
    arrays = cached(("scene", "torus"), lambda: CR.scene_of(verts))
    ro, rd = RC.rays_in_box(dict(verts=verts), 1000, 5)
    tm = np.random.default_rng(11).uniform(0.0, 2.0, len(ro)).astype(F32)
    dev = torch.device("cuda:0")
    ctx.upload_scene(arrays)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t_ro, t_rd, t_tm = to(ro), to(rd), to(tm)
    torch.cuda.synchronize()
    for K, tmax, t_tmax in ((1, None, None), (4, tm, t_tm), (7, None, None), (16, tm, t_tm)):
        host = ctx.multihit_rays(ro, rd, K, tmax)
        got = ctx.multihit_rays(t_ro, t_rd, K, t_tmax)
        ctx.synchronize()
        assert all(isinstance(x, torch.Tensor) and x.device == t_ro.device for x in got)
        _same([x.cpu().numpy() for x in got], host, f"device entry, K = {K}")
        _same(host, MR.multihit(arrays, ro, rd, K, tmax), f"host entry, K = {K}")
    assert ctx.last_multihit_ms() > 0


# ---- 6. worked uses and the upper layers -------------------------------------------------------------------------------------------
def test_thickness_and_layers_between(ctx):
    from pbrpathtracer_amd import rays
    arrays = CR.scene_of(XR.mesh("cube"))
    ctx.upload_scene(arrays)
    rng = np.random.default_rng(8)
    a = np.c_[rng.uniform(-0.9, 0.9, (200, 2)), np.full(200, -3.0)].astype(F32)
    b = np.c_[a[:, :2] + rng.uniform(-0.05, 0.05, (200, 2)), np.full(200, 3.0)].astype(F32)
    got = rays.layers_between(ctx, a, b, 4)
    _same(got, MR.multihit(arrays, a, b - a, 4, np.ones(200, F32)), "layers_between")
    assert (got[0] == 2).mean() > 0.9                                                       # (a segment through a face's diagonal: 3 or 4)
    length, complete = rays.thickness(ctx, a, b - a, 4)
    count, _, t, _, side = got
    want = rays.inside_length(count, t, side, 4)
    assert np.array_equal(length, want[0]) and np.array_equal(complete, want[1])
    two = count == 2
    assert np.array_equal(length[two], (t[two, 1] - t[two, 0])) and (np.abs(length[two] * 6.0 - 2.0) < 1e-3).all() and complete[two].all()
    # from inside the cube the list starts with a way out: the origin is taken to be outside, so nothing is counted
    o = np.zeros((1, 3), F32); d = np.array([[0.3, 0.2, 1.0]], F32)
    assert rays.thickness(ctx, o, d)[0].tolist() == [0.0]


def test_host_class_and_layers_cli(tmp_path):
    from pbrpathtracer_amd import ptk, render, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    from pbrpathtracer_amd.rays import equirect_rays
    pts_file, _, _ = S.build_config("C1", str(tmp_path), width=32, height=24, depth=4)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    arrays = pt.StagedScene()
    ro, rd = RC.rays_in_box(arrays, 300, 9)
    tm = np.random.default_rng(2).uniform(0, 3, len(ro)).astype(F32)
    _same(pt.multihit_rays(ro, rd, 5), MR.multihit(arrays, ro, rd, 5), "PathTracer.multihit_rays")          # no render before it
    assert pt.LastError() == ""
    _same(pt.MultiHitRays(ro, rd, 16, tm), MR.multihit(arrays, ro, rd, 16, tm), "PathTracer.MultiHitRays, tmax")
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays)
        _same(pt.multihit_rays(ro, rd, 3, tm), c.multihit_rays(ro, rd, 3, tm), "PathTracer against Context")
    finally:
        c.close()
    with pytest.raises(ptk.PtkError):
        pt.multihit_rays(ro, rd, 17)
    # a pending geometry edit applies, as for CrossingsRays
    M = np.eye(4, dtype=F32); M[3][0] = 0.05
    pt.SetObjectTransform(0, M)
    moved = pt.StagedScene()
    assert not np.array_equal(moved["verts"], arrays["verts"])
    _same(pt.multihit_rays(ro, rd, 5), MR.multihit(moved, ro, rd, 5), "after SetObjectTransform")
    cam = pt.GetCamera()
    pt.close()
    # the CLI: the arrays of --hits stay byte for byte, the layers are added
    plain, layered = str(tmp_path / "planes.npz"), str(tmp_path / "layers.npz")
    assert render.main([pts_file, "--equirect", "64", "--hits", plain]) == 0
    assert render.main([pts_file, "--equirect", "64", "--hits", layered, "--layers", "3"]) == 0
    assert render.main([pts_file, "--equirect", "64", "--hits", layered, "--layers", "17"]) == 1
    z0, z1 = np.load(plain), np.load(layered)
    assert sorted(z1.files) == sorted(z0.files + ["layer_t", "layer_tri", "layer_count"])
    for k in z0.files:
        assert z1[k].dtype == z0[k].dtype and z1[k].tobytes() == z0[k].tobytes(), k
    count, tri, t, _, _ = MR.multihit(arrays, *equirect_rays(*cam, 64, 32), 3)
    assert z1["layer_count"].shape == (32, 64) and np.array_equal(z1["layer_count"].ravel(), count)
    assert z1["layer_t"].shape == (3, 32, 64) and np.array_equal(z1["layer_t"].reshape(3, -1), t.T)
    assert z1["layer_tri"].dtype == np.int32 and np.array_equal(z1["layer_tri"].reshape(3, -1), tri.T)
