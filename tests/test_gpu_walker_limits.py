"""Every kernel that walks the BVH, held to a tree-free reference where tests/test_gpu_bvh_limits.py holds probe_hits and render: on
a tree whose traversal stack is full, leaves of every size, adversarial geometry, coordinates up to 2^61 and refitted trees.

    ptk_intersect_rays, ptk_occluded_rays (hits_kernel, occluded_kernel)   tests/hit_rule.py: every triangle, ascending (t, index)
    ptk_closest_points (closest_kernel)                                    tests/closest_rule.py: every triangle, no tree
    ptk_trace_rays, ptk_trace_rays_adaptive (rays_kernel, rays_keyed)      the CPU oracle's trace_counter (tests/ray_cases.py)
    ptk_render_features, ptk_pick                                          tests/hit_rule.py over the oracle's camera rays

Every comparison is np.array_equal with dtype and shape; the references are computed once per scene (tests/walker_limit_cases.py,
which tests/test_walker_limits_cpu.py holds on the CPU) and never from a kernel.  That a lane's column of the LDS stack really is
full is shown by simulation on the downloaded tree (tests/stats_bounds.py stack_lower_bound, closest_stack_lower_bound), and the
deepest queries then run with trivial ones in the neighbouring lanes: a column that spilled would corrupt a live neighbour."""
import numpy as np
import pytest

import closest_rule as CR
import feature_truth as FT
import hit_rule as HR
import ray_cases as RC
import stats_bounds as SB
import walker_limit_cases as WC
from bvh_check import check_bvh, leaf_sizes
from test_gpu_bvh_limits import PTK_MAX_BVH_DEPTH, STACK_REALISED
from test_gpu_geometry_update import _motion
from walker_limit_cases import SAMPLE, SEED

pytestmark = pytest.mark.gpu

F32 = np.float32
HIT_NAMES = ("tri", "t", "bary", "material")
CLOSEST_NAMES = ("tri", "dist", "point", "bary")
COUNTS = (1, 63, 64, 65, 129)     # around the 64-lane group


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


@pytest.fixture
def tuning(ctx):
    """Builder tuning is process-wide (g_bvh_tuning): whatever a test sets is set back to the builders' own choices."""
    def set_(leaf_max, trav_cost=0):
        ctx.set_option("bvh_leaf_max", leaf_max)
        ctx.set_option("bvh_trav_cost", trav_cost)
    try:
        yield set_
    finally:
        set_(0, 0)
        ctx.set_option("device_build", 1)
        ctx.set_option("flat", 1)


def _upload(c, arrays, device_build, strict=True):
    c.set_option("device_build", device_build)
    c.upload_scene(arrays)
    if strict:
        assert c.upload_timing()["built_on_device"] == bool(device_build)


def _same(got, want, names, what):
    assert len(got) == len(want)
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        assert np.array_equal(g, w), f"{what}: {name} differs from the reference in {len(bad)} of {len(g)} queries, first {bad[:5].tolist()}"


def _check_rays(c, want, ro, rd, what, bounds=None):
    """intersect_rays against the mirror `want`, occluded_rays against hit_rule.occluded of the mirror's t for each bound"""
    _same(c.intersect_rays(ro, rd, SAMPLE, SEED), want, HIT_NAMES, what)
    for label, tmax in (bounds if bounds is not None else WC.occlusion_bounds(want[1])):
        got = c.occluded_rays(ro, rd, tmax, SAMPLE, SEED)
        ref = HR.occluded(want[1], tmax)
        assert got.dtype == ref.dtype == np.uint8 and got.shape == ref.shape == (len(ro),), (what, label)
        assert np.array_equal(got, ref), (what, "occluded", label, np.nonzero(got != ref)[0][:5].tolist())


def _closest(c, pts, md):
    """closest_points in calls of at most 400 points"""
    parts = [c.closest_points(pts[s:s + 400], None if md is None else md[s:s + 400]) for s in range(0, len(pts), 400)]
    return tuple(np.concatenate(p) for p in zip(*parts))


def _check_points(c, refs, pts, what):
    for label, md, want in refs:
        _same(_closest(c, pts, md), want, CLOSEST_NAMES, f"{what}, {label}")


# ---- (a) a traversal stack filled to its bound ------------------------------------------------------------------------------

NEST_TREES = [(L, dev) for L in (1, 8) for dev in (0, 1)]
W, H, DEPTH, SPP, FSEED = 48, 32, 4, 2, 9


def _nest():
    return WC.cached("nest", WC._nest)


def _nest_rays(oracle_mod):
    """the nest's 256 rays and the trivial one behind them, with their mirror"""
    ro, rd = (np.concatenate(x) for x in zip(WC.nest_rays(), WC.NEST_TRIVIAL_RAY))
    return ro, rd, WC.hits_reference(oracle_mod, "nest", _nest(), ro, rd)


def _interleave(deep, trivial, n=129):
    """rows for n lanes: even lanes cycle through `deep` (indices), odd lanes hold `trivial` (one index)"""
    rows = np.full(n, trivial, np.int64)
    rows[0::2] = np.resize(deep, len(rows[0::2]))
    return rows


def test_full_stack_hits_occlusion_and_closest_points(ctx, oracle_mod, tuning):
    arrays = _nest()
    verts = arrays["verts"]
    ro, rd, want = _nest_rays(oracle_mod)
    pts = np.concatenate([WC.nest_points(), WC.NEST_TRIVIAL_POINT])
    assert (want[0][:128] < 0).all() and (want[0][128:256] >= 0).mean() > 0.2 and want[0][256] == -1
    bounds = WC.occlusion_bounds(want[1])
    refs = WC.closest_reference("nest", arrays, pts)
    free = refs[0][2]
    assert (free[0] >= 0).all()
    md = np.full(len(pts), np.inf, F32); md[-1] = 0.0
    best_rays = best_points = 0
    for L, dev in NEST_TREES:
        tuning(L, 0)
        _upload(ctx, arrays, dev, strict=False)
        built = "device" if ctx.upload_timing()["built_on_device"] else "host"
        nodes, order = ctx.download_bvh()
        info = check_bvh(nodes, order, verts, leaf_max=L)
        assert info["stack_need"] == ctx.bvh_layout()[2] == PTK_MAX_BVH_DEPTH
        lb_r = SB.stack_lower_bound(nodes, verts, ro, rd, want[1])
        lb_p = SB.closest_stack_lower_bound(nodes, verts, pts)
        print(f"nest leaf_max {L} device_build {dev} (built on the {built}): stack_need {info['stack_need']}, depth {info['depth']}, "
              f"largest realised stack lower bound: rays {lb_r.max()} ({(lb_r == lb_r.max()).sum()} rays), "
              f"closest points {lb_p.max()} ({(lb_p == lb_p.max()).sum()} points)")
        assert lb_r.max() <= PTK_MAX_BVH_DEPTH and lb_p.max() <= PTK_MAX_BVH_DEPTH
        best_rays, best_points = max(best_rays, int(lb_r.max())), max(best_points, int(lb_p.max()))
        what = f"nest L{L} dev{dev}"
        _check_rays(ctx, want, ro, rd, what, bounds)
        _check_points(ctx, refs, pts, what)
        # the deepest queries in the even lanes, a trivial one in the odd lanes (the nest has no opacity maps: a ray's answer does
        # not depend on its place in the call)
        rows = _interleave(np.nonzero(lb_r == lb_r.max())[0], len(ro) - 1)
        assert (lb_r[rows[0::2]] == lb_r.max()).all() and (lb_r[rows[1::2]] == 0).all()
        prow = _interleave(np.nonzero(lb_p[:-1] == lb_p[:-1].max())[0], len(pts) - 1)
        for n in COUNTS:
            r = rows[:n]
            _same(ctx.intersect_rays(ro[r], rd[r], SAMPLE, SEED), [w[r] for w in want], HIT_NAMES, f"{what}, {n} interleaved rays")
            assert np.array_equal(ctx.occluded_rays(ro[r], rd[r], None, SAMPLE, SEED), (want[0][r] >= 0).astype(np.uint8)), (what, n)
            p = prow[:n]
            got = ctx.closest_points(pts[p], md[p])
            _same([g[0::2] for g in got], [w[p[0::2]] for w in free], CLOSEST_NAMES, f"{what}, {n} interleaved points")
            assert (got[0][1::2] == -1).all() and np.isposinf(got[1][1::2]).all() and (got[2][1::2] == 0).all() and (got[3][1::2] == 0).all()
    assert best_rays >= STACK_REALISED, best_rays
    assert best_points >= STACK_REALISED, best_points


def test_full_stack_radiance_features_and_pick(ctx, oracle_mod, tuning):
    from pbrpathtracer_amd import ptk
    arrays = _nest()
    verts = arrays["verts"]
    ro, rd, hits = _nest_rays(oracle_mod)
    sel = np.r_[0:64, 128:192, 256]                              # the 64 first rays of each half, and the trivial one
    ro, rd, t_hit = ro[sel], rd[sel], hits[1][sel]
    cam = WC.NEST_CAMERA

    def references():
        o = oracle_mod.Oracle(arrays)
        radiance = RC.truth(o, ro[:128], rd[:128], DEPTH, SEED, 0, SPP)
        rec = FT.camera_records(oracle_mod, arrays, cam, W, H, FSEED, 0, oracle=o)
        o.close()
        assert rec["seen"].all()
        planes = HR.mirror(oracle_mod, arrays, rec["ro"], rec["rd"], HR.ray_keys(FSEED, 0, W * H, 0))
        return radiance, planes
    radiance, planes = WC.cached("nest radiance and planes", references)
    assert (radiance != 0).any() and not np.isnan(radiance).any()
    assert 0.05 <= (planes[0] >= 0).mean()
    mask = (1 << ptk.FEAT_TRIANGLE) | (1 << ptk.FEAT_DEPTH) | (1 << ptk.FEAT_BARY) | (1 << ptk.FEAT_MATERIAL)
    rng = np.random.default_rng(3)
    picks = np.concatenate([rng.choice(np.nonzero(planes[0] >= 0)[0], 4, replace=False), rng.choice(np.nonzero(planes[0] < 0)[0], 4, replace=False)])
    o = oracle_mod.Oracle(arrays)
    for L, dev in NEST_TREES:
        tuning(L, 0)
        _upload(ctx, arrays, dev, strict=False)
        assert ctx.bvh_layout()[2] == PTK_MAX_BVH_DEPTH
        got = ctx.trace_rays(ro[:128], rd[:128], DEPTH, 0, SPP, SEED)
        assert got.dtype == np.float32 and got.shape == (128, 3)
        assert np.array_equal(got, radiance), (L, dev, int((got != radiance).any(axis=1).sum()))
        # the rays whose first walk fills the stack in the even lanes, the trivial ray in the odd ones: row i is traced on the stream of
        # RNG pixel i, so the oracle traces the interleaved set itself and a shorter call is its first rows
        lb = SB.stack_lower_bound(ctx.download_bvh()[0], verts, ro, rd, t_hit)
        rows = _interleave(np.nonzero(lb == lb.max())[0], 128)
        mixed = RC.truth(o, ro[rows], rd[rows], DEPTH, SEED, 0, SPP)
        assert (mixed[1::2] == 0).all()
        for n in COUNTS:
            assert np.array_equal(ctx.trace_rays(ro[rows[:n]], rd[rows[:n]], DEPTH, 0, SPP, SEED), mixed[:n]), (L, dev, n)
        ctx.set_camera(**cam); ctx.set_frame(W, H, DEPTH); ctx.set_tile(0, 1); ctx.reset()
        ctx.render_features(mask, 0, FSEED)
        top_down = lambda f: ctx.read_feature(f)[::-1].reshape(W * H, -1).squeeze()
        feats = [top_down(f) for f in (ptk.FEAT_TRIANGLE, ptk.FEAT_DEPTH, ptk.FEAT_BARY, ptk.FEAT_MATERIAL)]
        _same(feats, planes, HIT_NAMES, f"nest L{L} dev{dev} feature planes")
        for p in picks:
            tri, mat, t = ctx.pick(int(p % W), int(p // W), FSEED)
            assert (tri, mat) == (planes[0][p], planes[3][p]) and F32(t) == planes[1][p], (L, dev, int(p))
    o.close()
    ro, rd = ro[:128], rd[:128]
    # rays_keyed_kernel on the last of the full-stack trees: every ray of an adaptive query holds ptk_trace_rays of its own count
    # (tests/test_gpu_rays_adaptive.py's invariant), and the count-SPP rays hold the oracle's sums
    s1, _, n, _ = ctx.trace_rays_adaptive(ro, rd, DEPTH, 0.05, SPP, 2, 6, SEED)
    for k in np.unique(n):
        plain = ctx.trace_rays(ro, rd, DEPTH, 0, int(k), SEED)
        assert np.array_equal(s1[n == k], plain[n == k]), int(k)
    assert np.array_equal(s1[n == SPP], radiance[n == SPP])


# ---- (b) leaves of every size up to 8, both builders ---------------------------------------------------------------------------

def _sweep_scene(scene):
    def make():
        if scene == 0:
            return "soup 20k", WC._scene(WC._soup(20000, 0.03, 31))
        arrays, _ = WC.random_scene(41, 6000, True)
        assert any((m["tex"][5] >= 0) for m in arrays["materials"]), "the textured scene needs opacity maps"
        return "textured 6000", arrays
    return WC.cached(("sweep", scene), make)


@pytest.mark.parametrize("scene", [0, 1], ids=["soup 20k", "textured 6000"])
def test_leaf_size_sweep(ctx, oracle_mod, tuning, scene):
    name, arrays = _sweep_scene(scene)
    verts = arrays["verts"]
    ro, rd = WC._aimed_rays(verts, 400, 7 + scene)
    pts = RC.rays_in_box(arrays, 400, 5)[0]
    want = WC.hits_reference(oracle_mod, name, arrays, ro, rd)
    assert (want[0] >= 0).mean() > 0.5
    bounds = WC.occlusion_bounds(want[1])
    refs = WC.closest_reference(name, arrays, pts)
    for L in (1, 2, 3, 5, 8):
        sizes = {0: np.zeros(9, np.int64), 1: np.zeros(9, np.int64)}
        for cost in (0, 4, 16):
            tuning(L, cost)
            for dev in (0, 1):
                _upload(ctx, arrays, dev)
                h = leaf_sizes(ctx.download_bvh()[0])
                assert h[L + 1:].sum() == 0 and h[0] == 0
                sizes[dev] += h
                what = f"{name} L{L} c{cost} dev{dev}"
                _check_rays(ctx, want, ro, rd, what, bounds)
                _check_points(ctx, refs, pts, what)
        for dev in (0, 1):
            assert (sizes[dev][2:L + 1] > 0).all(), (name, L, dev, sizes[dev].tolist())


# ---- (c) adversarial geometry --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", WC.SOAK_KINDS)
def test_adversarial_geometry(ctx, oracle_mod, tuning, kind):
    seed = WC.SOAK_SEEDS[kind]
    verts = WC._soak_scene(kind, seed)
    arrays = WC.cached(("soak", kind), lambda: WC._scene(verts))
    ro, rd = WC._aimed_rays(verts, 400, seed)
    pts = WC.soak_points(kind, verts, seed)
    want = WC.hits_reference(oracle_mod, ("soak", kind), arrays, ro, rd)
    bounds = WC.occlusion_bounds(want[1])
    refs = WC.closest_reference(("soak", kind), arrays, pts)
    assert (refs[0][2][0] >= 0).all()
    for L in (0, 8):
        tuning(L, 4 if L else 0)
        for dev in (0, 1):
            _upload(ctx, arrays, dev)
            what = f"{kind} L{L} dev{dev}"
            _check_rays(ctx, want, ro, rd, what, bounds)
            _check_points(ctx, refs, pts, what)


# ---- (d) the far domain --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("e", WC.FAR_EXPONENTS)
def test_far_domain(ctx, oracle_mod, tuning, e):
    verts, ro, rd = WC.far_cluster(e)
    arrays = WC.cached(("far scene", e), lambda: WC._scene(verts))
    m = len(ro)
    full = WC.hits_reference(oracle_mod, ("far", e), arrays, ro, rd)
    assert (full[0][m // 2:] >= 0).mean() > 0.3
    # the rays whose closest hit no tree can promise, from the brute-force reference alone (the scene has no opacity maps: a ray's
    # answer does not depend on its place in the call, so the reference of the rays that stay is its rows)
    ill = WC._off_box(verts, ro, rd, (full[0], np.concatenate([full[1][:, None], full[2]], axis=1)))
    print(f"2^{e}: {int(ill.sum())} of {m} rays hit off their triangle's box by more than the slack (left out)")
    assert ill.sum() <= m // 100, ill.sum()
    ok = ~ill
    want = tuple(w[ok] for w in full)
    bounds = WC.occlusion_bounds(want[1])
    pts = WC.far_points(e)
    refs = WC.closest_reference(("far", e), arrays, pts)
    assert (refs[0][2][0] >= 0).all() and np.isfinite(refs[0][2][1]).all()
    for L in (1, 8):
        tuning(L, 0)
        for dev in (0, 1):
            _upload(ctx, arrays, dev)
            what = f"2^{e} L{L} dev{dev}"
            _check_rays(ctx, want, ro[ok], rd[ok], what, bounds)
            _check_points(ctx, refs, pts, what)                   # every point: the rule is defined for every finite one


# ---- (e) after a refit ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["huge and tiny", "nest"])
def test_after_a_refit(ctx, oracle_mod, tuning, name):
    from pbrpathtracer_amd import ptk
    if name == "nest":
        arrays = _nest()
        ro, rd = WC.nest_rays()
        pts = WC.nest_points()[::2]
        tuning(1, 0)
        _upload(ctx, arrays, 0)
    else:
        seed = WC.SOAK_SEEDS[name]
        verts = WC._soak_scene(name, seed)
        arrays = WC.cached(("soak", name), lambda: WC._scene(verts))
        ro, rd = WC._aimed_rays(verts, 400, seed)
        pts = WC.soak_points(name, verts, seed)[::2]
        _upload(ctx, arrays, 1)
    stack = ctx.bvh_layout()[2]
    print(f"{name}: stack_need {stack} before the updates")
    assert stack == PTK_MAX_BVH_DEPTH or name != "nest"
    now = arrays
    for kind in ("jitter", "far"):
        first, nv, _, _, now = _motion(now, kind)
        assert len(nv) == len(now["verts"]) if kind == "jitter" else len(now["verts"]) // 4 < len(nv) < len(now["verts"]) // 2
        ctx.update_geometry(first, nv)
        assert ctx.bvh_layout()[2] == stack
        want = HR.mirror(oracle_mod, now, ro, rd, HR.ray_keys(SEED, 0, len(ro), SAMPLE))
        free = CR.mirror_radii(now, pts, [None])[0]
        md = np.random.default_rng(11).uniform(0.0, 2.0 * float(np.median(free["dist"])), len(pts)).astype(F32)
        four = lambda d: (d["tri"], d["dist"], d["point"], d["bary"])
        refs = [("no radius", None, four(free)), ("uniform", md, four(CR.mirror_radii(now, pts, [md])[0]))]
        bounds = WC.occlusion_bounds(want[1])[::3]                 # no bound, and the seeded uniform set
        what = f"{name} after {kind}"
        _check_rays(ctx, want, ro, rd, what, bounds)
        _check_points(ctx, refs, pts, what)
        fresh = ptk.Context(0)
        try:
            fresh.upload_scene(now)
            _check_rays(fresh, want, ro, rd, what + ", fresh context", bounds)
            _check_points(fresh, refs, pts, what + ", fresh context")
        finally:
            fresh.close()
