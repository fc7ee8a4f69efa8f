"""Probe visibility (include/ptk.h ptk_bake_probe_visibility, ptk_probes_irradiance_visible) against numpy, bit for
bit: the depth table is what ptk_intersect_rays returns for every (probe, direction) ray on the key of the ray's index - the candidate
rule of tests/hit_rule.py -, the moments and the lookup are the float32 restatement of tests/probe_vis_cases.py, whatever the
batching into blocks of probes, the builder, the leaf size, "flat", the tile split and the frame state.  Every comparison is
np.array_equal."""
import numpy as np
import pytest

import hit_rule as HR
import probe_cases as PC
import probe_vis_cases as PV
import ray_cases as RC
from pbrpathtracer_amd.probes import default_max_dist, fibonacci_dirs, grid_over_bounds, grid_positions

pytestmark = pytest.mark.gpu

F = np.float32
SEED, SAMPLE = (1 << 40) + 9, 2
FAR = 1e3                       # a max_dist no hit of the cases reaches
PASS_BYTES_DEFAULT = float(16 << 30)


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


_truth = {}


def _case(OB, case):
    """(arrays, positions, dirs, depth [P, D] of the mirror at (SAMPLE, SEED, key_base 0)) of a case of probe_cases.CASES; computed
    once, not to be modified"""
    if case not in _truth:
        arrays, _ = RC.scene(case)
        pos, dirs = PC.probes(case)
        _truth[case] = (arrays, pos, dirs, PV.depth_truth(OB, arrays, pos, dirs, SAMPLE, SEED, 0))
    return _truth[case]


def _bake(c, t, res, max_dist, **kw):
    return c.bake_probe_visibility(t[1], t[2], res, max_dist, SAMPLE, SEED, **kw)


# ---- 1. depth and moments equal the mirror ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(PC.CASES))
def test_depth_and_moments_equal_mirror(ctx, oracle_mod, case):
    """7 probes x 48 directions = 336 rays, not a multiple of 64; res 4 and 3; max_dist beyond every hit and at 0.8 of the median
    hit distance, where more than half of the hits are clamped"""
    t = _case(oracle_mod, case)
    want = t[3]
    hit = np.isfinite(want)
    near = float(F(0.8 * np.median(want[hit])))
    assert hit.mean() > 0.2 and (want[hit] > near).mean() > 0.5 and (want[hit] < near).any() and want[hit].max() < FAR
    ctx.upload_scene(t[0])
    for res, md in ((4, FAR), (3, near), (4, near)):
        depth, mom = _bake(ctx, t, res, md)
        assert depth.shape == (PC.P, PC.D) and mom.shape == (PC.P, res * res, 2) and depth.dtype == mom.dtype == F
        assert np.array_equal(depth, want), (case, int((depth != want).sum()))
        m = PV.moments(want, t[2], res, md)
        assert np.isfinite(m).all() and np.array_equal(mom, m), (case, res, md, int((mom != m).any(axis=2).sum()))
    # without a table of the caller's the moments come from the context's own
    none, mom2 = _bake(ctx, t, 4, near, want_depth=False)
    assert none is None and np.array_equal(mom2, m)
    if case == "s_opacity":
        # its opacity map decides depths: without it some of these rays stop nearer (the map is 0 or 1, so no draw is involved)
        bare = dict(t[0]); bare["materials"] = np.array(t[0]["materials"], copy=True)
        bare["materials"]["tex"][:, HR.OPACITY_SLOT] = -1
        nearer = PV.depth_truth(oracle_mod, bare, t[1], t[2], SAMPLE, SEED, 0)
        assert (nearer < want).any() and (nearer <= want).all()


def test_depth_equals_intersect_rays_sample_and_keys(ctx, oracle_mod):
    """random6000: the stochastic-opacity draws make sample, seed and key matter for some thirty of its 336 rays.  s_opacity cannot
    show that: its one opacity map holds 0 and 255 only, so every draw u in [0, 1) passes or fails whatever the key (its map does
    decide depths: test_depth_and_moments_equal_mirror).  2^32 - 100: the keys wrap inside the third probe."""
    t = _case(oracle_mod, "random6000")
    ctx.upload_scene(t[0])
    ro, rd = PC.expand(t[1], t[2])
    seen = []
    for sample, kb in ((SAMPLE, 0), (SAMPLE + 1, 0), (SAMPLE, 1000), (SAMPLE, 2 ** 32 - 100)):
        depth, mom = ctx.bake_probe_visibility(t[1], t[2], 4, FAR, sample, SEED, key_base=kb)
        want = ctx.intersect_rays(ro, rd, sample, SEED, key_base=kb)[1].reshape(PC.P, PC.D)
        assert np.array_equal(depth, want), (sample, kb)
        assert np.array_equal(mom, PV.moments(want, t[2], 4, FAR))
        seen.append(depth)
    assert np.array_equal(seen[0], t[3])
    assert np.array_equal(seen[3], PV.depth_truth(oracle_mod, t[0], t[1], t[2], SAMPLE, SEED, 2 ** 32 - 100))
    for other in seen[1:]:
        assert not np.array_equal(other, seen[0])
    assert not np.array_equal(ctx.bake_probe_visibility(t[1], t[2], 4, FAR, SAMPLE, SEED + 1)[0], seen[0])


# ---- 2. shapes, blocks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,D,res", [(1, 1, 4), (3, 65, 4), (4, 16, 1), (4, 16, 16), (2, 4099, 5), (70, 16, 2)])
def test_shapes(ctx, oracle_mod, P, D, res):
    """(1, 1, res 4): one ray.  (3, 65, res 4): one direction above the 64-ray group of hits_kernel and above the moments kernel's LDS
    chunk of 64 directions.  (4, 16, res 1) and (4, 16, res 16): exactly one group of rays, with 64 probes and one probe per
    workgroup of the moments kernel.  (2, 4099, res 5): 64 chunks of 64 directions and a rest of 3.  (70, 16, res 2): a full
    workgroup of 64 probes and one of 6."""
    arrays, _ = RC.scene("s_opacity")
    pos = RC.rays_in_box(arrays, P, 4)[0]
    dirs = fibonacci_dirs(D)
    want = PV.depth_truth(oracle_mod, arrays, pos, dirs, SAMPLE, SEED, 5)
    md = float(F(np.median(want[np.isfinite(want)]))) if np.isfinite(want).any() else 1.0
    ctx.upload_scene(arrays)
    depth, mom = ctx.bake_probe_visibility(pos, dirs, res, md, SAMPLE, SEED, key_base=5)
    m = PV.moments(want, dirs, res, md)
    assert depth.shape == (P, D) and mom.shape == (P, res * res, 2)
    assert np.array_equal(depth, want) and np.array_equal(mom, m)


def test_one_direction_has_unfaced_texels(ctx):
    """(P, D) = (1, 1) with a direction that hits: the texels that face away have sw = 0 and hold (max_dist, max_dist^2)"""
    arrays, _ = RC.scene("s_cornell")
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    pos = np.array([0.5 * (v.min(axis=0) + v.max(axis=0))], F)
    dirs = np.array([[0.0, -1.0, 0.0]], F)
    ctx.upload_scene(arrays)
    depth, mom = ctx.bake_probe_visibility(pos, dirs, 4, 50.0)
    assert np.isfinite(depth).all() and depth[0, 0] < 50.0
    m = PV.moments(depth, dirs, 4, 50.0)
    assert np.array_equal(mom, m)
    away = PV.texel_dirs(4)[:, 1] > 0
    assert away.sum() == 8 and (mom[0, away] == (F(50.0), F(2500.0))).all() and (mom[0, ~away, 0] == depth[0, 0]).all()


def test_blocks_of_probes(ctx):
    """"pass_bytes" at its smallest, 1 MiB: blocks of 4096 rays = 85 whole probes of 48 directions - 200 probes are three blocks, the
    last of 30"""
    arrays, _ = RC.scene("random300")
    pos = RC.rays_in_box(arrays, 200, 3)[0]
    dirs = fibonacci_dirs(48)
    ctx.upload_scene(arrays)
    depth, mom = ctx.bake_probe_visibility(pos, dirs, 3, 2.0, SAMPLE, SEED, key_base=2 ** 32 - 5000)
    ro, rd = PC.expand(pos, dirs)
    assert np.array_equal(depth.reshape(-1), ctx.intersect_rays(ro, rd, SAMPLE, SEED, key_base=2 ** 32 - 5000)[1])
    assert np.isfinite(depth).mean() > 0.3 and np.array_equal(mom, PV.moments(depth, dirs, 3, 2.0))
    try:
        ctx.set_option("pass_bytes", 1 << 20)
        depth2, mom2 = ctx.bake_probe_visibility(pos, dirs, 3, 2.0, SAMPLE, SEED, key_base=2 ** 32 - 5000)
        assert np.array_equal(depth2, depth) and np.array_equal(mom2, mom)
        _, mom3 = ctx.bake_probe_visibility(pos, dirs, 3, 2.0, SAMPLE, SEED, key_base=2 ** 32 - 5000, want_depth=False)
        assert np.array_equal(mom3, mom)
    finally:
        ctx.set_option("pass_bytes", PASS_BYTES_DEFAULT)


# ---- 3. independence, edits, state ------------------------------------------------------------------------------------------------
def test_independent_of_builder_leaf_size_flat_and_tiles(ctx, oracle_mod):
    try:
        t = _case(oracle_mod, "random6000")
        m = PV.moments(t[3], t[2], 4, 1.5)
        for device_build in (0, 1):
            for leaf_max in (1, 8):
                ctx.set_option("device_build", device_build); ctx.set_option("bvh_leaf_max", leaf_max)
                ctx.upload_scene(t[0])
                depth, mom = _bake(ctx, t, 4, 1.5)
                assert np.array_equal(depth, t[3]) and np.array_equal(mom, m), (device_build, leaf_max)
        ctx.set_option("bvh_leaf_max", 0)
        ctx.set_tile(1, 3)
        assert np.array_equal(_bake(ctx, t, 4, 1.5)[1], m)
        t = _case(oracle_mod, "s_cornell")
        m = PV.moments(t[3], t[2], 4, 1.5)
        ctx.upload_scene(t[0])
        for flat in (0, 1):
            for contract in (0, 1):
                ctx.set_option("flat", flat); ctx.set_option("contract", contract)
                depth, mom = _bake(ctx, t, 4, 1.5)
                assert np.array_equal(depth, t[3]) and np.array_equal(mom, m), (flat, contract)
    finally:
        ctx.set_option("bvh_leaf_max", 0); ctx.set_option("device_build", 1); ctx.set_option("flat", 1); ctx.set_option("contract", 0)
        ctx.set_tile(0, 1)


def test_geometry_edits_are_seen(ctx, oracle_mod):
    arrays, pos, dirs, want = _case(oracle_mod, "random300")
    ctx.upload_scene(arrays)
    moved = dict(arrays); moved["verts"] = arrays["verts"].copy()
    moved["verts"][:150] = (arrays["verts"][:150].reshape(-1, 3, 3) + np.array([0.3, 0.15, -0.2], F)).reshape(-1, 9)
    want_g = PV.depth_truth(oracle_mod, moved, pos, dirs, SAMPLE, SEED, 0)
    assert not np.array_equal(want_g, want)
    ctx.update_geometry(0, moved["verts"][:150])
    depth, mom = ctx.bake_probe_visibility(pos, dirs, 4, 2.0, SAMPLE, SEED)
    assert np.array_equal(depth, want_g) and np.array_equal(mom, PV.moments(want_g, dirs, 4, 2.0))


def test_leaves_frame_adaptive_and_feature_state_alone(ctx, oracle_mod):
    from pbrpathtracer_amd import ptk
    t = _case(oracle_mod, "random300")
    _, cam = RC.scene("random300")
    ctx.upload_scene(t[0]); ctx.set_camera(**cam); ctx.set_frame(40, 24, 4); ctx.set_tile(0, 1); ctx.reset()
    ctx.render_adaptive(0.05, 4, 2, 8, 3)
    ctx.render_features(ptk.FEAT_ALL, 1, 3)
    state = lambda: (ctx.read_accum(), ctx.samples(), ctx.read_sample_counts(), ctx.read_moments(), ctx.resolve_rgb8(),
                     *(ctx.read_feature(k) for k in range(len(ptk.FEAT_NAMES))))
    before = state()
    depth, mom = _bake(ctx, t, 4, 2.0)
    assert np.array_equal(depth, t[3]) and np.array_equal(mom, PV.moments(t[3], t[2], 4, 2.0))
    after = state()
    assert before[1] == after[1]
    for b, a in zip(before, after):
        assert np.array_equal(b, a, equal_nan=True)
    ctx.reset()


def test_needs_no_camera_and_no_frame_and_no_triangles(oracle_mod):
    from pbrpathtracer_amd import ptk
    t = _case(oracle_mod, "s_glass")
    c = ptk.Context(0)
    try:
        c.upload_scene(t[0])
        depth, mom = _bake(c, t, 4, 2.0)
        assert np.array_equal(depth, t[3]) and np.array_equal(mom, PV.moments(t[3], t[2], 4, 2.0))
        # a scene without triangles: every ray misses
        empty = {k: (np.asarray(v)[:0].copy() if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material") else np.asarray(v).copy())
                 for k, v in t[0].items()}
        empty["lights"] = np.zeros(0, np.int32)
        c.upload_scene(empty)
        depth, mom = _bake(c, t, 3, 2.5)
        assert np.isposinf(depth).all() and np.array_equal(mom, PV.moments(depth, t[2], 3, 2.5))
        assert (np.abs(mom[..., 0] - 2.5) < 1e-4).all()
    finally:
        c.close()


# ---- 4. the lookup equals numpy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(3, 2, 2), (1, 1, 1), (4, 1, 3)])
def test_lookup_equals_numpy(ctx, dims):
    import torch
    rng = np.random.default_rng(sum(dims))
    origin, spacing = (-1.0, 0.5, 2.0), (0.5, 1.25, 0.3)
    coefs = rng.uniform(-1, 2, (dims[2], dims[1], dims[0], 9, 3)).astype(F)
    pts, nrm = PC.queries(dims, origin, spacing, 1000, 9)
    assert np.isnan(pts).any() and np.isinf(pts).any()
    for res, bias in ((4, 0.0), (3, 0.05), (16, 0.05), (1, 0.0)):
        mom = PV.random_moments(dims, res, res)
        parts = []
        want = PV.irradiance_visible(dims, origin, spacing, coefs, res, mom, bias, pts, nrm, parts=parts)
        vis = np.stack([p[3] for p in parts])
        assert np.isfinite(want).all() and (vis == 1).any() and ((vis > 0) & (vis < 1)).any()
        if mom.size >= 2 * 100:                  # (enough texels for the rare kinds to be there)
            assert (mom[..., 1] < mom[..., 0] * mom[..., 0]).any() and (mom[..., 0] == 0).any() and (vis == 0).any()
        got = ctx.probes_irradiance_visible(dims, origin, spacing, coefs, res, mom, pts, nrm, bias)
        assert got.shape == (1000, 3) and got.dtype == F
        assert np.array_equal(got, want), (res, bias, int((got != want).any(axis=1).sum()))
        t = [torch.from_numpy(a).cuda() for a in (coefs, mom, pts, nrm)]
        torch.cuda.synchronize()
        dev = ctx.probes_irradiance_visible(dims, origin, spacing, t[0], res, t[1], t[2], t[3], bias)
        ctx.synchronize()
        assert np.array_equal(dev.cpu().numpy(), want)
    # it is another function than the plain lookup
    assert not np.array_equal(got, PC.irradiance(dims, origin, spacing, coefs, pts, nrm))


def test_two_rooms_on_the_gpu(ctx, oracle_mod):
    """the CPU test's scene end to end through the kernels: the same bits as the mirror, and no leak"""
    arrays = PV.two_rooms()
    dims, origin, spacing = (2, 1, 1), (-1.0, 0.0, 0.0), (2.0, 1.0, 1.0)
    pos, dirs = grid_positions(dims, origin, spacing), fibonacci_dirs(48)
    ctx.upload_scene(arrays)
    depth, mom = ctx.bake_probe_visibility(pos, dirs, 4, 6.0, 0, 11)
    want = PV.depth_truth(oracle_mod, arrays, pos, dirs, 0, 11, 0)
    assert np.array_equal(depth, want) and np.array_equal(mom, PV.moments(want, dirs, 4, 6.0))
    _, coefs = ctx.bake_probes(pos, dirs, 4, 0, 4, 11, 0.1)
    q = np.zeros((9, 3), F); q[:, 0] = np.linspace(0.3, 0.7, 9)
    n = np.tile(np.array([0.0, 1.0, 0.0], F), (9, 1))
    got = ctx.probes_irradiance_visible(dims, origin, spacing, coefs, 4, mom, q, n)
    assert np.array_equal(got, PV.irradiance_visible(dims, origin, spacing, coefs, 4, mom, 0.0, q, n))
    plain = ctx.probes_irradiance(dims, origin, spacing, coefs, q, n)
    assert (plain > 0).all() and (got < plain).all()


# ---- 5. the device entries --------------------------------------------------------------------------------------------------------
def test_device_entries_and_caller_stream(oracle_mod):
    import torch
    from pbrpathtracer_amd import ptk
    arrays, pos, dirs, want = _case(oracle_mod, "random300")
    m = PV.moments(want, dirs, 4, 2.0)
    dev = torch.device("cuda:0")
    dims, origin, spacing = (7, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)          # the seven probes as a row
    rng = np.random.default_rng(2)
    coefs = rng.uniform(-1, 2, (7, 9, 3)).astype(F)
    pts, nrm = PC.queries(dims, origin, spacing, 200, 6)
    want_E = PV.irradiance_visible(dims, origin, spacing, coefs, 4, m, 0.05, pts, nrm)
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays)
        t_pos, t_dirs = torch.from_numpy(pos).to(dev), torch.from_numpy(dirs).to(dev)
        torch.cuda.synchronize()
        got_d, got_m = c.bake_probe_visibility(t_pos, t_dirs, 4, 2.0, SAMPLE, SEED)
        c.synchronize()
        assert isinstance(got_d, torch.Tensor) and tuple(got_d.shape) == (PC.P, PC.D) and tuple(got_m.shape) == (PC.P, 16, 2)
        assert np.array_equal(got_d.cpu().numpy(), want) and np.array_equal(got_m.cpu().numpy(), m)
        none, m2 = c.bake_probe_visibility(t_pos, t_dirs, 4, 2.0, SAMPLE, SEED, want_depth=False)        # the context's table
        c.synchronize()
        assert none is None and np.array_equal(m2.cpu().numpy(), m)
        s = torch.cuda.Stream(device=dev)
        c.set_stream(s.cuda_stream)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            f_pos = torch.zeros_like(t_pos)
            f_pos.copy_(t_pos)
            r_d, r_m = c.bake_probe_visibility(f_pos, t_dirs, 4, 2.0, SAMPLE, SEED)
            snap = r_m.clone()
            E = c.probes_irradiance_visible(dims, origin, spacing, torch.from_numpy(coefs).to(dev, non_blocking=False), 4, r_m,
                                            torch.from_numpy(pts).to(dev, non_blocking=False),
                                            torch.from_numpy(nrm).to(dev, non_blocking=False), 0.05)
            E_snap = E.clone()
        s.synchronize()
        assert np.array_equal(snap.cpu().numpy(), m) and np.array_equal(r_d.cpu().numpy(), want)
        assert np.array_equal(E_snap.cpu().numpy(), want_E)
    finally:
        c.close()


# ---- 6. arguments -----------------------------------------------------------------------------------------------------------------
def test_arguments(ctx, oracle_mod):
    import ctypes as C
    from pbrpathtracer_amd import ptk
    arrays, pos, dirs, want = _case(oracle_mod, "s_cornell")
    L = ptk.load()
    P, D, R = PC.P, PC.D, 4
    dep = np.full((P, D), 7.0, F); mo = np.full((P, R * R, 2), 7.0, F)
    pp, pd, pz, pm = pos.ctypes.data, dirs.ctypes.data, dep.ctypes.data, mo.ctypes.data
    BAD = -1
    bakes = (L.ptk_bake_probe_visibility, L.ptk_bake_probe_visibility_device)
    inf, nan = float("inf"), float("nan")

    def err(c):
        return L.ptk_last_error(c.h).decode()

    fresh = ptk.Context(0)
    try:
        for fn in bakes:
            assert fn(fresh.h, P, pp, D, pd, R, 2.0, 0, 0, 0, pz, pm) == BAD and "ptk_upload_scene" in err(fresh)
        # the lookup needs no scene
        coefs = np.ones((1, 9, 3), F); m1 = PV.random_moments((1, 1, 1), R, 1)
        g = PV.irradiance_visible((1, 1, 1), (0, 0, 0), (1, 1, 1), coefs, R, m1, 0.0, pos, dirs[:P])
        assert np.array_equal(fresh.probes_irradiance_visible((1, 1, 1), (0, 0, 0), (1, 1, 1), coefs, R, m1, pos, dirs[:P]), g)
    finally:
        fresh.close()
    ctx.upload_scene(arrays)
    for fn in bakes:
        assert fn(None, P, pp, D, pd, R, 2.0, 0, 0, 0, pz, pm) == BAD                                            # null context
        assert fn(ctx.h, -1, pp, D, pd, R, 2.0, 0, 0, 0, pz, pm) == BAD and "negative" in err(ctx)
        assert fn(ctx.h, P, pp, -1, pd, R, 2.0, 0, 0, 0, pz, pm) == BAD and "negative" in err(ctx)
        for d in (0, 65537):
            assert fn(ctx.h, P, pp, d, pd, R, 2.0, 0, 0, 0, pz, pm) == BAD and "65536" in err(ctx)
        assert fn(ctx.h, 32768, pp, 65536, pd, R, 2.0, 0, 0, 0, pz, pm) == BAD and "2^31" in err(ctx)
        for a, b, c in ((None, pd, pm), (pp, None, pm), (pp, pd, None)):
            assert fn(ctx.h, P, a, D, b, R, 2.0, 0, 0, 0, pz, c) == BAD and "null" in err(ctx)
        for res in (0, 17, -4):
            assert fn(ctx.h, P, pp, D, pd, res, 2.0, 0, 0, 0, pz, pm) == BAD and "res" in err(ctx)
        for md in (inf, -inf, nan, 0.0, -1.0, 2e18):
            assert fn(ctx.h, P, pp, D, pd, R, md, 0, 0, 0, pz, pm) == BAD and "max_dist" in err(ctx)
        assert fn(ctx.h, 0, None, 0, None, R, 2.0, 0, 0, 0, None, None) == 0                                     # zero probes
    assert (dep == 7.0).all() and (mo == 7.0).all()
    assert L.ptk_bake_probe_visibility(ctx.h, P, pp, D, pd, R, 1e18, SAMPLE, SEED, 0, None, pm) == 0            # depth is optional
    assert np.array_equal(mo, PV.moments(want, dirs, R, 1e18)) and (dep == 7.0).all()
    ms = ctx.last_probe_visibility_ms()
    assert ms["raygen_ms"] > 0 and ms["hits_ms"] > 0 and ms["moments_ms"] > 0
    assert L.ptk_last_probe_visibility_ms(None, None, None, None) == BAD

    I3, F3 = C.c_int32 * 3, C.c_float * 3
    f32 = C.c_float
    co = np.ones((P, 9, 3), F)
    out = np.full((P, 3), 7.0, F)
    nrm = np.ascontiguousarray(dirs[:P])
    pc, po, pn = co.ctypes.data, out.ctypes.data, nrm.ctypes.data
    for fn in (L.ptk_probes_irradiance_visible, L.ptk_probes_irradiance_visible_device):
        ok = (I3(7, 1, 1), F3(0, 0, 0), F3(1, 1, 1))
        assert fn(None, *ok, pc, R, pm, f32(0), P, pp, pn, po) == BAD
        assert fn(ctx.h, *ok, pc, R, pm, f32(0), -1, pp, pn, po) == BAD and "negative" in err(ctx)
        for dims in ((0, 1, 1), (7, -1, 1), (7, 1, 0)):
            assert fn(ctx.h, I3(*dims), ok[1], ok[2], pc, R, pm, f32(0), P, pp, pn, po) == BAD and "dims" in err(ctx)
        for sp in ((0, 1, 1), (1, -1, 1), (1, 1, inf), (nan, 1, 1)):
            assert fn(ctx.h, ok[0], ok[1], F3(*sp), pc, R, pm, f32(0), P, pp, pn, po) == BAD and "spacing" in err(ctx)
        for og in ((inf, 0, 0), (0, nan, 0), (0, 0, -inf)):
            assert fn(ctx.h, ok[0], F3(*og), ok[2], pc, R, pm, f32(0), P, pp, pn, po) == BAD and "origin" in err(ctx)
        for a, m, b, c, d in ((None, pm, pp, pn, po), (pc, None, pp, pn, po), (pc, pm, None, pn, po), (pc, pm, pp, None, po),
                              (pc, pm, pp, pn, None)):
            assert fn(ctx.h, *ok, a, R, m, f32(0), P, b, c, d) == BAD and "null" in err(ctx)
        assert fn(ctx.h, None, ok[1], ok[2], pc, R, pm, f32(0), P, pp, pn, po) == BAD
        for res in (0, 17, -4):
            assert fn(ctx.h, *ok, pc, res, pm, f32(0), P, pp, pn, po) == BAD and "res" in err(ctx)
        for nb in (inf, -inf, nan):
            assert fn(ctx.h, *ok, pc, R, pm, f32(nb), P, pp, pn, po) == BAD and "normal_bias" in err(ctx)
        assert fn(ctx.h, *ok, None, R, None, f32(0), 0, None, None, None) == 0                                   # zero points
    assert (out == 7.0).all()


# ---- 7. host class and command line -----------------------------------------------------------------------------------------------
def test_host_class_and_visibility_cli(oracle_mod, tmp_path):
    from pbrpathtracer_amd import render, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    pts, _, _ = S.build_config("C1", str(tmp_path), width=32, height=24, depth=4)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    pt.SetSeed(5)
    arrays = pt.StagedScene()
    dims, D, res = (2, 1, 2), 16, 4
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    origin, spacing = grid_over_bounds(v.min(axis=0), v.max(axis=0), dims)
    pos, dirs, md = grid_positions(dims, origin, spacing), fibonacci_dirs(D), default_max_dist(spacing)
    want_d = PV.depth_truth(oracle_mod, arrays, pos, dirs, 0, 5, 0)
    want_m = PV.moments(want_d, dirs, res, md)
    got_d, got_m = pt.BakeProbeVisibility(pos, dirs, res, md)                    # no resolution set, no render before it
    assert pt.LastError() == "" and np.array_equal(got_d, want_d) and np.array_equal(got_m, want_m) and np.isfinite(want_d).any()
    got_d7, _ = pt.BakeProbeVisibility(pos, dirs, res, md, sample=3, key_base=7)
    assert np.array_equal(got_d7, PV.depth_truth(oracle_mod, arrays, pos, dirs, 3, 5, 7))
    rng = np.random.default_rng(1)
    coefs = rng.uniform(0, 1, (len(pos), 9, 3)).astype(F)
    qp, qn = PC.queries(dims, origin, spacing, 300, 2)
    want_E = PV.irradiance_visible(dims, origin, spacing, coefs, res, want_m, 0.02, qp, qn)
    assert np.array_equal(pt.SampleProbesVisible(dims, origin, spacing, coefs, res, got_m, qp, qn, 0.02), want_E)
    pt.close()
    npz = str(tmp_path / "probes.npz")
    assert render.main([pts, "--bake-probes", "2", "1", "2", "--probe-dirs", "16", "--spp", "3", "--seed", "5", "--probe-visibility", "4",
                        "-o", npz]) == 0
    z = np.load(npz)
    assert z["moments"].shape == (2, 1, 2, 16, 2) and z["moments"].dtype == F and np.array_equal(z["moments"].reshape(-1, 16, 2), want_m)
    assert int(z["res"]) == 4 and float(z["max_dist"]) == md and z["coefs"].shape == (2, 1, 2, 9, 3)
    assert np.array_equal(z["dims"], dims) and np.array_equal(z["origin"], origin) and np.array_equal(z["spacing"], spacing)
    npz2 = str(tmp_path / "probes2.npz")
    assert render.main([pts, "--bake-probes", "2", "1", "2", "--probe-dirs", "16", "--spp", "3", "--seed", "5", "--probe-visibility", "3",
                        "--probe-max-dist", "0.75", "-o", npz2]) == 0
    z2 = np.load(npz2)
    assert float(z2["max_dist"]) == 0.75 and np.array_equal(z2["moments"].reshape(-1, 9, 2), PV.moments(want_d, dirs, 3, 0.75))
    assert np.array_equal(z2["coefs"], z["coefs"])
    # misuse is an error line and return code 1, not a traceback
    for bad in (["--bake-probes", "2", "1", "2", "--probe-visibility", "17"], ["--bake-probes", "2", "1", "2", "--probe-max-dist", "1.0"],
                ["--bake-probes", "2", "1", "2", "--probe-visibility", "4", "--probe-max-dist", "0"], ["--probe-visibility", "4"]):
        assert render.main([pts, *bad, "--spp", "1", "-o", str(tmp_path / "bad.npz")]) == 1
    assert not (tmp_path / "bad.npz").exists()
    # the file round-trips into the lookup
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    try:
        got = c.probes_irradiance_visible(z["dims"], z["origin"], z["spacing"], z["coefs"], int(z["res"]), z["moments"], qp, qn, 0.02)
        assert np.array_equal(got, PV.irradiance_visible(dims, origin, spacing, z["coefs"], 4, want_m, 0.02, qp, qn))
    finally:
        c.close()
