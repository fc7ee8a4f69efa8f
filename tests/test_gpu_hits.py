"""Closest-hit and occlusion queries for caller-supplied rays (include/ptk.h ptk_intersect_rays, ptk_occluded_rays)
against the numpy mirror of the candidate rule (tests/hit_rule.py, which tests/test_hits_cpu.py holds to the CPU oracle) and
against the oracle's own camera records, bit for bit: whatever the ray count, the cut of the ray set, the builder, the leaf size,
the "flat" option and the tile split.  Every comparison is np.array_equal unless it says otherwise."""
import numpy as np
import pytest

import feature_truth as FT
import hit_rule as HR
import ray_cases as RC

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED, SAMPLE = (1 << 40) + 9, 3


def n_rays(case):
    return 400 if case == "random6000" else 1000


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


_mirror = {}


def _case(OB, case):
    """(arrays, ro, rd, (tri, t, bary, material) of the mirror) of a case at (SEED, SAMPLE, key_base 0); computed once, not to be
    modified"""
    if case not in _mirror:
        arrays, _ = RC.scene(case)
        n = n_rays(case)
        ro, rd = RC.rays_in_box(arrays, n, 5)
        _mirror[case] = (arrays, ro, rd, HR.mirror(OB, arrays, ro, rd, HR.ray_keys(SEED, 0, n, SAMPLE)))
    return _mirror[case]


def _same(got, want):
    return all(np.array_equal(g, w) and g.dtype == w.dtype and g.shape == w.shape for g, w in zip(got, want))


# ---- 1. hits equal the mirror --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.CASES)
def test_hits_equal_mirror(ctx, oracle_mod, case):
    arrays, ro, rd, want = _case(oracle_mod, case)
    ctx.upload_scene(arrays)
    got = ctx.intersect_rays(ro, rd, SAMPLE, SEED)
    for name, g, w in zip(("tri", "t", "bary", "material"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (case, name)
        assert np.array_equal(g, w), (case, name, int((g != w).sum()))
    assert 0.15 <= (got[0] >= 0).mean() <= 0.85


# ---- 2. camera rays against the oracle itself, stochastic opacity included -----------------------------------------------------
@pytest.mark.parametrize("case", ("s_opacity", "random16"))
def test_camera_rays_equal_oracle_and_feature_planes(ctx, oracle_mod, case):
    from pbrpathtracer_amd import ptk
    arrays, cam = RC.scene(case)
    W, H, seed, sample = 32, 24, 21, 2
    rec = FT.camera_records(oracle_mod, arrays, cam, W, H, seed, sample)
    assert rec["seen"].all()
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, 4); ctx.set_tile(0, 1); ctx.reset()
    tri, t, bary, mat = ctx.intersect_rays(rec["ro"], rec["rd"], sample, seed, key_base=0)
    assert np.array_equal(tri, rec["tri"]) and np.array_equal(t, rec["t"])
    assert (tri >= 0).any()
    mask = (1 << ptk.FEAT_TRIANGLE) | (1 << ptk.FEAT_DEPTH) | (1 << ptk.FEAT_BARY) | (1 << ptk.FEAT_MATERIAL)
    ctx.render_features(mask, sample, seed)
    top_down = lambda f: ctx.read_feature(f)[::-1].reshape(W * H, -1).squeeze()
    assert np.array_equal(top_down(ptk.FEAT_TRIANGLE), tri)
    assert np.array_equal(top_down(ptk.FEAT_DEPTH), t)
    assert np.array_equal(top_down(ptk.FEAT_BARY), bary)
    assert np.array_equal(top_down(ptk.FEAT_MATERIAL), mat)
    # another sample draws other opacities somewhere (or the check above would not see the key)
    other = FT.camera_records(oracle_mod, arrays, cam, W, H, seed, sample + 1)
    tri2, t2, _, _ = ctx.intersect_rays(other["ro"], other["rd"], sample + 1, seed)
    assert np.array_equal(tri2, other["tri"]) and np.array_equal(t2, other["t"])


# ---- 3. occlusion --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("random16", "random300"))
def test_occlusion(ctx, oracle_mod, case):
    arrays, ro, rd, (tri, t, _, _) = _case(oracle_mod, case)
    n = len(ro)
    ctx.upload_scene(arrays)
    hit = tri >= 0
    occ = lambda tmax: ctx.occluded_rays(ro, rd, tmax, SAMPLE, SEED)
    free = occ(None)
    assert free.dtype == np.uint8 and free.shape == (n,)
    assert np.array_equal(free, hit.astype(np.uint8))
    assert np.array_equal(occ(np.full(n, np.inf, F32)), free)
    assert (occ(t)[hit] == 0).all() and (occ(t) == 0).all()                       # strict: t_hit < t_hit is false
    nxt = np.nextafter(t, F32(np.inf))
    assert (occ(nxt)[hit] == 1).all() and (occ(nxt)[~hit] == 0).all()
    for bad in (np.nan, 0.0, -0.0, -1.0, -np.inf):
        assert (occ(np.full(n, bad, F32)) == 0).all(), bad
    rng = np.random.default_rng(11)
    tmax = rng.uniform(0.0, 2.0 * float(np.median(t[hit])), n).astype(F32)
    got = occ(tmax)
    assert np.array_equal(got, HR.occluded(t, tmax))
    assert got.mean() >= 0.1 and (1 - got).mean() >= 0.1
    # a mixture of every kind of bound in one call
    mix = tmax.copy(); mix[0::5] = np.nan; mix[1::5] = np.inf; mix[2::5] = 0.0; mix[3::5] = t[3::5]
    assert np.array_equal(occ(mix), HR.occluded(t, mix))


# ---- 4. ragged counts ----------------------------------------------------------------------------------------------------------
def test_ragged_counts(ctx, oracle_mod):
    arrays, ro, rd, want = _case(oracle_mod, "random300")
    ctx.upload_scene(arrays)
    rng = np.random.default_rng(12)
    tmax = rng.uniform(0.0, 2.0 * float(np.median(want[1][want[0] >= 0])), len(ro)).astype(F32)
    want_occ = HR.occluded(want[1], tmax)
    for n in (1, 63, 64, 65, 255, 256, 257):
        assert _same(ctx.intersect_rays(ro[:n], rd[:n], SAMPLE, SEED), [w[:n] for w in want]), n
        assert np.array_equal(ctx.occluded_rays(ro[:n], rd[:n], tmax[:n], SAMPLE, SEED), want_occ[:n]), n
        assert np.array_equal(ctx.occluded_rays(ro[:n], rd[:n], None, SAMPLE, SEED), (want[0][:n] >= 0).astype(np.uint8)), n


# ---- 5. cutting and wrapping ---------------------------------------------------------------------------------------------------
def test_cutting_and_key_wrap(ctx, oracle_mod):
    arrays, ro, rd, want = _case(oracle_mod, "random16")
    ctx.upload_scene(arrays)
    whole = ctx.intersect_rays(ro, rd, SAMPLE, SEED)
    whole_occ = ctx.occluded_rays(ro, rd, None, SAMPLE, SEED)
    assert _same(whole, want)
    differs = False
    for a, b in ((0, 300), (300, 1000), (77, 141), (640, 641)):
        part = ctx.intersect_rays(ro[a:b], rd[a:b], SAMPLE, SEED, key_base=a)
        assert _same(part, [w[a:b] for w in whole]), (a, b)
        assert np.array_equal(ctx.occluded_rays(ro[a:b], rd[a:b], None, SAMPLE, SEED, key_base=a), whole_occ[a:b]), (a, b)
        if a:
            differs |= not np.array_equal(ctx.intersect_rays(ro[a:b], rd[a:b], SAMPLE, SEED)[0], whole[0][a:b])
    assert differs                                                                # the key base counts
    # RNG pixels 2^32 - 10 ... 2^32 - 1, then 0, 1, ...
    kb = 2 ** 32 - 10
    wrapped = ctx.intersect_rays(ro, rd, SAMPLE, SEED, key_base=kb)
    assert _same([w[10:] for w in wrapped], ctx.intersect_rays(ro[10:], rd[10:], SAMPLE, SEED, key_base=0))
    assert _same(wrapped, HR.mirror(oracle_mod, arrays, ro, rd, HR.ray_keys(SEED, kb, len(ro), SAMPLE)))
    wrapped_occ = ctx.occluded_rays(ro, rd, None, SAMPLE, SEED, key_base=kb)
    assert np.array_equal(wrapped_occ[10:], ctx.occluded_rays(ro[10:], rd[10:], None, SAMPLE, SEED, key_base=0))


# ---- 6. independence -----------------------------------------------------------------------------------------------------------
def test_independent_of_builder_leaf_size_flat_and_tiles(ctx, oracle_mod):
    try:
        arrays, ro, rd, want = _case(oracle_mod, "random6000")
        want_occ = (want[0] >= 0).astype(np.uint8)
        rng = np.random.default_rng(13)
        tmax = rng.uniform(0.0, 2.0 * float(np.median(want[1][want[0] >= 0])), len(ro)).astype(F32)
        for device_build in (0, 1):
            for leaf_max in (1, 8):
                ctx.set_option("device_build", device_build); ctx.set_option("bvh_leaf_max", leaf_max)
                ctx.upload_scene(arrays)
                assert ctx.upload_timing()["built_on_device"] == bool(device_build)
                assert _same(ctx.intersect_rays(ro, rd, SAMPLE, SEED), want), (device_build, leaf_max)
                assert np.array_equal(ctx.occluded_rays(ro, rd, None, SAMPLE, SEED), want_occ), (device_build, leaf_max)
                assert np.array_equal(ctx.occluded_rays(ro, rd, tmax, SAMPLE, SEED), HR.occluded(want[1], tmax)), (device_build, leaf_max)
        ctx.set_option("bvh_leaf_max", 0)
        arrays, ro, rd, want = _case(oracle_mod, "random16")
        ctx.upload_scene(arrays)
        for flat in (0, 1):
            ctx.set_option("flat", flat)
            assert _same(ctx.intersect_rays(ro, rd, SAMPLE, SEED), want), flat
        ctx.set_tile(1, 3)
        assert _same(ctx.intersect_rays(ro, rd, SAMPLE, SEED), want)
        assert np.array_equal(ctx.occluded_rays(ro, rd, None, SAMPLE, SEED), (want[0] >= 0).astype(np.uint8))
    finally:
        ctx.set_option("bvh_leaf_max", 0); ctx.set_option("device_build", 1); ctx.set_option("flat", 1); ctx.set_tile(0, 1)


# ---- 7. tie and epsilon --------------------------------------------------------------------------------------------------------
def _two_triangles(verts):
    """a scene of the triangles `verts` [n, 9] with the records of s_cornell's first ones"""
    full, _ = RC.scene("s_cornell")
    n = len(verts)
    a = {k: (np.asarray(v)[:n].copy() if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material") else np.asarray(v).copy())
         for k, v in full.items()}
    a["verts"] = np.asarray(verts, F32).reshape(n, 9)
    a["lights"] = np.zeros(0, np.int32)
    return a


def test_tie_and_epsilon(ctx, oracle_mod):
    tri0 = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    arrays = _two_triangles([tri0, tri0])
    ctx.upload_scene(arrays)
    ro = np.array([[0.25, 0.25, 1.0], [0.25, 0.25, -2.0], [0.25, 0.25, 0.0], [0.25, 0.25, 0.0], [0.25, 0.25, 5e-6], [0.25, 0.25, 1e-3]], F32)
    rd = np.array([[0, 0, -1], [0, 0, 1], [0, 0, 1], [0, 0, -1], [0, 0, -1], [0, 0, -1]], F32)
    tri, t, bary, mat = ctx.intersect_rays(ro, rd)
    # two identical coplanar triangles: the smaller index; a ray that starts on (or within 1e-5 of) a triangle does not hit it
    assert tri.tolist() == [0, 0, -1, -1, -1, 0]
    assert t[0] == 1.0 and t[1] == 2.0 and np.isinf(t[2:5]).all() and t[5] == F32(1e-3)
    assert np.array_equal(bary[0], [0.25, 0.25]) and (bary[2:5] == 0).all() and mat[0] == arrays["material"][0] and (mat[2:5] == -1).all()
    assert _same((tri, t, bary, mat), HR.mirror(oracle_mod, arrays, ro, rd, HR.ray_keys(0, 0, len(ro), 0)))
    assert ctx.occluded_rays(ro, rd).tolist() == [1, 1, 0, 0, 0, 1]
    # the order of the pair does not matter, and the second one alone is triangle 1 once the first moves away
    moved = _two_triangles([[0, 0, 9, 1, 0, 9, 0, 1, 9], tri0])
    ctx.upload_scene(moved)
    assert ctx.intersect_rays(ro[:1], rd[:1])[0].tolist() == [1]


# ---- 8. edits are seen ---------------------------------------------------------------------------------------------------------
def test_geometry_edits_are_seen(ctx, oracle_mod):
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, want = _case(oracle_mod, "random300")
    ctx.upload_scene(arrays)
    assert _same(ctx.intersect_rays(ro, rd, SAMPLE, SEED), want)
    n = len(arrays["verts"])
    a, b = n // 3, (2 * n) // 3
    moved = dict(arrays); moved["verts"] = np.array(arrays["verts"], F32, copy=True).reshape(n, 9)
    moved["verts"][a:b] = (moved["verts"][a:b].reshape(-1, 3, 3) + np.array([0.3, 0.15, -0.2], F32)).reshape(-1, 9)
    ctx.update_geometry(a, moved["verts"][a:b])
    edited = ctx.intersect_rays(ro, rd, SAMPLE, SEED)
    edited_occ = ctx.occluded_rays(ro, rd, None, SAMPLE, SEED)
    assert not np.array_equal(edited[0], want[0])
    fresh = ptk.Context(0)
    try:
        fresh.upload_scene(moved)
        assert _same(edited, fresh.intersect_rays(ro, rd, SAMPLE, SEED))
        assert np.array_equal(edited_occ, fresh.occluded_rays(ro, rd, None, SAMPLE, SEED))
    finally:
        fresh.close()
    assert _same(edited, HR.mirror(oracle_mod, moved, ro, rd, HR.ray_keys(SEED, 0, len(ro), SAMPLE)))


# ---- 9. state left alone; the device entries -----------------------------------------------------------------------------------
def test_leaves_the_frame_state_alone(ctx, oracle_mod):
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, want = _case(oracle_mod, "random300")
    _, cam = RC.scene("random300")
    W, H = 40, 24
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, 4); ctx.set_tile(0, 1); ctx.reset()
    ctx.render_adaptive(0.05, 4, 2, 8, 3)
    ctx.render_features(ptk.FEAT_ALL, 0, 3)
    state = lambda: [ctx.read_accum(), np.array(ctx.samples()), ctx.read_sample_counts(), ctx.resolve_rgb8()] + \
        [ctx.read_feature(k) for k in range(len(ptk.FEAT_NAMES))]
    before = state()
    assert _same(ctx.intersect_rays(ro, rd, SAMPLE, SEED), want)                  # legal after render_adaptive
    assert np.array_equal(ctx.occluded_rays(ro, rd, None, SAMPLE, SEED), (want[0] >= 0).astype(np.uint8))
    for b, a in zip(before, state()):
        assert np.array_equal(b, a, equal_nan=b.dtype.kind == "f")
    with pytest.raises(ptk.PtkError):
        ctx.render(8, 1, 3)                                                       # (a plain render is not, until the next reset)
    ctx.reset()


def test_needs_no_camera_and_no_frame(oracle_mod):
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, want = _case(oracle_mod, "s_glass")
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays)
        assert _same(c.intersect_rays(ro, rd, SAMPLE, SEED), want)
        assert np.array_equal(c.occluded_rays(ro, rd, None, SAMPLE, SEED), (want[0] >= 0).astype(np.uint8))
        assert c.last_hits_ms() > 0
    finally:
        c.close()


def test_device_entries_and_caller_stream(oracle_mod):
    import torch
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, want = _case(oracle_mod, "random300")
    n = len(ro)
    rng = np.random.default_rng(14)
    tmax = rng.uniform(0.0, 2.0 * float(np.median(want[1][want[0] >= 0])), n).astype(F32)
    dev = torch.device("cuda:0")
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays)
        host = c.intersect_rays(ro, rd, SAMPLE, SEED)
        host_occ = c.occluded_rays(ro, rd, tmax, SAMPLE, SEED)
        assert _same(host, want) and np.array_equal(host_occ, HR.occluded(want[1], tmax))
        t_ro, t_rd, t_tm = (torch.from_numpy(x).to(dev) for x in (ro, rd, tmax))
        torch.cuda.synchronize()
        out = c.intersect_rays(t_ro, t_rd, SAMPLE, SEED)
        occ = c.occluded_rays(t_ro, t_rd, t_tm, SAMPLE, SEED)
        occ_free = c.occluded_rays(t_ro, t_rd, None, SAMPLE, SEED)
        c.synchronize()
        assert all(isinstance(o, torch.Tensor) and o.device == t_ro.device for o in out + (occ,))
        assert [tuple(o.shape) for o in out] == [(n,), (n,), (n, 2), (n,)] and occ.dtype == torch.uint8
        assert _same([o.cpu().numpy() for o in out], host)
        assert np.array_equal(occ.cpu().numpy(), host_occ) and np.array_equal(occ_free.cpu().numpy(), (want[0] >= 0).astype(np.uint8))
        # on a caller's stream, with no host wait: the inputs are filled on that stream behind a long kernel, the result is read on it
        s = torch.cuda.Stream(device=dev)
        c.set_stream(s.cuda_stream)
        big = torch.randn(2048, 2048, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            f_ro, f_rd, f_tm = torch.zeros_like(t_ro), torch.zeros_like(t_rd), torch.zeros_like(t_tm)
            for _ in range(8):
                big = big @ big * 1e-3
            f_ro.copy_(t_ro); f_rd.copy_(t_rd); f_tm.copy_(t_tm)
            res = [o.clone() for o in c.intersect_rays(f_ro, f_rd, SAMPLE, SEED)]
            res_occ = c.occluded_rays(f_ro, f_rd, f_tm, SAMPLE, SEED).clone()
        s.synchronize()
        assert _same([o.cpu().numpy() for o in res], host) and np.array_equal(res_occ.cpu().numpy(), host_occ)
    finally:
        c.close()


# ---- 10. arguments -------------------------------------------------------------------------------------------------------------
def test_arguments(ctx, oracle_mod):
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, want = _case(oracle_mod, "s_cornell")
    L = ptk.load()
    n = 10
    o, d = ro[:n].copy(), rd[:n].copy()
    tri = np.full(n, 77, np.int32); t = np.full(n, 7.0, F32); bary = np.full((n, 2), 7.0, F32); mat = np.full(n, 77, np.int32)
    occ = np.full(n, 7, np.uint8)
    po, pd = o.ctypes.data, d.ctypes.data
    outs = (tri.ctypes.data, t.ctypes.data, bary.ctypes.data, mat.ctypes.data)
    pocc = occ.ctypes.data
    BAD = -1
    hit_fns = (L.ptk_intersect_rays, L.ptk_intersect_rays_device)
    occ_fns = (L.ptk_occluded_rays, L.ptk_occluded_rays_device)

    def untouched():
        return (tri == 77).all() and (t == 7).all() and (bary == 7).all() and (mat == 77).all() and (occ == 7).all()

    fresh = ptk.Context(0)
    try:
        for fn in hit_fns:
            assert fn(fresh.h, n, po, pd, 0, 0, 0, *outs) == BAD                        # before ptk_upload_scene
        for fn in occ_fns:
            assert fn(fresh.h, n, po, pd, None, 0, 0, 0, pocc) == BAD
    finally:
        fresh.close()
    ctx.upload_scene(arrays)
    for fn in hit_fns:
        assert fn(None, n, po, pd, 0, 0, 0, *outs) == BAD                               # null context
        assert fn(ctx.h, -1, po, pd, 0, 0, 0, *outs) == BAD                             # negative count
        assert fn(ctx.h, n, None, pd, 0, 0, 0, *outs) == BAD                            # null rays
        assert fn(ctx.h, n, po, None, 0, 0, 0, *outs) == BAD
        assert fn(ctx.h, n, po, pd, 0, 0, 0, None, None, None, None) == BAD             # no output at all
        assert fn(ctx.h, 0, None, None, 0, 0, 0, None, None, None, None) == BAD
        assert fn(ctx.h, 0, None, None, 0, 0, 0, *outs) == 0                            # no rays: nothing to do
    for fn in occ_fns:
        assert fn(None, n, po, pd, None, 0, 0, 0, pocc) == BAD
        assert fn(ctx.h, -1, po, pd, None, 0, 0, 0, pocc) == BAD
        assert fn(ctx.h, n, None, pd, None, 0, 0, 0, pocc) == BAD
        assert fn(ctx.h, n, po, None, None, 0, 0, 0, pocc) == BAD
        assert fn(ctx.h, n, po, pd, None, 0, 0, 0, None) == BAD                         # null occluded
        assert fn(ctx.h, 0, None, None, None, 0, 0, 0, None) == 0
    assert L.ptk_last_hits_ms(None, None) == BAD
    ctx.synchronize()
    assert untouched()                                                                  # a refused call leaves the outputs alone
    # every subset of the outputs but the empty one, through the host entry
    for m in range(1, 16):
        tri[:] = 77; t[:] = 7; bary[:] = 7; mat[:] = 77
        sel = [p if m >> k & 1 else None for k, p in enumerate(outs)]
        assert L.ptk_intersect_rays(ctx.h, n, po, pd, SAMPLE, SEED, 0, *sel) == 0, m
        for k, (g, w, keep) in enumerate(zip((tri, t, bary, mat), want, (77, 7, 7, 77))):
            assert np.array_equal(g, w[:n]) if m >> k & 1 else (g == keep).all(), (m, k)
    assert ctx.last_hits_ms() > 0
    e = np.zeros((0, 3), F32)
    assert [x.shape for x in ctx.intersect_rays(e, e)] == [(0,), (0,), (0, 2), (0,)] and ctx.occluded_rays(e, e).shape == (0,)
    # a scene without triangles: misses
    empty = {k: (np.asarray(v)[:0].copy() if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material") else np.asarray(v).copy())
             for k, v in arrays.items()}
    empty["lights"] = np.zeros(0, np.int32)
    ctx.upload_scene(empty)
    g = ctx.intersect_rays(o, d, SAMPLE, SEED)
    assert (g[0] == -1).all() and np.isposinf(g[1]).all() and (g[2] == 0).all() and (g[3] == -1).all()
    assert L.ptk_intersect_rays(ctx.h, n, po, pd, 0, 0, 0, None, t.ctypes.data, None, None) == 0 and np.isposinf(t).all()
    assert (ctx.occluded_rays(o, d) == 0).all() and (ctx.occluded_rays(o, d, np.full(n, 5.0, F32)) == 0).all()
    assert ctx.last_hits_ms() == 0                                                      # (no kernel ran)


# ---- 11. worked uses -----------------------------------------------------------------------------------------------------------
def test_segments_and_ambient_occlusion(ctx, oracle_mod):
    from pbrpathtracer_amd.probes import fibonacci_dirs
    from pbrpathtracer_amd.rays import ambient_occlusion, ambient_occlusion_fold, ambient_occlusion_rays, segment_rays
    arrays, _ = RC.scene("s_cornell")
    ctx.upload_scene(arrays)
    rng = np.random.default_rng(15)
    v = np.asarray(arrays["verts"], F32).reshape(-1, 3, 3)
    pick = rng.integers(0, len(v), 50)
    w = rng.dirichlet((1.0, 1.0, 1.0), 50).astype(F32)
    points = (v[pick] * w[:, :, None]).sum(axis=1).astype(F32)
    normals = np.asarray(arrays["tbn"], F32).reshape(-1, 9)[pick, 0:3].copy()
    dirs = fibonacci_dirs(64)
    extent = float((v.reshape(-1, 3).max(axis=0) - v.reshape(-1, 3).min(axis=0)).max())
    radius, offset, sample, seed = 0.4 * extent, 1e-3 * extent, 1, 17
    got = ambient_occlusion(ctx, points, normals, dirs, radius, offset, sample=sample, seed=seed)
    assert got.dtype == F32 and got.shape == (50,)
    origins, ray_dirs, point, cos = ambient_occlusion_rays(points, normals, dirs, offset)
    _, t, _, _ = HR.mirror(oracle_mod, arrays, origins, ray_dirs, HR.ray_keys(seed, 0, len(origins), sample))
    flags = HR.occluded(t, np.full(len(origins), radius, F32))
    assert np.array_equal(ctx.occluded_rays(origins, ray_dirs, np.full(len(origins), radius, F32), sample, seed), flags)
    want = ambient_occlusion_fold(50, point, cos, flags)
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 1e-6
    assert not (got == 0).all() and not (got == 1).all() and (got >= 0).all() and (got <= 1).all()
    # visibility between point pairs: 1 - occluded of the segment, t in units of |b - a|
    a = points + normals * F32(offset)
    b = np.roll(a, 7, axis=0)
    so, sd, st = segment_rays(a, b)
    _, ts, _, _ = HR.mirror(oracle_mod, arrays, so, sd, HR.ray_keys(0, 0, len(so), 0))
    vis = 1 - ctx.occluded_rays(so, sd, st)
    assert np.array_equal(vis, 1 - HR.occluded(ts, st)) and vis.any() and not vis.all()


def test_host_class_and_equirect_hits_cli(oracle_mod, tmp_path):
    from pbrpathtracer_amd import render, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    from pbrpathtracer_amd.rays import equirect_rays
    pts, _, _ = S.build_config("C1", str(tmp_path), width=32, height=24, depth=4)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    pt.SetSeed(5)
    arrays = pt.StagedScene()
    ro, rd = RC.rays_in_box(arrays, 200, 9)
    want = HR.mirror(oracle_mod, arrays, ro, rd, HR.ray_keys(5, 17, len(ro), 2))
    got = pt.IntersectRays(ro, rd, sample=2, key_base=17)                             # no resolution work, no render before it
    assert pt.LastError() == "" and _same(got, want) and (want[0] >= 0).any() and (want[0] < 0).any()
    assert _same(pt.context().intersect_rays(ro, rd, 2, 5, key_base=17), want)
    tmax = np.random.default_rng(16).uniform(0.0, 2.0 * float(np.median(want[1][want[0] >= 0])), len(ro)).astype(F32)
    assert np.array_equal(pt.OccludedRays(ro, rd, tmax, sample=2, key_base=17), HR.occluded(want[1], tmax))
    assert np.array_equal(pt.OccludedRays(ro, rd, sample=2, key_base=17), (want[0] >= 0).astype(np.uint8))
    cam = pt.GetCamera()
    e_ro, e_rd = equirect_rays(*cam, 16, 8)
    tri, t, bary, mat = pt.IntersectRays(e_ro, e_rd)
    assert _same((tri, t, bary, mat), HR.mirror(oracle_mod, arrays, e_ro, e_rd, HR.ray_keys(5, 0, len(e_ro), 0))) and (tri >= 0).any()
    # a pending geometry edit applies, as for RenderFrame(): object 0 staged again under another matrix ([column][row])
    M = np.eye(4, dtype=F32); M[3][0] = 0.05
    pt.SetObjectTransform(0, M)
    moved = pt.StagedScene()
    assert not np.array_equal(moved["verts"], arrays["verts"])
    assert _same(pt.IntersectRays(ro, rd, sample=2, key_base=17), HR.mirror(oracle_mod, moved, ro, rd, HR.ray_keys(5, 17, len(ro), 2)))
    assert pt.LastError() == ""
    pt.close()
    npz = str(tmp_path / "pano_hits.npz")
    assert render.main([pts, "--equirect", "16", "--seed", "5", "--hits", npz]) == 0
    z = np.load(npz)
    assert sorted(z.files) == ["bary", "depth", "material", "triangle"]
    assert np.array_equal(z["triangle"], tri.reshape(8, 16)) and np.array_equal(z["depth"], t.reshape(8, 16))
    assert np.array_equal(z["bary"], bary.reshape(8, 16, 2)) and np.array_equal(z["material"], mat.reshape(8, 16))
