"""Adaptive ray queries and lightmap bakes (include/ptk.h ptk_trace_rays_adaptive, ptk_bake_lightmap_adaptive)
against the numpy mirror (tests/rays_adaptive_rule.py) fed with the CPU oracle's samples, bit for bit: counts, S1, S2 and the result
struct; and the invariant - every ray holds exactly ptk_trace_rays of its own count - whatever the pass cuts, the builder, "flat"
and the tile split.  Every comparison is np.array_equal; the recipe is fit for use by tests/test_rays_adaptive_cpu.py."""
import numpy as np
import pytest

import bake_cases as BC
import ray_cases as RC
import rays_adaptive_rule as RA

pytestmark = pytest.mark.gpu

T, MIN, STEP, MAX, DEPTH, SEED = RA.THRESHOLD, RA.MIN_SPP, RA.STEP, RA.MAX_SPP, RA.DEPTH, RA.SEED
PASS_BYTES_DEFAULT = float(16 << 30)
BAD = -1


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def _same(got, m):
    """(sum, sumsq, counts, result) of a call against the mirror's dict"""
    s1, s2, n, res = got
    assert n.dtype == np.uint32 and s1.dtype == s2.dtype == np.float32
    assert np.array_equal(n, m["n"]), (int((n != m["n"]).sum()), n[:16], m["n"][:16])
    assert np.array_equal(s1, m["S1"]) and np.array_equal(s2, m["S2"])
    assert res == dict(rounds=m["rounds"], max_count=m["max_count"], ray_samples=m["ray_samples"], active_rays=m["active"]), (res, m["rounds"])


def _invariant(ctx, ro, rd, got, key_base=0, lens_draws=False):
    """sum[i] is ptk_trace_rays(first_sample 0, spp counts[i]) of ray i, for every distinct count"""
    s1, _, n, _ = got
    for k in np.unique(n):
        plain = ctx.trace_rays(ro, rd, DEPTH, 0, int(k), SEED, key_base=key_base, lens_draws=lens_draws)
        assert np.array_equal(s1[n == k], plain[n == k]), int(k)
    return np.unique(n)


# ---- 1. the mirror, scene by scene -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RA.CASES)
def test_equals_mirror(ctx, oracle_mod, name):
    arrays, ro, rd, samples = RA.case(name)
    ctx.upload_scene(arrays)
    _same(ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED), RA.rays(samples, T, MIN, STEP, MAX))


def test_threshold_extremes_and_no_sumsq(ctx, oracle_mod):
    arrays, ro, rd, samples = RA.case("s_glass")
    ctx.upload_scene(arrays)
    _same(ctx.trace_rays_adaptive(ro, rd, DEPTH, 0.0, MIN, STEP, MAX, SEED), RA.rays(samples, 0.0, MIN, STEP, MAX))
    _same(ctx.trace_rays_adaptive(ro, rd, DEPTH, 1e30, MIN, STEP, MAX, SEED), RA.rays(samples, 1e30, MIN, STEP, MAX))
    # min_spp = max_spp: one launch, one test; min_spp = step: a test after the first round
    _same(ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MAX, STEP, MAX, SEED), RA.rays(samples, T, MAX, STEP, MAX))
    _same(ctx.trace_rays_adaptive(ro, rd, DEPTH, T, STEP, STEP, MAX, SEED), RA.rays(samples, T, STEP, STEP, MAX))
    s1, s2, n, _ = ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED, want_sumsq=False)
    m = RA.rays(samples, T, MIN, STEP, MAX)
    assert s2 is None and np.array_equal(s1, m["S1"]) and np.array_equal(n, m["n"])


# ---- 2. the invariant on the device-built tree -----------------------------------------------------------------------------------
def test_invariant_on_device_built_tree(ctx):
    arrays, _ = RC.scene("random6000")
    ro, rd = RC.rays_in_box(arrays, 500, 5)
    ctx.upload_scene(arrays)
    assert ctx.upload_timing()["built_on_device"]
    got = ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED)
    counts = _invariant(ctx, ro, rd, got)
    assert len(counts) >= 3 and counts[0] == MIN and counts[-1] == MAX
    assert got[3]["ray_samples"] == int(got[2].sum()) and got[3]["max_count"] == MAX


# ---- 3. ragged ray counts, the key wrap, lens draws ----------------------------------------------------------------------------
def test_ragged_counts_and_key_wrap(ctx, oracle_mod):
    arrays, ro, rd, samples = RA.case("s_opacity")
    ctx.upload_scene(arrays)
    for n in (1, 63, 65, 200):
        _same(ctx.trace_rays_adaptive(ro[:n], rd[:n], DEPTH, T, MIN, STEP, MAX, SEED), RA.rays(samples[:, :n], T, MIN, STEP, MAX))
    kb = 2 ** 32 - 70
    o = oracle_mod.Oracle(arrays)
    wrapped = RA.oracle_samples(o, ro, rd, DEPTH, SEED, MAX, key_base=kb)
    o.close()
    m = RA.rays(wrapped, T, MIN, STEP, MAX)
    assert not np.array_equal(m["n"], RA.rays(samples, T, MIN, STEP, MAX)["n"])
    _same(ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED, key_base=kb), m)


def test_lens_draws(ctx, oracle_mod):
    arrays, ro, rd, samples = RA.case("s_cornell")
    ctx.upload_scene(arrays)
    got = ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED, lens_draws=True)
    assert len(_invariant(ctx, ro, rd, got, lens_draws=True)) >= 3
    assert not np.array_equal(got[0], RA.rays(samples, T, MIN, STEP, MAX)["S1"])
    # S2 of a ray that stopped at the first test: the in-order sum of squares of its MIN plain samples
    i = int(np.flatnonzero(got[2] == MIN)[0])
    sq = np.zeros(3, np.float32)
    for s in range(MIN):
        v = ctx.trace_rays(ro[i:i + 1], rd[i:i + 1], DEPTH, s, 1, SEED, key_base=i, lens_draws=True)[0]
        sq = sq + v * v
    assert np.array_equal(got[1][i], sq)


# ---- 4. passes and blocks of rays -------------------------------------------------------------------------------------------------
def test_pass_cuts_give_the_same_bits(ctx):
    """"pass_bytes" is at least 1 MiB = 1024 groups of 64 rays x one sample: 70 000 rays are 1094 groups, so a round is cut into two
    blocks of rays, each in passes of one sample; at 3 MiB into passes of two samples."""
    arrays, _ = RC.scene("random300")
    ro, rd = RC.rays_in_box(arrays, 70000, 10)
    ctx.upload_scene(arrays)
    one = ctx.trace_rays_adaptive(ro, rd, DEPTH, T, 4, 2, 8, SEED)
    assert len(_invariant(ctx, ro, rd, one)) == 3
    try:
        for pass_bytes in (1 << 20, 3 << 20):
            ctx.set_option("pass_bytes", pass_bytes)
            cut = ctx.trace_rays_adaptive(ro, rd, DEPTH, T, 4, 2, 8, SEED)
            assert cut[3] == one[3]
            for a, b in zip(cut[:3], one[:3]):
                assert np.array_equal(a, b), pass_bytes
    finally:
        ctx.set_option("pass_bytes", PASS_BYTES_DEFAULT)


# ---- 5. independence ---------------------------------------------------------------------------------------------------------------
def test_independent_of_builder_flat_and_tiles(ctx, oracle_mod):
    try:
        arrays, _ = RC.scene("random6000")
        ro, rd = RC.rays_in_box(arrays, 500, 5)
        runs = []
        for device_build in (0, 1):
            ctx.set_option("device_build", device_build)
            ctx.upload_scene(arrays)
            assert ctx.upload_timing()["built_on_device"] == bool(device_build)
            runs.append(ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED))
        ctx.set_tile(1, 3)
        runs.append(ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED))
        for r in runs[1:]:
            assert r[3] == runs[0][3]
            for a, b in zip(r[:3], runs[0][:3]):
                assert np.array_equal(a, b)
        arrays, ro, rd, samples = RA.case("random16")
        ctx.upload_scene(arrays)
        for flat in (0, 1):
            ctx.set_option("flat", flat)
            _same(ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED), RA.rays(samples, T, MIN, STEP, MAX))
    finally:
        ctx.set_option("device_build", 1); ctx.set_option("flat", 1); ctx.set_tile(0, 1)


def test_leaves_the_frame_state_alone(ctx, oracle_mod):
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, samples = RA.case("random300")
    _, cam = RC.scene("random300")
    W, H = 40, 24
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, DEPTH); ctx.set_tile(0, 1); ctx.reset()
    ctx.render_adaptive(0.05, 4, 2, 8, 3)
    ctx.render_features(1 << ptk.FEAT_DEPTH, 0, 3)
    state = lambda: (ctx.read_accum(), np.array(ctx.samples()), ctx.read_sample_counts(), ctx.read_moments(), ctx.resolve_rgb8(),
                     ctx.read_feature(ptk.FEAT_DEPTH))
    before = state()
    _same(ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED), RA.rays(samples, T, MIN, STEP, MAX))
    uvs = BC.atlas("random300")[0]
    ctx.bake_lightmap_adaptive(32, 32, BC.offset_of(arrays), DEPTH, T, MIN, STEP, MAX, SEED, uvs=uvs)
    for b, a in zip(before, state()):
        assert np.array_equal(b, a)
    ctx.reset()


# ---- 6. edits are seen -------------------------------------------------------------------------------------------------------------
def test_material_and_geometry_edits_are_seen(ctx, oracle_mod):
    arrays, ro, rd, samples = RA.case("random300")
    ctx.upload_scene(arrays)
    m0 = RA.rays(samples, T, MIN, STEP, MAX)
    _same(ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED), m0)
    edited = dict(arrays); edited["materials"] = arrays["materials"].copy()
    edited["materials"][0]["emissive"] = (0.2, 1.0, 0.4)
    o = oracle_mod.Oracle(edited)
    m1 = RA.rays(RA.oracle_samples(o, ro, rd, DEPTH, SEED, MAX), T, MIN, STEP, MAX)
    o.close()
    assert not np.array_equal(m1["S1"], m0["S1"])
    ctx.update_materials(edited["materials"])
    _same(ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED), m1)
    n = len(arrays["verts"])
    a, b = n // 3, (2 * n) // 3
    moved = dict(edited); moved["verts"] = arrays["verts"].copy()
    moved["verts"][a:b] = (arrays["verts"][a:b].reshape(-1, 3, 3) + np.array([0.3, 0.15, -0.2], np.float32)).reshape(-1, 9)
    o = oracle_mod.Oracle(moved)
    m2 = RA.rays(RA.oracle_samples(o, ro, rd, DEPTH, SEED, MAX), T, MIN, STEP, MAX)
    o.close()
    assert not np.array_equal(m2["S1"], m1["S1"])
    ctx.update_geometry(a, moved["verts"][a:b])
    _same(ctx.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED), m2)


# ---- 7. the device entry -----------------------------------------------------------------------------------------------------------
def test_device_entry_on_a_callers_stream(oracle_mod):
    import torch
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, samples = RA.case("random300")
    m = RA.rays(samples, T, MIN, STEP, MAX)
    dev = torch.device("cuda:0")
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays)
        host = c.trace_rays_adaptive(ro, rd, DEPTH, T, MIN, STEP, MAX, SEED)
        _same(host, m)
        t_ro, t_rd = torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=dev)
        c.set_stream(s.cuda_stream)
        big = torch.randn(2048, 2048, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            f_ro, f_rd = torch.zeros_like(t_ro), torch.zeros_like(t_rd)
            for _ in range(8):
                big = big @ big * 1e-3
            f_ro.copy_(t_ro); f_rd.copy_(t_rd)                       # the inputs are filled on that stream behind a long kernel
            s1, s2, n, res = c.trace_rays_adaptive(f_ro, f_rd, DEPTH, T, MIN, STEP, MAX, SEED)
        # synchronous: no wait of the caller's before reading
        assert isinstance(s1, torch.Tensor) and s1.device == t_ro.device
        _same((s1.cpu().numpy(), s2.cpu().numpy(), n.cpu().numpy().view(np.uint32), res), m)
    finally:
        c.close()


# ---- 8. the lightmap ---------------------------------------------------------------------------------------------------------------
W = H = 32


def _lightmap_mirror(OB, name, flags=0, key_base=0):
    arrays, _ = RC.scene(name)
    uvs = BC.atlas(name)[0]
    off = BC.offset_of(arrays)
    t, ro, rd, owner = BC.rays(arrays, uvs, W, H, off, flags)
    o = OB.Oracle(arrays)
    samples = RA.oracle_samples(o, ro, rd, DEPTH, SEED, MAX, keys=(key_base + t) & 0xffffffff)
    o.close()
    return arrays, uvs, off, t, owner, samples


def _check_lightmap(got, t, owner, m):
    out, counts, own, res = got
    assert out.shape == (H, W, 3) and counts.shape == (H, W) and counts.dtype == np.uint32
    assert np.array_equal(own, owner)
    n = np.zeros(W * H, np.uint32); n[t] = m["n"]
    s1 = np.zeros((W * H, 3), np.float32); s1[t] = m["S1"]
    assert np.array_equal(counts.reshape(-1), n), int((counts.reshape(-1) != n).sum())
    assert np.array_equal(out.reshape(-1, 3), s1)
    assert (counts[owner < 0] == 0).all() and (out[owner < 0] == 0).all() and (owner < 0).any()
    assert res == dict(rounds=m["rounds"], max_count=m["max_count"], ray_samples=m["ray_samples"], active_rays=m["active"])


@pytest.mark.parametrize("name", ["s_cornell", "random300"])
def test_lightmap_equals_mirror(ctx, oracle_mod, name):
    arrays, uvs, off, t, owner, samples = _lightmap_mirror(oracle_mod, name)
    m = RA.lightmap(samples, t, W, H, T, MIN, STEP, MAX)
    # the neighbourhood term is at work, and texels stop at different counts
    assert len(np.unique(m["n"])) >= 3 and not np.array_equal(m["n"], RA.rays(samples, T, MIN, STEP, MAX)["n"])
    ctx.upload_scene(arrays)
    assert np.array_equal(ctx.bake_coverage(W, H, uvs)[0], owner)
    _check_lightmap(ctx.bake_lightmap_adaptive(W, H, off, DEPTH, T, MIN, STEP, MAX, SEED, uvs=uvs), t, owner, m)
    # threshold 0: a plain bake of max_spp
    out, counts, _, res = ctx.bake_lightmap_adaptive(W, H, off, DEPTH, 0.0, MIN, STEP, MAX, SEED, uvs=uvs)
    plain, _ = ctx.bake_lightmap(W, H, off, DEPTH, 0, MAX, SEED, uvs=uvs)
    assert np.array_equal(out, plain) and (counts[owner >= 0] == MAX).all() and res["active_rays"] == len(t)


def test_lightmap_back_key_base_and_device_entry(ctx, oracle_mod):
    import torch
    kb = 2 ** 32 - 300
    arrays, uvs, off, t, owner, samples = _lightmap_mirror(oracle_mod, "s_cornell", BC.BACK, kb)
    m = RA.lightmap(samples, t, W, H, T, MIN, STEP, MAX)
    ctx.upload_scene(arrays)
    _check_lightmap(ctx.bake_lightmap_adaptive(W, H, off, DEPTH, T, MIN, STEP, MAX, SEED, uvs=uvs, key_base=kb, back=True), t, owner, m)
    d = ctx.bake_lightmap_adaptive(W, H, off, DEPTH, T, MIN, STEP, MAX, SEED, uvs=torch.from_numpy(uvs).to("cuda:0"), key_base=kb, back=True)
    _check_lightmap((d[0].cpu().numpy(), d[1].cpu().numpy().view(np.uint32), d[2].cpu().numpy(), d[3]), t, owner, m)


# ---- 9. arguments ------------------------------------------------------------------------------------------------------------------
def test_arguments(ctx, oracle_mod):
    import ctypes as C
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, samples = RA.case("s_cornell")
    L = ptk.load()
    n = 10
    o, d = ro[:n].copy(), rd[:n].copy()
    s1 = np.full((n, 3), 7.0, np.float32); s2 = s1.copy(); cnt = np.full(n, 7, np.uint32)
    res = ptk.RaysAdaptiveResult(); res.rounds = 99
    po, pd, p1, p2, pc = o.ctypes.data, d.ctypes.data, s1.ctypes.data, s2.ctypes.data, cnt.ctypes.data
    rays = (L.ptk_trace_rays_adaptive, L.ptk_trace_rays_adaptive_device)

    def ray_call(fn, h=None, num=n, org=po, dr=pd, thr=T, mn=MIN, st=STEP, mx=MAX, flags=0, sm=p1, c=pc):
        return fn(ctx.h if h is None else h, num, org, dr, DEPTH, thr, mn, st, mx, SEED, 0, flags, sm, p2, c, C.byref(res))

    fresh = ptk.Context(0)
    try:
        for fn in rays:
            assert ray_call(fn, h=fresh.h) == BAD                                   # before ptk_upload_scene
            assert b"ptk_upload_scene" in L.ptk_last_error(fresh.h)
    finally:
        fresh.close()
    ctx.upload_scene(arrays)
    bad_rays = [dict(org=None), dict(dr=None), dict(sm=None), dict(c=None), dict(num=-1), dict(flags=ptk.RAYS_ACCUMULATE), dict(flags=4),
                dict(st=1), dict(st=0), dict(st=3), dict(mn=6, mx=32), dict(mn=8, mx=30), dict(mn=0), dict(mn=16, mx=8),
                dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=-0.5)]
    for fn in rays:
        assert fn(None, n, po, pd, DEPTH, T, MIN, STEP, MAX, SEED, 0, 0, p1, p2, pc, None) == BAD
        for kw in bad_rays:
            assert ray_call(fn, **kw) == BAD, kw
            assert L.ptk_last_error(ctx.h) != b"", kw
        assert fn(ctx.h, 0, None, None, DEPTH, T, MIN, STEP, MAX, SEED, 0, 0, None, None, None, None) == 0      # no rays: nothing to do
    assert (s1 == 7.0).all() and (s2 == 7.0).all() and (cnt == 7).all() and res.rounds == 99             # the outputs were left alone
    assert L.ptk_last_rays_adaptive_ms(None, None, None, None) == BAD
    # the lightmap entries
    uvs = BC.atlas("s_cornell")[0]
    off = BC.offset_of(arrays)
    out = np.full((H, W, 3), 7.0, np.float32); lc = np.full((H, W), 7, np.uint32)
    pu, pout, plc = uvs.ctypes.data, out.ctypes.data, lc.ctypes.data

    def map_call(fn, w=W, h=H, offset=off, thr=T, mn=MIN, st=STEP, mx=MAX, flags=0, o_=pout, c=plc):
        return fn(ctx.h, w, h, pu, offset, DEPTH, thr, mn, st, mx, SEED, 0, flags, o_, c, None, C.byref(res))

    bad_maps = [dict(w=0), dict(h=16385), dict(offset=0.0), dict(offset=float("nan")), dict(flags=ptk.BAKE_ACCUMULATE), dict(flags=4),
                dict(o_=None), dict(c=None), dict(st=1), dict(st=3), dict(mn=0), dict(mn=16, mx=8), dict(mn=8, mx=30),
                dict(thr=float("nan")), dict(thr=-1.0)]
    for fn in (L.ptk_bake_lightmap_adaptive, L.ptk_bake_lightmap_adaptive_device):
        assert fn(None, W, H, pu, off, DEPTH, T, MIN, STEP, MAX, SEED, 0, 0, pout, plc, None, None) == BAD
        for kw in bad_maps:
            assert map_call(fn, **kw) == BAD, kw
            assert L.ptk_last_error(ctx.h) != b"", kw
    assert (out == 7.0).all() and (lc == 7).all() and res.rounds == 99
    # no rays through the wrapper; a scene without triangles: black converges at the first test (never, at threshold 0)
    e = ctx.trace_rays_adaptive(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), DEPTH, T, MIN, STEP, MAX, SEED)
    assert e[0].shape == (0, 3) and e[2].shape == (0,) and e[3] == dict(rounds=0, max_count=0, ray_samples=0, active_rays=0)
    empty = {k: (v[:0] if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material", "lights") else v) for k, v in arrays.items()}
    ctx.upload_scene(empty)
    s1, s2, cnt, r = ctx.trace_rays_adaptive(o, d, DEPTH, T, MIN, STEP, MAX, SEED)
    assert (s1 == 0).all() and (s2 == 0).all() and (cnt == MIN).all()
    assert r == dict(rounds=MIN // STEP, max_count=MIN, ray_samples=n * MIN, active_rays=0)
    _, _, cnt, r = ctx.trace_rays_adaptive(o, d, DEPTH, 0.0, MIN, STEP, MAX, SEED)
    assert (cnt == MAX).all() and r == dict(rounds=MAX // STEP, max_count=MAX, ray_samples=n * MAX, active_rays=n)
    ctx.upload_scene(arrays)
    ctx.trace_rays_adaptive(o, d, DEPTH, T, MIN, STEP, MAX, SEED)
    ms = ctx.last_rays_adaptive_ms()
    assert ms["total_ms"] > 0 and ms["trace_ms"] > 0 and ms["other_ms"] > 0


# ---- 10. host class, pth_ wrapper and command line -----------------------------------------------------------------------------------
def test_host_class_and_cli(oracle_mod, tmp_path):
    from pbrpathtracer_amd import render, scenes as S
    from pbrpathtracer_amd.lightmap import grid_atlas
    from pbrpathtracer_amd.pathtracer import PathTracer, image_load
    from pbrpathtracer_amd.rays import equirect_rays
    pts, _, _ = S.build_config("C1", str(tmp_path), width=32, height=24, depth=4)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    pt.SetSeed(5)
    arrays = pt.StagedScene()
    depth = pt.GetTraceDepth()
    ro, rd = RC.rays_in_box(arrays, 100, 9)
    o = oracle_mod.Oracle(arrays)
    m = RA.rays(RA.oracle_samples(o, ro, rd, depth, 5, 16, key_base=17), 0.1, 4, 4, 16)
    got = pt.TraceRaysAdaptive(ro, rd, 0.1, 4, 4, 16, key_base=17)          # (through pth_trace_rays_adaptive)
    assert pt.LastError() == ""
    _same(got, m)
    assert len(np.unique(m["n"])) >= 2
    c = pt.context()
    for a, b in zip(c.trace_rays_adaptive(ro, rd, depth, 0.1, 4, 4, 16, 5, key_base=17)[:3], got[:3]):
        assert np.array_equal(a, b)
    uvs = grid_atlas(pt.GetTriangleCount(), 16, 16)
    off = render.bake_offset(pt)
    lm = pt.BakeLightmapAdaptive(16, 16, off, 0.1, 4, 4, 16, uvs=uvs)        # (through pth_bake_lightmap_adaptive)
    direct = c.bake_lightmap_adaptive(16, 16, off, depth, 0.1, 4, 4, 16, 5, uvs=uvs)
    assert lm[3] == direct[3] and all(np.array_equal(a, b) for a, b in zip(lm[:3], direct[:3])) and (lm[1] > 0).any()
    cam = pt.GetCamera()
    pt.close()
    # --equirect WIDTH --noise-threshold T
    png, npy = str(tmp_path / "pano.png"), str(tmp_path / "pano.npy")
    args = ["--noise-threshold", "0.1", "--min-spp", "4", "--step", "4", "--spp", "16", "--seed", "5"]
    assert render.main([pts, "--equirect", "16", *args, "-o", png, "--npy", npy]) == 0
    e_ro, e_rd = equirect_rays(*cam, 16, 8)
    pm = RA.rays(RA.oracle_samples(o, e_ro, e_rd, depth, 5, 16), 0.1, 4, 4, 16)
    o.close()
    mean = (pm["S1"] / pm["n"].astype(np.float32)[:, None]).reshape(8, 16, 3)
    assert np.array_equal(np.load(npy), mean) and np.array_equal(np.load(str(tmp_path / "pano.counts.npy")), pm["n"].reshape(8, 16))
    img = image_load(png)
    assert img is not None and np.array_equal(img[..., :3], render.resolve_mean(mean, 1))
    # --bake-lightmap SIZE --noise-threshold T
    png, npy = str(tmp_path / "map.png"), str(tmp_path / "map.npy")
    assert render.main([pts, "--bake-lightmap", "16", "--bake-atlas", *args, "-o", png, "--npy", npy]) == 0
    with np.errstate(all="ignore"):
        lmean = np.where(lm[1][..., None] == 0, np.float32(0), lm[0] / lm[1].astype(np.float32)[..., None]).astype(np.float32)
    assert np.array_equal(np.load(npy), lmean) and np.array_equal(np.load(str(tmp_path / "map.counts.npy")), lm[1])
    img = image_load(png)
    assert img is not None and np.array_equal(img[..., :3], render.resolve_mean(lmean, 1)[::-1])
