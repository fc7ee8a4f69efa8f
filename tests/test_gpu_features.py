"""First-hit feature planes and picking (include/ptk.h ptk_render_features, ptk_pick) on the GPU: every plane array_equal to
tests/feature_truth.py - the CPU oracle's camera-ray records plus a float32 restatement of its shading lines - NaN == NaN where a
degenerate normal makes one.  Then what must not change a bit (lens, primary-hit cache, FLAT option, tile split), what must not
be touched (accumulator, adaptive state), the mask / resolution rules, material edits, picking, the host class and a caller's
stream."""
import numpy as np
import pytest

import feature_truth as FT
from conftest import load_golden, scene_from_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def _golden(name, aperture=0.0):
    z = load_golden(f"tier_{name}.npz")
    cam = z["cam"]; proj = z["proj"]
    return scene_from_golden(z), dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]),
                                      focal_dist=float(z["focal_dist"]), aperture=aperture)


def _random(seed, n, tex=True):
    from test_gpu_random_scenes import random_scene
    arrays, cam = random_scene(seed, n, tex)
    return arrays, dict(cam, aperture=0.0)


def _setup(ctx, arrays, cam, W, H, rank=0, world=1, D=4):
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(rank, world); ctx.reset()


def _planes(ctx, mask=None, sample=0, seed=0):
    from pbrpathtracer_amd import ptk
    mask = ptk.FEAT_ALL if mask is None else mask
    ctx.render_features(mask, sample, seed)
    return {nm: ctx.read_feature(k) for k, nm in enumerate(ptk.FEAT_NAMES) if (mask >> k) & 1}


def _assert_planes(got, want, what=""):
    for nm, g in got.items():
        w = want[nm]
        if not FT.planes_equal(g, w):
            bad = np.argwhere((g != w) & ~(np.isnan(g) & np.isnan(w)) if g.dtype.kind == "f" else g != w)
            print(f"{what} {nm}: {len(bad)} elements differ, first {bad[:3].tolist()}, got {g[tuple(bad[0])]!r} want {w[tuple(bad[0])]!r}")
        assert FT.planes_equal(g, w), (what, nm)


CASES = [("golden_s_cornell", 48, 40), ("golden_s_glass", 48, 40), ("golden_s_opacity", 48, 40), ("flat16", 48, 32),
         ("host300", 48, 32), ("device6000", 48, 32), ("ragged", 53, 37), ("one", 1, 1)]


def _case(kind):
    if kind.startswith("golden_"):
        return _golden(kind[7:])
    return {"flat16": lambda: _random(12, 16), "host300": lambda: _random(14, 300), "device6000": lambda: _random(16, 6000),
            "ragged": lambda: _random(18, 1500), "one": lambda: _random(14, 300)}[kind]()


BRANCHES = {}


@pytest.mark.parametrize("kind,W,H", CASES)
def test_planes_match_oracle(ctx, oracle_mod, kind, W, H):
    arrays, cam = _case(kind)
    seed, sample = 9, 3
    want = FT.truth(oracle_mod, arrays, cam, W, H, seed, sample)
    _setup(ctx, arrays, cam, W, H)
    got = _planes(ctx, sample=sample, seed=seed)
    _assert_planes(got, want, kind)
    if W * H > 1:
        assert (want["triangle"] >= 0).any(), "nothing in view: a poor test"
    BRANCHES[kind] = want["branches"]
    print(kind, want["branches"], "misses", int((want["triangle"] < 0).sum()), "of", W * H)


def test_every_branch_of_the_normal_code_was_in_view(oracle_mod):
    """A smoothed triangle, a normal-mapped one, one with both and a back-facing hit (the flip) must each occur in some pixel
    of some case above - computed here again on the truth planes, so that this test stands on its own."""
    total = dict(smooth=0, normal_map=0, both=0, flip=0)
    for kind, W, H in CASES:
        if kind not in BRANCHES:
            arrays, cam = _case(kind)
            BRANCHES[kind] = FT.truth(oracle_mod, arrays, cam, W, H, 9, 3)["branches"]
        for k in total:
            total[k] += BRANCHES[kind][k]
    print(total)
    for k, n in total.items():
        assert n > 0, f"no case has a pixel in the '{k}' branch"


def _opacity_scene():
    return _random(12, 16)[0], _random(12, 16)[1], 48, 32


def test_opacity_draws_are_the_paths_own(ctx, oracle_mod):
    """Stochastic opacity: the hit of a pixel depends on (seed, pixel, sample).  First, on the oracle's records alone: samples 0
    and 1 see different triangles in at least 1 % of the pixels (so the per-sample draw is exercised); then samples 0, 1, 7 and
    two seeds, one with its high word set."""
    arrays, cam, W, H = _opacity_scene()
    seed = 9
    r0 = FT.camera_records(oracle_mod, arrays, cam, W, H, seed, 0)
    r1 = FT.camera_records(oracle_mod, arrays, cam, W, H, seed, 1)
    differ = float((r0["tri"] != r1["tri"]).mean())
    print(f"hit triangle of samples 0 and 1 differs in {differ:.4f} of the pixels")
    assert differ >= 0.01, differ
    _setup(ctx, arrays, cam, W, H)
    for seed in (9, (0xABCD1234 << 32) | 77):
        for sample in (0, 1, 7):
            want = FT.truth(oracle_mod, arrays, cam, W, H, seed, sample)
            _assert_planes(_planes(ctx, sample=sample, seed=seed), want, f"seed {seed:#x} sample {sample}")


@pytest.mark.parametrize("kind,W,H", [("golden_s_cornell", 48, 40), ("flat16", 48, 32), ("host300", 48, 32)])
def test_lens_cache_and_flat_options_change_nothing(ctx, oracle_mod, kind, W, H):
    arrays, cam = _case(kind)
    want = FT.truth(oracle_mod, arrays, cam, W, H, 4, 1)
    try:
        for aperture in (0.0, 0.06):
            for cache in (1, 0):
                for flat in (1, 0):
                    ctx.set_option("primary_cache", cache); ctx.set_option("flat", flat)
                    _setup(ctx, arrays, dict(cam, aperture=aperture), W, H)
                    _assert_planes(_planes(ctx, sample=1, seed=4), want, f"{kind} aperture {aperture} cache {cache} flat {flat}")
    finally:
        ctx.set_option("primary_cache", 1); ctx.set_option("flat", 1)


def test_render_state_is_not_touched(ctx, oracle_mod):
    from pbrpathtracer_amd import ptk
    arrays, cam = _golden("s_cornell")
    W, H = 48, 40
    _setup(ctx, arrays, cam, W, H)
    ctx.render(0, 16, 5)
    ref = ctx.read_accum(), ctx.resolve_rgb8(), ctx.samples()
    _setup(ctx, arrays, cam, W, H)
    ctx.render(0, 8, 5); ctx.render_features(ptk.FEAT_ALL, 2, 5); ctx.render(8, 8, 5)
    assert np.array_equal(ctx.read_accum(), ref[0]) and np.array_equal(ctx.resolve_rgb8(), ref[1]) and ctx.samples() == ref[2] == 16
    # ... with the camera set anew in between (the features call is then the one that refreshes the primary-hit cache)
    _setup(ctx, arrays, cam, W, H)
    ctx.render(0, 8, 5); ctx.set_camera(**cam); ctx.render_features(ptk.FEAT_ALL, 0, 5); ctx.render(8, 8, 5)
    assert np.array_equal(ctx.read_accum(), ref[0]) and np.array_equal(ctx.resolve_rgb8(), ref[1])
    # around an adaptive render: counts, S1, S2
    _setup(ctx, arrays, cam, W, H)
    ctx.render_adaptive(0.1, 8, 4, 32, 5)
    want = ctx.read_sample_counts(), ctx.read_accum(), ctx.read_moments(), ctx.resolve_rgb8()
    _setup(ctx, arrays, cam, W, H)
    ctx.render_features(ptk.FEAT_ALL, 0, 5)
    ctx.render_adaptive(0.1, 8, 4, 32, 5)
    ctx.render_features(ptk.FEAT_ALL, 1, 5)
    got = ctx.read_sample_counts(), ctx.read_accum(), ctx.read_moments(), ctx.resolve_rgb8()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("world", [2, 3])
def test_tile_split_writes_owned_pixels_only(ctx, oracle_mod, world):
    arrays, cam = _random(14, 300)
    W, H = 53, 37
    full = FT.truth(oracle_mod, arrays, cam, W, H, 6, 0)
    seen = np.zeros((H, W), int)
    for rank in range(world):
        want = FT.truth(oracle_mod, arrays, cam, W, H, 6, 0, rank=rank, world=world)
        own = want["owned"]
        seen += own
        _setup(ctx, arrays, cam, W, H, rank, world)
        got = _planes(ctx, seed=6)
        _assert_planes(got, want, f"rank {rank} of {world}")
        for nm in FT.NAMES:
            assert FT.planes_equal(got[nm][own], full[nm][own]), nm
        assert (got["triangle"][~own] == -1).all() and (got["material"][~own] == -1).all() and np.isposinf(got["depth"][~own]).all()
        for nm in ("bary", "position", "normal_geom", "normal", "albedo", "emission", "gloss"):
            assert not got[nm][~own].any(), nm
    assert (seen == 1).all()
    ctx.set_tile(0, 1)


def test_mask_and_resolution_rules(ctx, oracle_mod):
    from pbrpathtracer_amd import ptk
    arrays, cam = _golden("s_cornell")
    W, H = 48, 40
    want = FT.truth(oracle_mod, arrays, cam, W, H, 0, 0)
    _setup(ctx, arrays, cam, W, H)
    with pytest.raises(ptk.PtkError):
        ctx.read_feature(ptk.FEAT_DEPTH)                    # nothing rendered yet
    got = _planes(ctx, mask=(1 << ptk.FEAT_DEPTH) | (1 << ptk.FEAT_ALBEDO))
    _assert_planes(got, want, "depth | albedo")
    rc = ctx.L.ptk_read_feature(ctx.h, ptk.FEAT_NORMAL, np.zeros((H, W, 3), np.float32).ctypes.data)
    assert rc == -1                                         # PTK_ERR_BAD_ARG
    with pytest.raises(ptk.PtkError):
        ctx.feature_device_ptr(ptk.FEAT_NORMAL)
    for bad in (-1, 10):
        assert ctx.L.ptk_read_feature(ctx.h, bad, np.zeros(W * H * 3, np.float32).ctypes.data) == -1
    with pytest.raises(ptk.PtkError):
        ctx.render_features(1 << 10)                        # unknown bit
    # a plane that was rendered once but is not in the newest mask is not readable either
    _planes(ctx)
    _planes(ctx, mask=1 << ptk.FEAT_TRIANGLE)
    with pytest.raises(ptk.PtkError):
        ctx.read_feature(ptk.FEAT_DEPTH)
    # another resolution: every read fails until the next render_features
    _planes(ctx)
    ctx.set_frame(32, 24, 4)
    for k in range(10):
        with pytest.raises(ptk.PtkError):
            ctx.read_feature(k)
    want2 = FT.truth(oracle_mod, arrays, cam, 32, 24, 0, 0)
    _assert_planes(_planes(ctx), want2, "after set_frame")
    # no scene / no frame: BAD_ARG, nothing else
    c2 = ptk.Context(0)
    with pytest.raises(ptk.PtkError):
        c2.render_features(ptk.FEAT_ALL)
    c2.upload_scene(arrays)
    with pytest.raises(ptk.PtkError):
        c2.render_features(ptk.FEAT_ALL)
    with pytest.raises(ptk.PtkError):
        c2.pick(0, 0)
    c2.close()


def test_material_edit_is_seen(ctx, oracle_mod):
    from pbrpathtracer_amd import ptk
    arrays, cam = _golden("s_cornell")
    W, H = 48, 40
    _setup(ctx, arrays, cam, W, H)
    before = _planes(ctx)
    edited = dict(arrays)
    mats = np.array(arrays["materials"], dtype=ptk.MATERIAL_DTYPE, copy=True)
    visible = np.unique(before["material"][before["material"] >= 0])
    untextured = [m for m in visible if mats[m]["tex"][0] < 0]
    assert untextured
    mats["diffuse"][untextured[0]] = (0.125, 0.5, 0.875)
    edited["materials"] = mats
    ctx.update_materials(mats)
    after = _planes(ctx)
    want = FT.truth(oracle_mod, edited, cam, W, H, 0, 0)
    _assert_planes(after, want, "edited")
    assert np.array_equal(after["triangle"], before["triangle"])
    assert not np.array_equal(after["albedo"], before["albedo"])


def test_pick_equals_the_planes(ctx, oracle_mod):
    from pbrpathtracer_amd import ptk
    for (arrays, cam), W, H, seed in ((_golden("s_cornell"), 48, 40, 0), ((_opacity_scene()[0], _opacity_scene()[1]), 48, 32, 9)):
        _setup(ctx, arrays, cam, W, H)
        p = _planes(ctx, seed=seed)
        rng = np.random.default_rng(3)
        hit = np.argwhere(p["triangle"] >= 0); miss = np.argwhere(p["triangle"] < 0)
        pts = [hit[i] for i in rng.choice(len(hit), min(len(hit), 35), replace=False)]
        pts += [miss[i] for i in rng.choice(len(miss), min(len(miss), 15), replace=False)] if len(miss) else []
        if len(miss) == 0:
            pts += [hit[i] for i in rng.choice(len(hit), 15, replace=False)]
        assert len(pts) == 50
        for b, x in pts:
            tri, mat, t = ctx.pick(int(x), int(H - 1 - b), seed)         # planes are bottom-up, pick counts y from the top
            assert (tri, mat) == (p["triangle"][b, x], p["material"][b, x]) and np.float32(t) == p["depth"][b, x], (x, b)
        for x, y in ((-1, 0), (0, -1), (W, 0), (0, H)):
            with pytest.raises(ptk.PtkError):
                ctx.pick(x, y, seed)
        # the planes were not disturbed by picking
        assert np.array_equal(ctx.read_feature(ptk.FEAT_TRIANGLE), p["triangle"])
        if seed == 0:
            assert len(miss) > 0 and len(hit) > 0, "the golden Cornell frame should show hits and sky"


def test_host_class(tmp_path, oracle_mod):
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer, camera_from_scene
    pts, scene, _ = S.build_config("C1", str(tmp_path), width=96, height=64, depth=4)
    pt = PathTracer(0); pt.LoadSceneFile(pts); pt.SetSeed(3); pt.SetCameraAperture(0.0)
    W, H = pt.GetResolution()
    pt.RenderFrames(2)
    acc = pt.ReadAccumulation()
    pt.RenderFeatures(ptk.FEAT_ALL, 1)
    host = {nm: pt.ReadFeature(k) for k, nm in enumerate(ptk.FEAT_NAMES)}
    assert pt.LastError() == "" and pt.GetSamples() == 2 and np.array_equal(pt.ReadAccumulation(), acc)
    cam = dict(camera_from_scene(scene), aperture=0.0)
    staged = pt.StagedScene()
    c = ptk.Context(0)
    _setup(c, staged, cam, W, H)
    abi = _planes(c, sample=1, seed=3)
    for nm in ptk.FEAT_NAMES:
        assert FT.planes_equal(host[nm], abi[nm]), nm
    _assert_planes(host, FT.truth(oracle_mod, staged, cam, W, H, 3, 1), "host class")
    c.close()
    # Pick: sample 0 of the class's seed; no opacity map here, so the sample does not matter
    objs = [(o, e) for o in range(pt.L.pth_num_objects(pt.h)) for e in range(pt.L.pth_num_elements(pt.h, o))]
    tri, mat = host["triangle"], host["material"]
    assert (tri < 0).any() and (tri >= 0).any()
    rng = np.random.default_rng(1)
    for sel in (np.argwhere(tri >= 0), np.argwhere(tri < 0)):
        for b, x in sel[rng.choice(len(sel), 10, replace=False)]:
            o, e, t = pt.Pick(int(x), int(H - 1 - b))
            if tri[b, x] < 0:
                assert (o, e, t) == (-1, -1, -1)
            else:
                assert t == tri[b, x] and objs[mat[b, x]] == (o, e)
    with pytest.raises(ptk.PtkError):
        pt.Pick(W, 0)
    pt.close()


def test_caller_stream_and_device_view(ctx, oracle_mod):
    import torch
    from pbrpathtracer_amd import ptk
    arrays, cam = _random(14, 300)
    W, H = 48, 32
    c = ptk.Context(0)
    _setup(c, arrays, cam, W, H)
    s = torch.cuda.Stream()
    c.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        c.render_features(ptk.FEAT_ALL, 0, 2)
        views = {}
        for k, nm in enumerate(ptk.FEAT_NAMES):
            ptr, nbytes = c.feature_device_ptr(k)
            ch, isint = ptk.feature_info(k)
            assert nbytes == W * H * ch * 4
            iface = dict(shape=(H, W, ch) if ch > 1 else (H, W), typestr="<i4" if isint else "<f4", data=(ptr, False), version=2)
            holder = type("Plane", (), {"__cuda_array_interface__": iface})()
            views[nm] = torch.as_tensor(holder, device="cuda").clone()
    s.synchronize()
    want = FT.truth(oracle_mod, arrays, cam, W, H, 2, 0)
    for k, nm in enumerate(ptk.FEAT_NAMES):
        host = c.read_feature(k)
        assert FT.planes_equal(views[nm].cpu().numpy(), host), nm
        assert FT.planes_equal(host, want[nm]), nm
    c.close()


@pytest.mark.parametrize("cfg,world,all_planes", [("C4", 61, False), ("C5", 61, False), ("C3", 149, True)])
def test_full_size_on_one_rank_of_a_wide_split(tmp_path, oracle_mod, cfg, world, all_planes):
    """The big configs at 1280x720, whole frame on the GPU; the oracle's records for the tiles of one rank of a wide split
    (as test_full_size_spot_check_against_oracle picks it)."""
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer, camera_from_scene
    pts, scene, _ = S.build_config(cfg, str(tmp_path), width=1280, height=720)
    pt = PathTracer(0); pt.LoadSceneFile(pts); pt.SetSeed(21)
    W, H = pt.GetResolution()
    assert (W, H) == (1280, 720)
    mask = ptk.FEAT_ALL if all_planes else (1 << ptk.FEAT_TRIANGLE) | (1 << ptk.FEAT_DEPTH)
    pt.RenderFeatures(mask, 5)
    assert pt.LastError() == ""
    got = {nm: pt.ReadFeature(k) for k, nm in enumerate(ptk.FEAT_NAMES) if (mask >> k) & 1}
    cam = dict(camera_from_scene(scene), aperture=0.0)
    rank = world // 3
    want = FT.truth(oracle_mod, pt.StagedScene(), cam, W, H, 21, 5, rank=rank, world=world)
    own = want["owned"]
    assert own.sum() >= 16 * 16 * 4 and (want["triangle"][own] >= 0).any()
    for nm, g in got.items():
        assert FT.planes_equal(g[own], want[nm][own]), (cfg, nm)
    print(cfg, "owned pixels", int(own.sum()), "hits", int((want["triangle"][own] >= 0).sum()), want["branches"])
    pt.close()
