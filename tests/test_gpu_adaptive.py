"""The adaptive render (include/ptk.h ptk_render_adaptive) on the GPU, bit for bit against the numpy mirror of the rule
(tests/adaptive_rule.py) fed with the CPU oracle's per-sample values: counts, S1, S2 and RGB8.  Then what must not change a
bit - the tile split, the work distribution, threshold 0 against a plain render - and the call order."""
import threading
import time

import numpy as np
import pytest

import adaptive_rule as AR
from conftest import load_golden, scene_from_golden

pytestmark = pytest.mark.gpu

STEP, MIN_SPP, MAX_SPP = 4, 8, 32
THRESHOLDS = (0.3, 0.2, 0.12, 0.08, 0.05, 0.03, 0.02, 0.5, 0.8, 1.2)


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def _golden_cam(z, aperture=None):
    cam = z["cam"]; proj = z["proj"]
    return dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]),
                focal_dist=float(z["focal_dist"]), aperture=float(z["aperture"]) if aperture is None else aperture)


def _scene(kind):
    if kind.startswith("golden_"):
        name, _, lens = kind[7:].partition("+")
        z = load_golden(f"tier_{name}.npz")
        return scene_from_golden(z), _golden_cam(z, 0.06 if lens else 0.0), int(z["depth"])
    from test_gpu_random_scenes import random_scene
    seed, n = {"flat": (12, 16), "host_bvh": (14, 300), "device_bvh": (16, 6000)}[kind]
    arrays, cam = random_scene(seed, n, True)
    return arrays, cam, 5


def _oracle_samples(oracle_mod, arrays, cam, W, H, D, count, seed):
    o = oracle_mod.Oracle(arrays)
    ocam = oracle_mod.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])
    s = AR.oracle_samples(o, ocam, W, H, D, count, seed)
    o.close()
    return s


def _pick_threshold(samples):
    """The first threshold under which the mirror gives >= 3 distinct counts, some pixels below MAX_SPP and some at it."""
    for t in THRESHOLDS:
        r = AR.adaptive(samples, t, MIN_SPP, STEP, MAX_SPP)
        n = r["n"]
        if len(np.unique(n)) >= 3 and (n < MAX_SPP).any() and (n == MAX_SPP).any():
            return t, r
    pytest.fail("no threshold spreads the counts: a poor test scene")


def _setup(ctx, arrays, cam, W, H, D, rank=0, world=1):
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(rank, world); ctx.reset()


def _state(ctx):
    return ctx.read_sample_counts(), ctx.read_accum(), ctx.read_moments(), ctx.resolve_rgb8()


def _assert_equals_mirror(got, want, what=""):
    n, S1, S2, rgb = got
    assert np.array_equal(n, want["n"]), (what, np.argwhere(n != want["n"])[:5])
    assert np.array_equal(S1, want["S1"]), what
    assert np.array_equal(S2, want["S2"]), what
    assert np.array_equal(rgb, want["rgb8"]), what


@pytest.mark.parametrize("kind,W,H", [("golden_s_cornell", 48, 48), ("golden_s_cornell+lens", 48, 48), ("golden_s_opacity", 48, 40),
                                      ("golden_s_glass", 53, 37), ("flat", 48, 32), ("host_bvh", 48, 32), ("device_bvh", 48, 32)])
def test_adaptive_matches_oracle_rule(ctx, oracle_mod, kind, W, H):
    arrays, cam, D = _scene(kind)
    seed = 77
    samples = _oracle_samples(oracle_mod, arrays, cam, W, H, D, MAX_SPP, seed)
    t, want = _pick_threshold(samples)
    _setup(ctx, arrays, cam, W, H, D)
    res = ctx.render_adaptive(t, MIN_SPP, STEP, MAX_SPP, seed)
    _assert_equals_mirror(_state(ctx), want, kind)
    assert res["max_count"] == want["n"].max() == ctx.samples()
    assert res["pixel_samples"] == int(want["n"].sum())
    assert res["active_pixels"] == want["active_pixels"]
    assert res["rounds"] == want["rounds"]
    print(f"{kind}: threshold {t}, counts {np.unique(want['n']).tolist()}, rounds {res['rounds']}, "
          f"pixel samples {res['pixel_samples'] / (W * H * MAX_SPP):.3f} of uniform")


@pytest.mark.parametrize("contract", [0, 2])
def test_threshold_zero_is_a_plain_render(ctx, contract):
    z = load_golden("tier_s_glass.npz")
    arrays, cam = scene_from_golden(z), _golden_cam(z)
    W, H, D = 61, 45, int(z["depth"])
    ctx.set_option("contract", contract)
    try:
        _setup(ctx, arrays, cam, W, H, D)
        ctx.render(0, 24, 5)
        plain, plain8 = ctx.read_accum(), ctx.resolve_rgb8()
        res = ctx.render_adaptive(0.0, 4, 4, 24, 5)
        n, S1, _, rgb = _state(ctx)
        assert (n == 24).all() and res["active_pixels"] == W * H and res["rounds"] == 6
        assert np.array_equal(S1, plain) and np.array_equal(rgb, plain8)
    finally:
        ctx.set_option("contract", 0)


def _adaptive_state(ctx, arrays, cam, W, H, D, t, rank=0, world=1):
    _setup(ctx, arrays, cam, W, H, D, rank, world)
    ctx.render_adaptive(t, MIN_SPP, STEP, MAX_SPP, 9)
    return _state(ctx)


def test_tile_split_and_work_distribution_change_nothing(ctx):
    z = load_golden("tier_s_cornell.npz")
    arrays, cam = scene_from_golden(z), _golden_cam(z)
    W, H, D = 75, 50, int(z["depth"])
    ref = _adaptive_state(ctx, arrays, cam, W, H, D, 0.1)
    assert len(np.unique(ref[0])) >= 3
    for world in (2, 3):
        for rank in range(world):
            got = _adaptive_state(ctx, arrays, cam, W, H, D, 0.1, rank, world)
            own = AR.owned_mask(W, H, rank, world)
            assert (got[0][~own] == 0).all()
            for a, b in zip(got, ref):
                assert np.array_equal(a[own], b[own]), (rank, world)
    # work distribution: at 160 x 128 one sample of the frame is 320 KiB of sample buffer, so a 1 MiB budget splits every
    # round of 4 samples into passes of 3 + 1
    W, H = 160, 128
    ref = _adaptive_state(ctx, arrays, cam, W, H, D, 0.1)
    try:
        for opts in (dict(pass_bytes=1 << 20, chunk=1), dict(chunk=4, persistent=0), dict(chunk=8, persistent=1),
                     dict(pass_bytes=1 << 20, chunk=1, persistent=1), dict(overlap=0, chunk=2)):
            for k, v in opts.items():
                ctx.set_option(k, v)
            got = _adaptive_state(ctx, arrays, cam, W, H, D, 0.1)
            for a, b in zip(got, ref):
                assert np.array_equal(a, b), opts
            for k, v in dict(pass_bytes=16 << 30, chunk=0, persistent=-1, overlap=1).items():
                ctx.set_option(k, v)
    finally:
        for k, v in dict(pass_bytes=16 << 30, chunk=0, persistent=-1, overlap=1).items():
            ctx.set_option(k, v)


def test_exit_leaves_every_pixel_a_plain_render_of_its_count(ctx):
    from pbrpathtracer_amd import ptk
    z = load_golden("tier_s_glass.npz")
    arrays, cam = scene_from_golden(z), _golden_cam(z)
    W, H, D = 256, 192, int(z["depth"])
    _setup(ctx, arrays, cam, W, H, D)
    timer = threading.Timer(0.05, ctx.request_exit)
    timer.start()
    t0 = time.time()
    res = ctx.render_adaptive(0.0, 2, 2, 4096, 3)          # never converges: only the exit ends it early
    took = time.time() - t0
    timer.join()
    n, S1, S2, rgb = _state(ctx)
    counts = np.unique(n).tolist()
    print(f"exit: {took:.3f} s, counts {counts}, {res}")
    assert res["max_count"] == max(counts) and res["pixel_samples"] == int(n.astype(np.int64).sum())
    other = ptk.Context(0)
    try:
        other.upload_scene(arrays); other.set_camera(**cam); other.set_frame(W, H, D)
        for c in counts:
            other.reset()
            if c:
                other.render(0, c, 3)
            sel = n == c
            assert np.array_equal(other.read_accum()[sel], S1[sel]), c
            if c:
                assert np.array_equal(other.resolve_rgb8()[sel], rgb[sel]), c
    finally:
        other.close()
    # the next render is not cut
    res2 = ctx.render_adaptive(0.0, 2, 2, 4, 3)
    assert res2["max_count"] == 4 and (ctx.read_sample_counts() == 4).all()


def test_call_order_arguments_and_handoff(ctx):
    from pbrpathtracer_amd import ptk
    z = load_golden("tier_s_cornell.npz")
    arrays, cam = scene_from_golden(z), _golden_cam(z)
    W, H, D = 40, 36, int(z["depth"])
    _setup(ctx, arrays, cam, W, H, D)
    L, h = ctx.L, ctx.h
    for args in ((0.1, 8, 1, 32), (0.1, 6, 4, 32), (0.1, 8, 4, 30), (0.1, 16, 4, 8), (float("nan"), 8, 4, 32),
                 (float("inf"), 8, 4, 32), (-0.1, 8, 4, 32)):
        assert L.ptk_render_adaptive(h, *args, 1, None) == -1, args
    assert L.ptk_render_adaptive(h, 0.1, 8, 4, 32, 1, None) == 0
    assert L.ptk_render(h, 32, 4, 1) == -1                  # the accumulator has no single sample count
    ctx.reset()
    ctx.render(0, 8, 1)
    after = ctx.read_accum(), ctx.resolve_rgb8()
    fresh = ptk.Context(0)
    try:
        fresh.upload_scene(arrays); fresh.set_camera(**cam); fresh.set_frame(W, H, D); fresh.reset(); fresh.render(0, 8, 1)
        assert np.array_equal(after[0], fresh.read_accum()) and np.array_equal(after[1], fresh.resolve_rgb8())
    finally:
        fresh.close()
    # a bound hand-off buffer receives the per-pixel-count resolve
    raw = L.ptk_host_alloc(W * H * 3)
    try:
        buf = np.ctypeslib.as_array((ptk.C.c_uint8 * (W * H * 3)).from_address(raw)).reshape(H, W, 3)
        ctx.bind_out_image(buf)
        ctx.render_adaptive(0.15, MIN_SPP, STEP, MAX_SPP, 4)
        ctx.synchronize()
        n = ctx.read_sample_counts()
        assert len(np.unique(n)) >= 2
        assert np.array_equal(buf, AR.resolve_rgb8(ctx.read_accum(), n))
        ctx.bind_out_image(None)
        assert np.array_equal(ctx.resolve_rgb8(), AR.resolve_rgb8(ctx.read_accum(), n))
    finally:
        ctx.bind_out_image(None)
        L.ptk_host_free(raw)


def test_drop_in_class_matches_the_context(ctx, tmp_path):
    from pbrpathtracer_amd import scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer, camera_from_scene
    pts, scene, _ = S.build_config("C1", str(tmp_path), width=64, height=48, depth=4)
    pt = PathTracer(device=0)
    pt.LoadSceneFile(pts)
    out = np.zeros((48, 64, 3), np.uint8)
    pt.SetOutImage(out)
    pt.SetSeed(6)
    res = pt.RenderAdaptive(0.1, MIN_SPP, STEP, MAX_SPP)
    assert pt.LastError() == ""
    n, total = pt.ReadSampleCounts(), pt.ReadAccumulation()
    assert pt.GetSamples() == res["max_count"] == n.max()
    pt.RenderFrame()                                         # refused: nothing is added
    assert np.array_equal(pt.ReadAccumulation(), total) and pt.LastError() != ""
    arrays = pt.StagedScene()
    from pbrpathtracer_amd import ptk
    a = ptk.Context(0)
    try:
        cam = camera_from_scene(scene)
        a.upload_scene(arrays); a.set_camera(**cam); a.set_frame(64, 48, 4); a.reset()
        res2 = a.render_adaptive(0.1, MIN_SPP, STEP, MAX_SPP, 6)
        assert res == res2
        assert np.array_equal(a.read_sample_counts(), n) and np.array_equal(a.read_accum(), total)
        assert np.array_equal(a.resolve_rgb8(), out)
    finally:
        a.close()
