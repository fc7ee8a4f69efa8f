"""Radiance along caller-supplied rays (include/ptk.h ptk_trace_rays) against the CPU oracle, bit for bit: out[i]
is the float32 in-order sum of orc_trace_counter(scene, ro_i, rd_i, depth, seed, key_base + i, sample) over the sample range,
whatever the batching into calls and passes, the cut of the ray set, the builder, the "flat" option and the tile split; with
PTK_RAYS_LENS_DRAWS a camera's own rays reproduce ptk_render's accumulator.  Every comparison is np.array_equal; the rays are NaN-free
and carry light by tests/test_rays_cpu.py."""

import numpy as np
import pytest

import ray_cases as RC

pytestmark = pytest.mark.gpu

N, DEPTH, SEED, FIRST, SPP = 1000, 4, (1 << 40) + 9, 3, 5
PASS_BYTES_DEFAULT = float(16 << 30)


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


_truth = {}


def _case(OB, case):
    """(arrays, ro, rd, oracle's out) of a case at (N, DEPTH, SEED, FIRST, SPP); computed once, not to be modified"""
    if case not in _truth:
        arrays, _ = RC.scene(case)
        ro, rd = RC.rays_in_box(arrays, N, 5)
        o = OB.Oracle(arrays)
        _truth[case] = (arrays, ro, rd, RC.truth(o, ro, rd, DEPTH, SEED, FIRST, SPP))
        o.close()
    return _truth[case]


def _ocam(OB, cam):
    return OB.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])


# ---- 1. radiance equals the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.CASES)
def test_radiance_equals_oracle(ctx, oracle_mod, case):
    arrays, ro, rd, want = _case(oracle_mod, case)
    ctx.upload_scene(arrays)
    got = ctx.trace_rays(ro, rd, DEPTH, FIRST, SPP, SEED)
    assert got.shape == (N, 3) and got.dtype == np.float32
    assert (want != 0).any(axis=1).mean() >= 0.2 and not np.isnan(want).any()
    assert np.array_equal(got, want), (case, int((got != want).any(axis=1).sum()), float(np.abs(got - want).max()))


# ---- 2. ragged sizes -----------------------------------------------------------------------------------------------------------
def test_ragged_sizes(ctx, oracle_mod):
    """Ray counts around the 64-ray group, sample counts of one chunk and of several (19 > 2 x 8) with a partial last one."""
    arrays, _ = RC.scene("s_opacity")
    ro, rd = RC.rays_in_box(arrays, 129, 7)
    o = oracle_mod.Oracle(arrays)
    want = {spp: RC.truth(o, ro, rd, DEPTH, SEED, 0, spp) for spp in (1, 19)}
    o.close()
    ctx.upload_scene(arrays)
    for n in (1, 63, 64, 65, 129):
        for spp in (1, 19):
            got = ctx.trace_rays(ro[:n], rd[:n], DEPTH, 0, spp, SEED)
            assert np.array_equal(got, want[spp][:n]), (n, spp)


# ---- 3. batching into calls and passes -----------------------------------------------------------------------------------------
def test_batching_into_calls_and_passes(ctx, oracle_mod):
    arrays, _ = RC.scene("random300")
    ro, rd = RC.rays_in_box(arrays, 300, 8)
    o = oracle_mod.Oracle(arrays)
    want = RC.truth(o, ro, rd, DEPTH, SEED, 0, 12)
    o.close()
    ctx.upload_scene(arrays)
    one = ctx.trace_rays(ro, rd, DEPTH, 0, 12, SEED)
    assert np.array_equal(one, want)
    two = ctx.trace_rays(ro, rd, DEPTH, 0, 5, SEED)
    back = ctx.trace_rays(ro, rd, DEPTH, 5, 7, SEED, out=two)
    assert back is two and np.array_equal(two, want)
    # Passes.  "pass_bytes" is at least 1 MiB = 1024 groups of 64 rays x one sample: 70 000 rays are 1094 groups, so even one sample
    # of all of them exceeds it - two blocks of rays, each in passes of one sample, later ones folding onto earlier ones.  The
    # oracle checks every 233rd ray (ray i alone, at its own RNG pixel), the one-pass call all of them.
    ro, rd = RC.rays_in_box(arrays, 70000, 10)
    one = ctx.trace_rays(ro, rd, DEPTH, 0, 5, SEED)
    o = oracle_mod.Oracle(arrays)
    for i in range(0, len(ro), 233):
        assert np.array_equal(one[i], RC.truth(o, ro[i:i + 1], rd[i:i + 1], DEPTH, SEED, 0, 5, key_base=i)[0]), i
    o.close()
    try:
        ctx.set_option("pass_bytes", 1 << 20)
        assert np.array_equal(ctx.trace_rays(ro, rd, DEPTH, 0, 5, SEED), one)
        half = ctx.trace_rays(ro, rd, DEPTH, 0, 2, SEED)
        assert np.array_equal(ctx.trace_rays(ro, rd, DEPTH, 2, 3, SEED, out=half), one)
        ctx.set_option("pass_bytes", 3 << 20)       # one block of rays, passes of two samples (and a last one of one)
        assert np.array_equal(ctx.trace_rays(ro, rd, DEPTH, 0, 5, SEED), one)
    finally:
        ctx.set_option("pass_bytes", PASS_BYTES_DEFAULT)


# ---- 4. cutting the ray set ----------------------------------------------------------------------------------------------------
def test_ray_set_splitting_and_key_wrap(ctx, oracle_mod):
    arrays, ro, rd, want = _case(oracle_mod, "random300")
    ctx.upload_scene(arrays)
    a = ctx.trace_rays(ro[:300], rd[:300], DEPTH, FIRST, SPP, SEED)
    b = ctx.trace_rays(ro[300:], rd[300:], DEPTH, FIRST, SPP, SEED, key_base=300)
    assert np.array_equal(np.concatenate([a, b]), want)
    assert not np.array_equal(ctx.trace_rays(ro[300:], rd[300:], DEPTH, FIRST, SPP, SEED), want[300:])
    # RNG pixels 2^32 - 10 ... 2^32 - 1, then 0, 1, ...: as the oracle's uint32 wraps
    kb = 2 ** 32 - 10
    o = oracle_mod.Oracle(arrays)
    wrapped = RC.truth(o, ro[:80], rd[:80], DEPTH, SEED, FIRST, SPP, key_base=kb)
    o.close()
    assert np.array_equal(ctx.trace_rays(ro[:80], rd[:80], DEPTH, FIRST, SPP, SEED, key_base=kb), wrapped)


# ---- 5. lens draws: a camera's own rays reproduce the render ------------------------------------------------------------------
def test_lens_draws_reproduce_render(ctx, oracle_mod):
    OB = oracle_mod
    arrays, cam = RC.scene("s_cornell")
    cam = dict(cam, aperture=0.0)
    W, H, D, spp, seed = 24, 20, 4, 4, 21
    o = OB.Oracle(arrays)
    ocam = _ocam(OB, cam)
    rec = o.render_counted(ocam, W, H, D, 0, 1, seed, dump=True)["rays"]
    ref, _ = o.render(ocam, W, H, D, 0, spp, seed)
    o.close()
    rec = rec[(rec["kind"] == OB.RAY_CAMERA) & (rec["sample"] == 0)]
    rec = rec[np.argsort(rec["pixel"], kind="stable")]
    assert np.array_equal(rec["pixel"], np.arange(W * H))           # one camera ray per pixel, top-down index
    ro, rd = np.ascontiguousarray(rec["ro"]), np.ascontiguousarray(rec["rd"])
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(0, 1); ctx.reset()
    ctx.render(0, spp, seed)
    acc = ctx.read_accum()
    assert np.array_equal(acc, ref) and (ref != 0).any()
    with_draws = ctx.trace_rays(ro, rd, D, 0, spp, seed, lens_draws=True).reshape(H, W, 3)[::-1]
    assert np.array_equal(with_draws, ref) and np.array_equal(with_draws, acc)
    without = ctx.trace_rays(ro, rd, D, 0, spp, seed).reshape(H, W, 3)[::-1]
    assert not np.array_equal(without, ref)


# ---- 6. independence -----------------------------------------------------------------------------------------------------------
def test_independent_of_builder_flat_and_tiles(ctx, oracle_mod):
    try:
        arrays, ro, rd, want = _case(oracle_mod, "random6000")
        for device_build in (0, 1):
            ctx.set_option("device_build", device_build)
            ctx.upload_scene(arrays)
            assert ctx.upload_timing()["built_on_device"] == bool(device_build)
            assert np.array_equal(ctx.trace_rays(ro, rd, DEPTH, FIRST, SPP, SEED), want), device_build
        ctx.set_tile(1, 3)
        assert np.array_equal(ctx.trace_rays(ro, rd, DEPTH, FIRST, SPP, SEED), want)
        arrays, ro, rd, want = _case(oracle_mod, "random16")
        ctx.upload_scene(arrays)
        for flat in (0, 1):
            ctx.set_option("flat", flat)
            assert np.array_equal(ctx.trace_rays(ro, rd, DEPTH, FIRST, SPP, SEED), want), flat
    finally:
        ctx.set_option("device_build", 1); ctx.set_option("flat", 1); ctx.set_tile(0, 1)


def test_leaves_the_frame_state_alone(ctx, oracle_mod):
    """After an adaptive render and a feature pass: the accumulator, the sample count, the per-pixel counts, the 8-bit image and the
    feature plane are what they were, and the call is legal (a plain render is not, until the next reset)."""
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, want = _case(oracle_mod, "random300")
    _, cam = RC.scene("random300")
    W, H = 40, 24
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, DEPTH); ctx.set_tile(0, 1); ctx.reset()
    ctx.render_adaptive(0.05, 4, 2, 8, 3)
    ctx.render_features(1 << ptk.FEAT_DEPTH, 0, 3)
    before = (ctx.read_accum(), ctx.samples(), ctx.read_sample_counts(), ctx.resolve_rgb8(), ctx.read_feature(ptk.FEAT_DEPTH))
    assert np.array_equal(ctx.trace_rays(ro, rd, DEPTH, FIRST, SPP, SEED), want)
    after = (ctx.read_accum(), ctx.samples(), ctx.read_sample_counts(), ctx.resolve_rgb8(), ctx.read_feature(ptk.FEAT_DEPTH))
    assert before[1] == after[1]
    for b, a in zip(before, after):
        assert np.array_equal(b, a)
    with pytest.raises(ptk.PtkError):
        ctx.render(8, 1, 3)
    ctx.reset()


def test_needs_no_camera_and_no_frame(oracle_mod):
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, want = _case(oracle_mod, "s_glass")
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays)
        assert np.array_equal(c.trace_rays(ro, rd, DEPTH, FIRST, SPP, SEED), want)
    finally:
        c.close()


# ---- 7. edits are seen ---------------------------------------------------------------------------------------------------------
def test_material_and_geometry_edits_are_seen(ctx, oracle_mod):
    arrays, ro, rd, want = _case(oracle_mod, "random300")
    ctx.upload_scene(arrays)
    assert np.array_equal(ctx.trace_rays(ro, rd, DEPTH, FIRST, SPP, SEED), want)
    # the sure light's colour (tests/test_gpu_random_scenes.py: material 0)
    edited = dict(arrays); edited["materials"] = arrays["materials"].copy()
    edited["materials"][0]["emissive"] = (0.2, 1.0, 0.4)
    o = oracle_mod.Oracle(edited)
    want_m = RC.truth(o, ro, rd, DEPTH, SEED, FIRST, SPP)
    o.close()
    assert not np.array_equal(want_m, want)
    ctx.update_materials(edited["materials"])
    assert np.array_equal(ctx.trace_rays(ro, rd, DEPTH, FIRST, SPP, SEED), want_m)
    # ... then a third of the triangles move
    n = len(arrays["verts"])
    a, b = n // 3, (2 * n) // 3
    moved = dict(edited); moved["verts"] = arrays["verts"].copy()
    moved["verts"][a:b] = (arrays["verts"][a:b].reshape(-1, 3, 3) + np.array([0.3, 0.15, -0.2], np.float32)).reshape(-1, 9)
    o = oracle_mod.Oracle(moved)
    want_g = RC.truth(o, ro, rd, DEPTH, SEED, FIRST, SPP)
    o.close()
    assert not np.array_equal(want_g, want_m)
    ctx.update_geometry(a, moved["verts"][a:b])
    assert np.array_equal(ctx.trace_rays(ro, rd, DEPTH, FIRST, SPP, SEED), want_g)


# ---- 8. the device entry -------------------------------------------------------------------------------------------------------
def test_device_entry_and_caller_stream(oracle_mod):
    import torch
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, want = _case(oracle_mod, "random300")
    dev = torch.device("cuda:0")
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays)
        host = c.trace_rays(ro, rd, DEPTH, FIRST, SPP, SEED)
        assert np.array_equal(host, want)
        # on the context's own stream: the caller synchronises around the call
        t_ro, t_rd = torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev)
        torch.cuda.synchronize()
        out = c.trace_rays(t_ro, t_rd, DEPTH, FIRST, SPP, SEED)
        c.synchronize()
        assert isinstance(out, torch.Tensor) and out.device == t_ro.device and tuple(out.shape) == (N, 3)
        assert np.array_equal(out.cpu().numpy(), host)
        # two device calls that continue each other
        part = c.trace_rays(t_ro, t_rd, DEPTH, FIRST, 2, SEED)
        assert c.trace_rays(t_ro, t_rd, DEPTH, FIRST + 2, SPP - 2, SEED, out=part) is part
        c.synchronize()
        assert np.array_equal(part.cpu().numpy(), host)
        # on a caller's stream, with no host wait: the inputs are filled on that stream behind a long kernel, the result is read on it
        s = torch.cuda.Stream(device=dev)
        c.set_stream(s.cuda_stream)
        big = torch.randn(2048, 2048, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            f_ro, f_rd = torch.zeros_like(t_ro), torch.zeros_like(t_rd)
            for _ in range(8):
                big = big @ big * 1e-3
            f_ro.copy_(t_ro); f_rd.copy_(t_rd)
            res = c.trace_rays(f_ro, f_rd, DEPTH, FIRST, SPP, SEED)
            snap = res.clone()
        s.synchronize()
        assert np.array_equal(snap.cpu().numpy(), host)
    finally:
        c.close()


# ---- 9. arguments --------------------------------------------------------------------------------------------------------------
def test_arguments(ctx, oracle_mod):
    from pbrpathtracer_amd import ptk
    arrays, ro, rd, want = _case(oracle_mod, "s_cornell")
    L = ptk.load()
    n = 10
    o, d = ro[:n].copy(), rd[:n].copy()
    out = np.zeros((n, 3), np.float32)
    po, pd, pout = o.ctypes.data, d.ctypes.data, out.ctypes.data
    BAD = -1
    fresh = ptk.Context(0)
    try:
        for fn in (L.ptk_trace_rays, L.ptk_trace_rays_device):
            assert fn(fresh.h, n, po, pd, DEPTH, 0, 1, 0, 0, 0, pout) == BAD          # before ptk_upload_scene
    finally:
        fresh.close()
    ctx.upload_scene(arrays)
    for fn in (L.ptk_trace_rays, L.ptk_trace_rays_device):
        assert fn(None, n, po, pd, DEPTH, 0, 1, 0, 0, 0, pout) == BAD                 # null context
        assert fn(ctx.h, n, None, pd, DEPTH, 0, 1, 0, 0, 0, pout) == BAD              # null arrays
        assert fn(ctx.h, n, po, None, DEPTH, 0, 1, 0, 0, 0, pout) == BAD
        assert fn(ctx.h, n, po, pd, DEPTH, 0, 1, 0, 0, 0, None) == BAD
        assert fn(ctx.h, -1, po, pd, DEPTH, 0, 1, 0, 0, 0, pout) == BAD               # negative count
        assert fn(ctx.h, n, po, pd, DEPTH, 0, 1, 0, 0, 4, pout) == BAD                # unknown flag bits
        assert fn(ctx.h, n, po, pd, DEPTH, 0, 1, 0, 0, 0x80000001, pout) == BAD
        assert fn(ctx.h, 0, None, None, DEPTH, 0, 1, 0, 0, 0, None) == 0              # no rays: nothing to do
    assert L.ptk_last_rays_ms(None, None, None) == BAD
    empty = ctx.trace_rays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), DEPTH, 0, 4, SEED)
    assert empty.shape == (0, 3)
    # no samples: zeroes out, or leaves it alone when it is to be added to
    out[:] = 7.0
    assert L.ptk_trace_rays(ctx.h, n, po, pd, DEPTH, 0, 0, 0, 0, 0, pout) == 0 and (out == 0).all()
    keep = want[:n].copy()
    assert np.array_equal(ctx.trace_rays(o, d, DEPTH, 5, 0, SEED, out=keep), want[:n])
    # a depth limit <= 0 (ptk_set_frame takes it too) ends every path at its first interaction: black
    assert (ctx.trace_rays(o, d, 0, 0, 2, SEED) == 0).all()
    t, f = ctx.last_rays_ms()
    assert t > 0 and f > 0


# ---- 10. host class and command line -------------------------------------------------------------------------------------------
def test_host_class_and_equirect_cli(oracle_mod, tmp_path):
    from pbrpathtracer_amd import render, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    from pbrpathtracer_amd.rays import equirect_rays
    pts, _, _ = S.build_config("C1", str(tmp_path), width=32, height=24, depth=4)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    pt.SetSeed(5)
    arrays = pt.StagedScene()
    depth = pt.GetTraceDepth()
    ro, rd = RC.rays_in_box(arrays, 200, 9)
    o = oracle_mod.Oracle(arrays)
    want = RC.truth(o, ro, rd, depth, 5, 1, 3, key_base=17)
    got = pt.TraceRays(ro, rd, 1, 3, key_base=17)                                    # no resolution work, no render before it
    assert pt.LastError() == "" and np.array_equal(got, want) and (want != 0).any()
    assert np.array_equal(pt.context().trace_rays(ro, rd, depth, 1, 3, 5, key_base=17), want)
    part = pt.TraceRays(ro, rd, 1, 1, key_base=17)
    assert np.array_equal(pt.TraceRays(ro, rd, 2, 2, key_base=17, out=part), want)
    cam = pt.GetCamera()
    pt.close()
    png, npy = str(tmp_path / "pano.png"), str(tmp_path / "pano.npy")
    assert render.main([pts, "--equirect", "16", "--spp", "3", "--seed", "5", "-o", png, "--npy", npy]) == 0
    total = np.load(npy)
    assert total.shape == (8, 16, 3) and total.dtype == np.float32
    e_ro, e_rd = equirect_rays(*cam, 16, 8)
    want_pano = RC.truth(o, e_ro, e_rd, depth, 5, 0, 3)
    o.close()
    assert np.array_equal(total.reshape(-1, 3), want_pano) and (want_pano != 0).any()
    from pbrpathtracer_amd.pathtracer import image_load
    img = image_load(png)
    x = np.clip(want_pano.reshape(8, 16, 3) / np.float32(3), 0, 1).astype(np.float32)
    assert img is not None and np.array_equal(img[..., :3], (x * np.float32(255)).astype(np.uint8))
