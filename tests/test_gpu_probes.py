"""Irradiance probe baking (include/ptk.h ptk_bake_probes, ptk_probes_irradiance) against numpy and the CPU oracle,
bit for bit: the radiance table is the float32 in-order sum of orc_trace_counter along every (probe, direction) ray on the stream
keyed by the ray's index - what ptk_trace_rays gives for the expanded ray list -, the coefficients are the float32 restatement of
tests/probe_cases.py, whatever the batching into calls, blocks of probes and passes, the builder, "flat", the tile split and the
frame state; the irradiance lookup equals numpy.  Every comparison is np.array_equal; the cases carry light and are NaN-free by
tests/test_probes_cpu.py."""
import numpy as np
import pytest

import probe_cases as PC
import ray_cases as RC
from pbrpathtracer_amd.probes import fibonacci_dirs, grid_over_bounds, grid_positions, sh_weight

pytestmark = pytest.mark.gpu

F = np.float32
DEPTH, SEED, FIRST, SPP = PC.DEPTH, (1 << 40) + 9, PC.FIRST, PC.SPP
WEIGHT = sh_weight(PC.D, SPP)
PASS_BYTES_DEFAULT = float(16 << 30)


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


_truth = {}


def _case(OB, case):
    """(arrays, positions, dirs, oracle's S, coefs) of a case at (DEPTH, SEED, FIRST, SPP, WEIGHT); computed once, not to be modified"""
    if case not in _truth:
        arrays, _ = RC.scene(case)
        pos, dirs = PC.probes(case)
        o = OB.Oracle(arrays)
        S, coefs = PC.truth_probes(o, pos, dirs, DEPTH, SEED, FIRST, SPP, WEIGHT)
        o.close()
        _truth[case] = (arrays, pos, dirs, S, coefs)
    return _truth[case]


def _bake(c, t, first=FIRST, spp=SPP, weight=WEIGHT, **kw):
    return c.bake_probes(t[1], t[2], DEPTH, first, spp, SEED, weight, **kw)


# ---- 1. the table and the coefficients equal the oracle and numpy ---------------------------------------------------------------
@pytest.mark.parametrize("case", list(PC.CASES))
def test_bake_equals_truth(ctx, oracle_mod, case):
    t = _case(oracle_mod, case)
    ctx.upload_scene(t[0])
    S, coefs = _bake(ctx, t)
    assert S.shape == (PC.P, PC.D, 3) and coefs.shape == (PC.P, 9, 3) and S.dtype == coefs.dtype == F
    assert np.array_equal(S, t[3]), (case, int((S != t[3]).any(axis=2).sum()))
    assert np.array_equal(coefs, t[4]), (case, float(np.abs(coefs - t[4]).max()))
    # without a table of the caller's the projection comes from the context's own
    none, coefs2 = _bake(ctx, t, want_radiance=False)
    assert none is None and np.array_equal(coefs2, t[4])


def test_radiance_equals_trace_rays(ctx, oracle_mod):
    t = _case(oracle_mod, "random300")
    ctx.upload_scene(t[0])
    ro, rd = PC.expand(t[1], t[2])
    rays = ctx.trace_rays(ro, rd, DEPTH, FIRST, SPP, SEED, key_base=77)
    S, coefs = _bake(ctx, t, key_base=77)
    assert np.array_equal(S.reshape(-1, 3), rays) and np.array_equal(coefs, PC.project(S, t[2], WEIGHT))


# ---- 2. batching: calls, blocks of probes, passes; keys -------------------------------------------------------------------------
def test_two_accumulating_calls_equal_one(ctx, oracle_mod):
    t = _case(oracle_mod, "s_glass")
    ctx.upload_scene(t[0])
    part, c_part = _bake(ctx, t, first=FIRST, spp=2)
    assert not np.array_equal(c_part, t[4])
    back, coefs = _bake(ctx, t, first=FIRST + 2, spp=1, radiance=part)
    assert back is part and np.array_equal(part, t[3]) and np.array_equal(coefs, t[4])


def test_blocks_of_probes_and_passes(ctx):
    """"pass_bytes" at its smallest, 1 MiB: blocks of 4096 rays = 85 whole probes of 48 directions - 200 probes are three blocks, the
    last of 30 -, and each block's 64 groups of rays take 16 samples per pass: 37 samples are three passes."""
    arrays, _ = RC.scene("random300")
    pos = RC.rays_in_box(arrays, 200, 3)[0]
    dirs = fibonacci_dirs(48)
    w = sh_weight(48, 37)
    ctx.upload_scene(arrays)
    S, coefs = ctx.bake_probes(pos, dirs, DEPTH, 0, 37, SEED, w)
    assert (S != 0).any(axis=2).mean() > 0.2 and np.array_equal(coefs, PC.project(S, dirs, w))
    try:
        ctx.set_option("pass_bytes", 1 << 20)
        S2, coefs2 = ctx.bake_probes(pos, dirs, DEPTH, 0, 37, SEED, w)
        assert np.array_equal(S2, S) and np.array_equal(coefs2, coefs)
        _, coefs3 = ctx.bake_probes(pos, dirs, DEPTH, 0, 37, SEED, w, want_radiance=False)
        assert np.array_equal(coefs3, coefs)
        half, _ = ctx.bake_probes(pos, dirs, DEPTH, 0, 20, SEED, w)
        S4, coefs4 = ctx.bake_probes(pos, dirs, DEPTH, 20, 17, SEED, w, radiance=half)
        assert np.array_equal(S4, S) and np.array_equal(coefs4, coefs)
    finally:
        ctx.set_option("pass_bytes", PASS_BYTES_DEFAULT)


def test_key_base_and_wrap(ctx, oracle_mod):
    t = _case(oracle_mod, "s_cornell")
    ctx.upload_scene(t[0])
    o = oracle_mod.Oracle(t[0])
    for kb in (1000, 2 ** 32 - 100):            # 336 rays: the second wraps inside the second probe
        S, coefs = PC.truth_probes(o, t[1], t[2], DEPTH, SEED, FIRST, 2, WEIGHT, key_base=kb)
        got_S, got_c = _bake(ctx, t, spp=2, key_base=kb)
        assert np.array_equal(got_S, S) and np.array_equal(got_c, coefs) and not np.array_equal(got_S[1:], t[3][1:]), kb
    o.close()


@pytest.mark.parametrize("P,D", [(1, 1), (3, 65), (4, 16)])
def test_shapes(ctx, oracle_mod, P, D):
    """one ray; a direction count one above the 64-ray group; exactly one group"""
    arrays, _ = RC.scene("s_opacity")
    pos = RC.rays_in_box(arrays, P, 4)[0]
    dirs = fibonacci_dirs(D)
    o = oracle_mod.Oracle(arrays)
    S, coefs = PC.truth_probes(o, pos, dirs, DEPTH, SEED, 0, 2, 0.25)
    o.close()
    ctx.upload_scene(arrays)
    got_S, got_c = ctx.bake_probes(pos, dirs, DEPTH, 0, 2, SEED, 0.25)
    assert got_S.shape == (P, D, 3) and np.array_equal(got_S, S) and np.array_equal(got_c, coefs)
    assert (S != 0).any() or P * D == 1


# ---- 3. independence ------------------------------------------------------------------------------------------------------------
def test_independent_of_builder_flat_and_tiles(ctx, oracle_mod):
    try:
        t = _case(oracle_mod, "random6000")
        for device_build in (0, 1):
            ctx.set_option("device_build", device_build)
            ctx.upload_scene(t[0])
            S, coefs = _bake(ctx, t)
            assert np.array_equal(S, t[3]) and np.array_equal(coefs, t[4]), device_build
        ctx.set_tile(1, 3)
        assert np.array_equal(_bake(ctx, t)[1], t[4])
        t = _case(oracle_mod, "s_cornell")
        ctx.upload_scene(t[0])
        for flat in (0, 1):
            ctx.set_option("flat", flat)
            S, coefs = _bake(ctx, t)
            assert np.array_equal(S, t[3]) and np.array_equal(coefs, t[4]), flat
    finally:
        ctx.set_option("device_build", 1); ctx.set_option("flat", 1); ctx.set_tile(0, 1)


def test_leaves_the_frame_state_alone(ctx, oracle_mod):
    t = _case(oracle_mod, "random300")
    _, cam = RC.scene("random300")
    ctx.upload_scene(t[0]); ctx.set_camera(**cam); ctx.set_frame(40, 24, DEPTH); ctx.set_tile(0, 1); ctx.reset()
    ctx.render_adaptive(0.05, 4, 2, 8, 3)
    before = (ctx.read_accum(), ctx.samples(), ctx.read_sample_counts(), ctx.resolve_rgb8())
    S, coefs = _bake(ctx, t)
    assert np.array_equal(S, t[3]) and np.array_equal(coefs, t[4])
    after = (ctx.read_accum(), ctx.samples(), ctx.read_sample_counts(), ctx.resolve_rgb8())
    assert before[1] == after[1]
    for b, a in zip(before, after):
        assert np.array_equal(b, a)
    ctx.reset()


def test_needs_no_camera_and_no_frame(oracle_mod):
    from pbrpathtracer_amd import ptk
    t = _case(oracle_mod, "s_glass")
    c = ptk.Context(0)
    try:
        c.upload_scene(t[0])
        S, coefs = _bake(c, t)
        assert np.array_equal(S, t[3]) and np.array_equal(coefs, t[4])
    finally:
        c.close()


# ---- 4. edits are seen ----------------------------------------------------------------------------------------------------------
def test_material_and_geometry_edits_are_seen(ctx, oracle_mod):
    arrays, pos, dirs, S, coefs = _case(oracle_mod, "random300")
    ctx.upload_scene(arrays)
    edited = dict(arrays); edited["materials"] = arrays["materials"].copy()
    edited["materials"][0]["emissive"] = (0.2, 1.0, 0.4)
    o = oracle_mod.Oracle(edited)
    S_m, c_m = PC.truth_probes(o, pos, dirs, DEPTH, SEED, FIRST, SPP, WEIGHT)
    o.close()
    assert not np.array_equal(S_m, S)
    ctx.update_materials(edited["materials"])
    got = ctx.bake_probes(pos, dirs, DEPTH, FIRST, SPP, SEED, WEIGHT)
    assert np.array_equal(got[0], S_m) and np.array_equal(got[1], c_m)
    moved = dict(edited); moved["verts"] = arrays["verts"].copy()
    moved["verts"][:150] = (arrays["verts"][:150].reshape(-1, 3, 3) + np.array([0.3, 0.15, -0.2], F)).reshape(-1, 9)
    o = oracle_mod.Oracle(moved)
    S_g, c_g = PC.truth_probes(o, pos, dirs, DEPTH, SEED, FIRST, SPP, WEIGHT)
    o.close()
    assert not np.array_equal(S_g, S_m)
    ctx.update_geometry(0, moved["verts"][:150])
    got = ctx.bake_probes(pos, dirs, DEPTH, FIRST, SPP, SEED, WEIGHT)
    assert np.array_equal(got[0], S_g) and np.array_equal(got[1], c_g)


# ---- 5. the device entries ------------------------------------------------------------------------------------------------------
def test_device_entries_and_caller_stream(oracle_mod):
    import torch
    from pbrpathtracer_amd import ptk
    arrays, pos, dirs, S, coefs = _case(oracle_mod, "random300")
    dev = torch.device("cuda:0")
    dims, origin, spacing = (7, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)          # the seven probes as a row
    pts, nrm = PC.queries(dims, origin, spacing, 200, 6)
    want_E = PC.irradiance(dims, origin, spacing, coefs, pts, nrm)
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays)
        t_pos, t_dirs = torch.from_numpy(pos).to(dev), torch.from_numpy(dirs).to(dev)
        torch.cuda.synchronize()
        got_S, got_c = c.bake_probes(t_pos, t_dirs, DEPTH, FIRST, SPP, SEED, WEIGHT)
        c.synchronize()
        assert isinstance(got_S, torch.Tensor) and tuple(got_S.shape) == (PC.P, PC.D, 3) and tuple(got_c.shape) == (PC.P, 9, 3)
        assert np.array_equal(got_S.cpu().numpy(), S) and np.array_equal(got_c.cpu().numpy(), coefs)
        part, _ = c.bake_probes(t_pos, t_dirs, DEPTH, FIRST, 1, SEED, WEIGHT)
        back, c2 = c.bake_probes(t_pos, t_dirs, DEPTH, FIRST + 1, SPP - 1, SEED, WEIGHT, radiance=part)
        c.synchronize()
        assert back is part and np.array_equal(part.cpu().numpy(), S) and np.array_equal(c2.cpu().numpy(), coefs)
        none, c3 = c.bake_probes(t_pos, t_dirs, DEPTH, FIRST, SPP, SEED, WEIGHT, want_radiance=False)
        c.synchronize()
        assert none is None and np.array_equal(c3.cpu().numpy(), coefs)
        s = torch.cuda.Stream(device=dev)
        c.set_stream(s.cuda_stream)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            f_pos = torch.zeros_like(t_pos)
            f_pos.copy_(t_pos)
            r_S, r_c = c.bake_probes(f_pos, t_dirs, DEPTH, FIRST, SPP, SEED, WEIGHT)
            snap = r_c.clone()
            E = c.probes_irradiance(dims, origin, spacing, r_c, torch.from_numpy(pts).to(dev, non_blocking=False),
                                    torch.from_numpy(nrm).to(dev, non_blocking=False))
            E_snap = E.clone()
        s.synchronize()
        assert np.array_equal(snap.cpu().numpy(), coefs) and np.array_equal(r_S.cpu().numpy(), S)
        assert np.array_equal(E_snap.cpu().numpy(), want_E, equal_nan=True)
    finally:
        c.close()


# ---- 6. no samples, arguments ---------------------------------------------------------------------------------------------------
def test_no_samples(ctx, oracle_mod):
    t = _case(oracle_mod, "s_cornell")
    ctx.upload_scene(t[0])
    S, coefs = _bake(ctx, t, spp=0)
    assert (S == 0).all() and (coefs == 0).all()
    keep = t[3].copy()
    S, coefs = _bake(ctx, t, first=9, spp=0, radiance=keep)
    assert S is keep and np.array_equal(keep, t[3]) and np.array_equal(coefs, t[4])


def test_arguments(ctx, oracle_mod):
    import ctypes as C
    from pbrpathtracer_amd import ptk
    arrays, pos, dirs, S, coefs = _case(oracle_mod, "s_cornell")
    L = ptk.load()
    P, D = PC.P, PC.D
    rad = np.zeros((P, D, 3), F); co = np.full((P, 9, 3), 7.0, F)
    pp, pd, pr, pc = pos.ctypes.data, dirs.ctypes.data, rad.ctypes.data, co.ctypes.data
    BAD = -1
    bakes = (L.ptk_bake_probes, L.ptk_bake_probes_device)

    def err(c):
        return L.ptk_last_error(c.h).decode()

    fresh = ptk.Context(0)
    try:
        for fn in bakes:
            assert fn(fresh.h, P, pp, D, pd, DEPTH, 0, 1, 0, 0, 0, 1.0, pr, pc) == BAD and "ptk_upload_scene" in err(fresh)
        # the lookup needs no scene
        g = PC.irradiance((1, 1, 1), (0, 0, 0), (1, 1, 1), coefs[0], pos, dirs[:P])
        assert np.array_equal(fresh.probes_irradiance((1, 1, 1), (0, 0, 0), (1, 1, 1), coefs[0], pos, dirs[:P]), g)
    finally:
        fresh.close()
    ctx.upload_scene(arrays)
    inf, nan = float("inf"), float("nan")
    for fn in bakes:
        assert fn(None, P, pp, D, pd, DEPTH, 0, 1, 0, 0, 0, 1.0, pr, pc) == BAD                                  # null context
        assert fn(ctx.h, -1, pp, D, pd, DEPTH, 0, 1, 0, 0, 0, 1.0, pr, pc) == BAD and "negative" in err(ctx)
        assert fn(ctx.h, P, pp, -1, pd, DEPTH, 0, 1, 0, 0, 0, 1.0, pr, pc) == BAD and "negative" in err(ctx)
        for d in (0, 65537):
            assert fn(ctx.h, P, pp, d, pd, DEPTH, 0, 1, 0, 0, 0, 1.0, pr, pc) == BAD and "65536" in err(ctx)
        assert fn(ctx.h, 32768, pp, 65536, pd, DEPTH, 0, 1, 0, 0, 0, 1.0, pr, pc) == BAD and "2^31" in err(ctx)
        for a, b, c in ((None, pd, pc), (pp, None, pc), (pp, pd, None)):
            assert fn(ctx.h, P, a, D, b, DEPTH, 0, 1, 0, 0, 0, 1.0, pr, c) == BAD and "null" in err(ctx)
        assert fn(ctx.h, P, pp, D, pd, DEPTH, 0, 1, 0, 0, 1, 1.0, None, pc) == BAD and "ACCUMULATE" in err(ctx)
        for fl in (2, 0x80000001):
            assert fn(ctx.h, P, pp, D, pd, DEPTH, 0, 1, 0, 0, fl, 1.0, pr, pc) == BAD and "flag" in err(ctx)
        for w in (inf, -inf, nan):
            assert fn(ctx.h, P, pp, D, pd, DEPTH, 0, 1, 0, 0, 0, w, pr, pc) == BAD and "weight" in err(ctx)
        # zero probes: nothing to do, whatever the other arguments
        assert fn(ctx.h, 0, None, 0, None, DEPTH, 0, 1, 0, 0, 0, 1.0, None, None) == 0
    assert (co == 7.0).all() and (rad == 0).all()
    assert L.ptk_bake_probes(ctx.h, P, pp, D, pd, DEPTH, FIRST, SPP, SEED, 0, 0, WEIGHT, None, pc) == 0          # radiance is optional
    assert np.array_equal(co, coefs)
    ms = ctx.last_probes_ms()
    assert ms["raygen_ms"] > 0 and ms["trace_ms"] > 0 and ms["project_ms"] > 0
    assert L.ptk_last_probes_ms(None, None, None, None) == BAD

    I3, F3 = C.c_int32 * 3, C.c_float * 3
    out = np.full((P, 3), 7.0, F)
    po = out.ctypes.data
    nrm = np.ascontiguousarray(dirs[:P])
    pn = nrm.ctypes.data
    for fn in (L.ptk_probes_irradiance, L.ptk_probes_irradiance_device):
        ok = (I3(7, 1, 1), F3(0, 0, 0), F3(1, 1, 1))
        assert fn(None, *ok, pc, P, pp, pn, po) == BAD
        assert fn(ctx.h, *ok, pc, -1, pp, pn, po) == BAD and "negative" in err(ctx)
        for dims in ((0, 1, 1), (7, -1, 1), (7, 1, 0)):
            assert fn(ctx.h, I3(*dims), ok[1], ok[2], pc, P, pp, pn, po) == BAD and "dims" in err(ctx)
        for sp in ((0, 1, 1), (1, -1, 1), (1, 1, inf), (nan, 1, 1)):
            assert fn(ctx.h, ok[0], ok[1], F3(*sp), pc, P, pp, pn, po) == BAD and "spacing" in err(ctx)
        for og in ((inf, 0, 0), (0, nan, 0), (0, 0, -inf)):
            assert fn(ctx.h, ok[0], F3(*og), ok[2], pc, P, pp, pn, po) == BAD and "origin" in err(ctx)
        for a, b, c, d in ((None, pp, pn, po), (pc, None, pn, po), (pc, pp, None, po), (pc, pp, pn, None)):
            assert fn(ctx.h, *ok, a, P, b, c, d) == BAD and "null" in err(ctx)
        assert fn(ctx.h, None, ok[1], ok[2], pc, P, pp, pn, po) == BAD
        assert fn(ctx.h, *ok, None, 0, None, None, None) == 0                                                    # zero points
    assert (out == 7.0).all()


# ---- 7. the irradiance lookup equals numpy --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(3, 2, 2), (1, 1, 1), (4, 1, 3)])
def test_irradiance_equals_numpy(ctx, dims):
    import torch
    rng = np.random.default_rng(sum(dims))
    origin, spacing = (-1.0, 0.5, 2.0), (0.5, 1.25, 0.3)
    coefs = rng.uniform(-1, 2, (dims[2], dims[1], dims[0], 9, 3)).astype(F)
    pts, nrm = PC.queries(dims, origin, spacing, 1000, 9)
    want = PC.irradiance(dims, origin, spacing, coefs, pts, nrm)
    assert np.isfinite(want).all() and np.isnan(pts).any()
    got = ctx.probes_irradiance(dims, origin, spacing, coefs, pts, nrm)
    assert got.shape == (1000, 3) and got.dtype == F
    assert np.array_equal(got, want), int((got != want).any(axis=1).sum())
    t = [torch.from_numpy(a).cuda() for a in (coefs, pts, nrm)]
    torch.cuda.synchronize()
    dev = ctx.probes_irradiance(dims, origin, spacing, *t)
    ctx.synchronize()
    assert np.array_equal(dev.cpu().numpy(), want)


# ---- 8. host class and command line ---------------------------------------------------------------------------------------------
def test_host_class_and_probes_cli(oracle_mod, tmp_path):
    from pbrpathtracer_amd import render, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    pts, _, _ = S.build_config("C1", str(tmp_path), width=32, height=24, depth=4)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    pt.SetSeed(5)
    arrays = pt.StagedScene()
    depth = pt.GetTraceDepth()
    dims, D = (2, 1, 2), 16
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    origin, spacing = grid_over_bounds(v.min(axis=0), v.max(axis=0), dims)
    pos, dirs, w = grid_positions(dims, origin, spacing), fibonacci_dirs(D), sh_weight(D, 3)
    o = oracle_mod.Oracle(arrays)
    want_S, want_c = PC.truth_probes(o, pos, dirs, depth, 5, 0, 3, w)
    o.close()
    got_S, got_c = pt.BakeProbes(pos, dirs, 0, 3, w)                              # no resolution set, no render before it
    assert pt.LastError() == "" and np.array_equal(got_S, want_S) and np.array_equal(got_c, want_c) and (want_c != 0).any()
    part, _ = pt.BakeProbes(pos, dirs, 0, 1, w)
    both_S, both_c = pt.BakeProbes(pos, dirs, 1, 2, w, radiance=part)
    assert both_S is part and np.array_equal(both_S, want_S) and np.array_equal(both_c, want_c)
    qp, qn = PC.queries(dims, origin, spacing, 300, 2)
    want_E = PC.irradiance(dims, origin, spacing, want_c, qp, qn)
    assert np.array_equal(pt.SampleProbes(dims, origin, spacing, got_c, qp, qn), want_E)
    pt.close()
    npz = str(tmp_path / "probes.npz")
    assert render.main([pts, "--bake-probes", "2", "1", "2", "--probe-dirs", "16", "--spp", "3", "--seed", "5", "-o", npz]) == 0
    z = np.load(npz)
    assert z["coefs"].shape == (2, 1, 2, 9, 3) and z["coefs"].dtype == F and np.array_equal(z["coefs"].reshape(-1, 9, 3), want_c)
    assert np.array_equal(z["dims"], dims) and np.array_equal(z["origin"], origin) and np.array_equal(z["spacing"], spacing)
    # the file round-trips into the lookup
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    try:
        assert np.array_equal(c.probes_irradiance(z["dims"], z["origin"], z["spacing"], z["coefs"], qp, qn), want_E)
    finally:
        c.close()
