"""Temporal reprojection (include/ptk.h ptk_get_view, ptk_reproject_planes, ptk_temporal_frame) on the GPU: every output array_equal -
dtype and shape included - to tests/temporal_rule.py, the numpy float32 restatement of the header's rule.  The planes entry over
sizes that split blocks and push taps over every edge; the frame entry chained over camera moves after plain, adaptive and
tile-split renders; what the calls must not touch; refusals; the host class; and one check that the feature does its job."""
import ctypes as C
import math

import numpy as np
import pytest

import denoise_rule as DR
import feature_truth as FT
import ray_cases as RC
import temporal_rule as TR

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD_ARG = -1            # PTK_ERR_BAD_ARG
W, H = 96, 64


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def same(got, want):
    """array_equal with dtype and shape; NaN == NaN (an invalid pixel may hold one and keeps its bits)"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def same2(got, want):
    return same(got[0], want[0]) and same(got[1], want[1])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def diff(got, want):
    return np.argwhere(~((got[1] == want[1]) | (np.isnan(got[1]) & np.isnan(want[1]))))[:3].tolist()


# ---- the planes entries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 35), (130, 70)])
def test_planes_equal_the_mirror(ctx, w, h):
    import torch
    case = TR.random_case(w, h, seed=w + h)
    cur, hist = case["current"], case["history"]
    rng = np.random.default_rng(w)
    # the identity view: other colours and counts over the current frame's own geometry
    _, same_geometry = TR.planes_under(TR.orbit_camera(13.0), w, h, rng)
    assert np.array_equal(same_geometry[2], cur[2])
    # a camera outside the box that looks away from it: s <= 0 for every point
    away = TR.orbit_camera(180.0, distance=3.0)
    away["dir"] = (-np.asarray(away["dir"])).astype(f32)
    setups = [("moved", case["hist_view"], hist), ("identity", case["view"], same_geometry), ("behind", TR.view_of(away, w, h), hist)]
    dev = torch.device("cuda", ctx.device_ordinal())
    to = lambda planes: [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in planes]
    tcur = to(cur)
    inv = cur[2] < 0
    for name, view, history in setups:
        thist = to(history)
        torch.cuda.synchronize()
        for match in (0, 1):
            for max_history in (1.0, 64.0):
                p = TR.params(case["extent"] / 100.0, 0.9, max_history, match)
                want = TR.reproject(view, cur, history, p, want_found=True)
                got = ctx.reproject_planes(view, cur, history, p)
                again = ctx.reproject_planes(view, cur, history, p)
                dgot = ctx.reproject_planes(view, tcur, thist, p)
                ctx.synchronize()
                tag = (w, h, name, match, max_history)
                assert same2(got, want), (tag, diff(got, want))
                assert same2(again, want), tag
                assert same2([t.cpu().numpy() for t in dgot], want), tag
                assert np.array_equal(bits(got[0])[inv], bits(cur[0])[inv]) and np.array_equal(bits(got[1])[inv], bits(cur[1])[inv])
                assert np.isfinite(got[0][~inv]).all() and np.isfinite(got[1][~inv]).all()
                if name == "behind":
                    assert not want[2].any() and np.array_equal(bits(got[0]), bits(cur[0]))
                elif w >= 67:
                    frac = want[2].sum() / (~inv).sum()
                    assert (frac > 0.9) if name == "identity" else (0.7 < frac < 0.995), (tag, frac)
                    assert not np.array_equal(got[0][want[2]], cur[0][want[2]])


def test_zero_sized_image_does_nothing(ctx):
    from pbrpathtracer_amd import ptk
    prm = ptk.temporal_defaults(1.0)
    view = ptk._view(TR.view_of(TR.orbit_camera(0.0), 4, 4))
    none = [None] * 10
    assert ctx.L.ptk_reproject_planes(ctx.h, 0, 7, C.byref(view), *none, C.byref(prm), None, None) == ptk.PTK_OK
    assert ctx.L.ptk_reproject_planes_device(ctx.h, 5, 0, C.byref(view), *none, C.byref(prm), None, None) == ptk.PTK_OK


# ---- the frame entry ----------------------------------------------------------------------------------------------------------------
def three():
    from pbrpathtracer_amd import ptk
    return (1 << ptk.FEAT_MATERIAL) | (1 << ptk.FEAT_POSITION) | (1 << ptk.FEAT_NORMAL)


def orbit(cam, degrees, centre=(0.0, 0.0, 0.0)):
    """the camera turned about the vertical axis through `centre`"""
    a = math.radians(degrees)
    R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    c = np.asarray(centre, np.float64)
    rot = lambda v: (R @ np.asarray(v, np.float64)).astype(f32)
    return dict(cam, pos=(c + R @ (np.asarray(cam["pos"], np.float64) - c)).astype(f32), dir=rot(cam["dir"]), up=rot(cam["up"]))


def setup(ctx, w=W, h=H, rank=0, world=1, depth=4):
    arrays, cam = RC.scene("s_cornell")
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(w, h, depth); ctx.set_tile(rank, world); ctx.reset()
    return arrays, cam


def extent_of(arrays):
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


def guides(ctx):
    from pbrpathtracer_amd import ptk
    return ctx.read_feature(ptk.FEAT_MATERIAL), ctx.read_feature(ptk.FEAT_POSITION), ctx.read_feature(ptk.FEAT_NORMAL)


def current_of(ctx):
    """the current frame as the context reports it: accumulator, counts and the three guide planes"""
    color, count = TR.frame_inputs(ctx.read_accum(), ctx.read_sample_counts())
    ident, pos, nrm = guides(ctx)
    return (color, count, ident, pos, nrm)


class Chain:
    """the mirror chained over the frame calls of a context"""

    def __init__(self, prm):
        self.prm, self.hist, self.view, self.found = prm, None, None, None

    def call(self, ctx, **kw):
        """ptk_temporal_frame over the guide planes as they are - with PTK_TEMPORAL_RESET while this chain has no history, whatever
        an earlier test left in the context - and its result beside the mirror's"""
        reset = self.hist is None
        ctx.temporal_frame(self.prm, reset=reset, render_features=False, **kw)
        got = ctx.read_temporal()
        return got, self.step(ctx, reset)

    def step(self, ctx, reset=False):
        cur = current_of(ctx)
        view = ctx.get_view().as_dict()
        if self.hist is None or reset:
            out, n = TR.no_history(cur); self.found = np.zeros(n.shape, bool)
        else:
            out, n, self.found = TR.reproject(self.view, cur, self.hist, self.prm, want_found=True)
        self.hist, self.view = (out, n) + cur[2:], view
        return out, n


def frame(ctx, cam, spp=4, seed=5, features=True):
    ctx.set_camera(**cam); ctx.reset(); ctx.render(0, spp, seed)
    if features:
        ctx.render_features(three(), 0, seed)


@pytest.fixture
def fresh():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def test_frame_chain_over_camera_moves(fresh):
    """(a context of its own: its first call has no history without being told so)"""
    from pbrpathtracer_amd import ptk
    ctx = fresh
    arrays, cam = setup(ctx)
    prm = ptk.temporal_defaults(extent_of(arrays))
    chain = Chain(prm)
    for k, deg in enumerate((0.0, 2.0, 5.0)):
        frame(ctx, orbit(cam, deg))
        ctx.temporal_frame(prm, render_features=False)
        got = ctx.read_temporal()
        want = chain.step(ctx)
        assert same2(got, want), (k, diff(got, want))
        valid = chain.hist[2] >= 0
        assert valid.sum() > 1000 and (~valid).any()
        if k:
            assert chain.found.sum() > 0.5 * valid.sum()
            # (4 samples a frame: 8 behind every pixel with history after the first move, up to 12 after the second)
            assert (got[1][chain.found] == 8.0).all() if k == 1 else (got[1][chain.found].max() == 12.0 and got[1][chain.found].min() >= 8.0)
    # the convenience path renders the same three planes itself
    frame(ctx, orbit(cam, 7.0), features=False)
    ctx.temporal_frame(prm, seed=5)
    got = ctx.read_temporal()
    assert same2(got, chain.step(ctx))
    # ... equal again after an adaptive render, with per-pixel counts
    ctx.set_camera(**orbit(cam, 9.0))
    res = ctx.render_adaptive(0.05, 8, 4, 32, 5)
    n = ctx.read_sample_counts()
    assert res["rounds"] >= 2 and len(np.unique(n)) >= 2, "every pixel holds the same count: a poor test"
    ctx.temporal_frame(prm, seed=5)
    got = ctx.read_temporal()
    want = chain.step(ctx)
    assert same2(got, want), diff(got, want)
    assert chain.found.sum() > 1000 and len(np.unique(got[1][chain.found])) >= 2
    # either pointer of ptk_read_temporal may be null
    only = np.empty((H, W), f32)
    assert ctx.L.ptk_read_temporal(ctx.h, None, only.ctypes.data) == ptk.PTK_OK and same(only, want[1])
    assert ctx.L.ptk_read_temporal(ctx.h, None, None) == ptk.PTK_OK


def test_frame_tile_split(ctx):
    from pbrpathtracer_amd import ptk
    arrays, cam = setup(ctx)
    prm = ptk.temporal_defaults(extent_of(arrays))
    chain = Chain(prm)
    frame(ctx, cam)
    got, want = chain.call(ctx)
    assert same2(got, want)
    owned = np.ascontiguousarray(FT.owned_mask(W, H, 0, 2)[::-1])
    assert 0.3 < owned.mean() < 0.7
    try:
        # guide planes of the whole frame, samples on this rank's tiles only: the other pixels have nc = 0 and take the history
        ctx.set_camera(**orbit(cam, 2.0)); ctx.render_features(three(), 0, 5)
        ctx.set_tile(0, 2); ctx.reset(); ctx.render(0, 4, 5)
        ctx.temporal_frame(prm, render_features=False)
        got = ctx.read_temporal()
        assert np.array_equal(ctx.read_sample_counts() > 0, owned)
        want = chain.step(ctx)
        assert same2(got, want), diff(got, want)
        took = chain.found & ~owned
        assert took.sum() > 500 and (got[1][took] == 4.0).all() and (got[0][took] != 0).any()
        assert (got[1][chain.found & owned] == 8.0).all()
        # guide planes of the split frame: the pixels of the other rank are invalid and pass through as 0
        frame(ctx, orbit(cam, 4.0))
        ctx.temporal_frame(prm, render_features=False)
        got = ctx.read_temporal()
        want = chain.step(ctx)
        assert same2(got, want), diff(got, want)
        assert (chain.hist[2][~owned] < 0).all() and (got[0][~owned] == 0).all() and (got[1][~owned] == 0).all()
        assert (chain.found & owned).sum() > 500
    finally:
        ctx.set_tile(0, 1)


def test_reset_and_a_resolution_change_drop_the_history(ctx):
    from pbrpathtracer_amd import ptk
    arrays, cam = setup(ctx)
    prm = ptk.temporal_defaults(extent_of(arrays))
    chain = Chain(prm)
    for deg in (0.0, 1.0):
        frame(ctx, orbit(cam, deg))
        got, want = chain.call(ctx)
        assert same2(got, want)
    cur = current_of(ctx)
    assert not np.array_equal(got[0], cur[0])
    ctx.temporal_frame(prm, reset=True, render_features=False)
    got = ctx.read_temporal()
    assert same2(got, chain.step(ctx, reset=True)) and same2(got, cur[:2])
    # ... and the call after it has that frame for its history
    frame(ctx, orbit(cam, 2.0))
    ctx.temporal_frame(prm, render_features=False)
    got = ctx.read_temporal()
    assert same2(got, chain.step(ctx)) and (got[1][chain.found] == 8.0).all() and chain.found.any()
    # another resolution: no result to read, and the next call starts over
    ctx.set_frame(48, 32, 4)
    buf = np.full((32, 48, 3), 7.25, f32)
    assert ctx.L.ptk_read_temporal(ctx.h, buf.ctypes.data, None) == BAD_ARG and (buf == 7.25).all()
    a = C.c_void_p(); b = C.c_void_p(); n = C.c_size_t()
    assert ctx.L.ptk_temporal_device_ptr(ctx.h, C.byref(a), C.byref(b), C.byref(n)) == BAD_ARG
    assert ctx.L.ptk_temporal_frame(ctx.h, C.byref(prm), 0) == BAD_ARG            # (no feature planes at this resolution yet)
    frame(ctx, orbit(cam, 2.0))
    ctx.temporal_frame(prm, render_features=False)
    got = ctx.read_temporal()
    assert got[0].shape == (32, 48, 3) and same2(got, current_of(ctx)[:2])
    # back at the first resolution the old history is gone too
    ctx.set_frame(W, H, 4)
    frame(ctx, orbit(cam, 2.0))
    ctx.temporal_frame(prm, render_features=False)
    assert same2(ctx.read_temporal(), current_of(ctx)[:2])


def test_device_planes_chain_into_the_denoiser(ctx):
    import torch
    from pbrpathtracer_amd import ptk
    arrays, cam = setup(ctx)
    prm = ptk.temporal_defaults(extent_of(arrays))
    dprm = ptk.denoise_defaults(extent_of(arrays))
    feats = three() | (1 << ptk.FEAT_TRIANGLE) | (1 << ptk.FEAT_ALBEDO)
    chain = Chain(prm)
    for deg in (0.0, 2.0):
        ctx.set_camera(**orbit(cam, deg)); ctx.reset(); ctx.render(0, 4, 5); ctx.render_features(feats, 0, 5)
        got, want = chain.call(ctx)
        assert same2(got, want)
    color, count, px = ctx.temporal_device_ptr()
    assert color and count and px == W * H
    out = torch.empty((H, W, 3), dtype=torch.float32, device=torch.device("cuda", ctx.device_ordinal()))
    torch.cuda.synchronize()
    fp = lambda k: C.c_void_p(ctx.feature_device_ptr(k)[0])
    rc = ctx.L.ptk_denoise_planes_device(ctx.h, W, H, C.c_void_p(color), fp(ptk.FEAT_TRIANGLE), fp(ptk.FEAT_NORMAL), fp(ptk.FEAT_POSITION),
                                         fp(ptk.FEAT_ALBEDO), None, C.byref(dprm), C.c_void_p(out.data_ptr()), None)
    assert rc == ptk.PTK_OK
    ctx.synchronize()
    tri, albedo = ctx.read_feature(ptk.FEAT_TRIANGLE), ctx.read_feature(ptk.FEAT_ALBEDO)
    den, _ = DR.denoise(want[0], tri, chain.hist[4], chain.hist[3], albedo, None, dprm)
    assert same(out.cpu().numpy(), den)
    assert not np.array_equal(den, want[0])


def test_frame_state_is_left_alone(ctx):
    from pbrpathtracer_amd import ptk
    arrays, cam = setup(ctx)
    prm = ptk.temporal_defaults(extent_of(arrays))
    five = (1 << ptk.FEAT_TRIANGLE) | (1 << ptk.FEAT_POSITION) | (1 << ptk.FEAT_NORMAL) | (1 << ptk.FEAT_ALBEDO) | (1 << ptk.FEAT_EMISSION)
    mask = five | (1 << ptk.FEAT_MATERIAL)

    def state(adaptive):
        s = dict(accum=ctx.read_accum(), rgb8=ctx.resolve_rgb8(), samples=np.array(ctx.samples()), denoised=ctx.read_denoised())
        s.update({nm: ctx.read_feature(k) for k, nm in enumerate(ptk.FEAT_NAMES) if (mask >> k) & 1})
        if adaptive:
            s.update(counts=ctx.read_sample_counts(), moments=ctx.read_moments())
        return s

    ctx.render(0, 8, 5)
    ctx.render_features(mask, 0, 5)
    ctx.denoise_frame(ptk.denoise_defaults(extent_of(arrays)), render_features=False)
    before = state(False)
    for _ in range(2):
        ctx.temporal_frame(prm, render_features=False)
        ctx.read_temporal()
    after = state(False)
    for k in before:
        assert same(before[k], after[k]), k
    ctx.render(8, 4, 5)
    twelve = ctx.read_accum()
    ctx.reset(); ctx.render(0, 12, 5)
    assert ctx.samples() == 12 and same(twelve, ctx.read_accum())
    ctx.render_adaptive(0.05, 8, 4, 24, 5)
    ctx.render_features(mask, 0, 5)
    ctx.denoise_frame(ptk.denoise_defaults(extent_of(arrays)), render_features=False)
    before = state(True)
    ctx.temporal_frame(prm, render_features=False)
    ctx.read_temporal()
    after = state(True)
    for k in before:
        assert same(before[k], after[k]), k


# ---- the view -------------------------------------------------------------------------------------------------------------------------
def view_equal(got, want):
    got = got.as_dict()
    return all(np.array_equal(bits(np.asarray(got[k], f32)), bits(np.asarray(want[k], f32))) for k in want)


def test_get_view_equals_the_mirror(ctx):
    arrays, cam = setup(ctx)
    cams = [orbit(cam, d) for d in (0.0, 1.0, 2.0, 5.0, 33.0, 180.0)] + [TR.orbit_camera(d) for d in (10.0, 13.0)]
    cams.append(dict(cam, focal=-1.0, fovy=0.0)); cams.append(dict(cam, fovy=200.0))          # the setter's clamps
    for w, h in ((W, H), (130, 70)):
        ctx.set_frame(w, h, 4)
        for k, cm in enumerate(cams):
            ctx.set_camera(**cm)
            # (a pending set_camera: nothing has rendered with it yet)
            assert view_equal(ctx.get_view(), TR.view_of(cm, w, h)), (w, h, k)
        ctx.render(0, 1, 5)
        assert view_equal(ctx.get_view(), TR.view_of(cams[-1], w, h))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
BAD_PARAMS = [dict(max_plane_dist=v) for v in (0.0, -1.0, float("nan"), float("inf"))] + \
    [dict(min_normal_dot=v) for v in (-1.5, 1.5, float("nan"), float("inf"))] + \
    [dict(max_history=v) for v in (0.5, 0.0, -1.0, float("nan"), float("inf"))]


def test_refusals(ctx):
    import torch
    from pbrpathtracer_amd import ptk
    L = ctx.L
    w, h = 9, 7
    case = TR.random_case(w, h, 3)
    planes = [np.ascontiguousarray(a) for a in case["current"] + case["history"]]
    out = np.full((h, w, 3), 7.25, f32); out_n = np.full((h, w), 7.25, f32)
    view = ptk._view(case["hist_view"])
    ptr = lambda a: None if a is None else a.ctypes.data
    good = TR.params(0.05)

    def planes_call(prm, ww=w, hh=h, drop=None, v=True, p=True, o=(out, out_n), c=ctx.h):
        a = [None if k == drop else ptr(x) for k, x in enumerate(planes)]
        return L.ptk_reproject_planes(c, ww, hh, C.byref(view) if v else None, *a, C.byref(prm) if p else None, ptr(o[0]), ptr(o[1]))

    # the frame entry's history, which refused calls must leave as it is
    arrays, cam = setup(ctx, 48, 32)
    fprm = ptk.temporal_defaults(extent_of(arrays))
    chain = Chain(fprm)
    frame(ctx, cam)
    kept, want = chain.call(ctx)
    assert same2(kept, want)
    for bad in BAD_PARAMS:
        prm = ptk._temporal_params(dict(good, **bad))
        assert planes_call(prm) == BAD_ARG, bad
        assert L.ptk_temporal_frame(ctx.h, C.byref(prm), 0) == BAD_ARG, bad
    prm = ptk._temporal_params(good)
    assert planes_call(prm, ww=-1) == BAD_ARG and planes_call(prm, hh=-1) == BAD_ARG
    assert planes_call(prm, v=False) == BAD_ARG and planes_call(prm, p=False) == BAD_ARG and planes_call(prm, c=None) == BAD_ARG
    for k in range(10):
        assert planes_call(prm, drop=k) == BAD_ARG, k
    assert planes_call(prm, o=(None, out_n)) == BAD_ARG and planes_call(prm, o=(out, None)) == BAD_ARG
    assert (out == 7.25).all() and (out_n == 7.25).all()
    # the device entry refuses alike
    dev = torch.device("cuda", ctx.device_ordinal())
    d_out = torch.full((h, w, 3), 7.25, device=dev); d_n = torch.full((h, w), 7.25, device=dev)
    t = [torch.from_numpy(a).to(dev) for a in planes]
    dp = lambda x: C.c_void_p(x.data_ptr())
    bad = ptk._temporal_params(dict(good, max_history=0.0))
    assert L.ptk_reproject_planes_device(ctx.h, w, h, C.byref(view), *map(dp, t), C.byref(bad), dp(d_out), dp(d_n)) == BAD_ARG
    assert L.ptk_reproject_planes_device(ctx.h, w, h, None, *map(dp, t), C.byref(prm), dp(d_out), dp(d_n)) == BAD_ARG
    assert L.ptk_reproject_planes_device(ctx.h, w, h, C.byref(view), None, *map(dp, t[1:]), C.byref(prm), dp(d_out), dp(d_n)) == BAD_ARG
    assert L.ptk_reproject_planes_device(ctx.h, w, h, C.byref(view), *map(dp, t), C.byref(prm), None, dp(d_n)) == BAD_ARG
    ctx.synchronize()
    assert (d_out == 7.25).all().item() and (d_n == 7.25).all().item()
    # frame entry: unknown flag bits, null params, null context
    assert L.ptk_temporal_frame(ctx.h, C.byref(fprm), 2) == BAD_ARG
    assert L.ptk_temporal_frame(ctx.h, C.byref(fprm), 0x80000001) == BAD_ARG
    assert L.ptk_temporal_frame(ctx.h, None, 0) == BAD_ARG and L.ptk_temporal_frame(None, C.byref(fprm), 0) == BAD_ARG
    assert L.ptk_get_view(ctx.h, None) == BAD_ARG and L.ptk_get_view(None, C.byref(view)) == BAD_ARG
    assert L.ptk_read_temporal(None, None, None) == BAD_ARG and L.ptk_temporal_device_ptr(None, None, None, None) == BAD_ARG
    # a missing guide plane
    for k in (ptk.FEAT_MATERIAL, ptk.FEAT_POSITION, ptk.FEAT_NORMAL):
        ctx.render_features(three() & ~(1 << k), 0, 5)
        assert L.ptk_temporal_frame(ctx.h, C.byref(fprm), 0) == BAD_ARG, k
    assert same2(ctx.read_temporal(), kept)
    # ... and the history is as it was: the next good call blends with it
    frame(ctx, orbit(cam, 2.0))
    assert L.ptk_temporal_frame(ctx.h, C.byref(fprm), 0) == ptk.PTK_OK
    got = ctx.read_temporal()
    assert same2(got, chain.step(ctx)) and chain.found.sum() > 300
    # a context without a frame, and one that never reprojected
    c2 = ptk.Context(0)
    try:
        assert c2.L.ptk_get_view(c2.h, C.byref(view)) == BAD_ARG
        assert c2.L.ptk_temporal_frame(c2.h, C.byref(fprm), 0) == BAD_ARG
        c2.upload_scene(arrays); c2.set_camera(**cam); c2.set_frame(48, 32, 4)
        buf = np.full((32, 48, 3), 7.25, f32)
        assert c2.L.ptk_read_temporal(c2.h, buf.ctypes.data, None) == BAD_ARG and (buf == 7.25).all()
        assert c2.L.ptk_temporal_frame(c2.h, C.byref(fprm), 0) == BAD_ARG          # no feature planes
        # the planes entry needs no scene, no camera and no frame
        c3 = ptk.Context(0)
        got = c3.reproject_planes(case["hist_view"], case["current"], case["history"], good)
        c3.close()
        assert same2(got, TR.reproject(case["hist_view"], case["current"], case["history"], good))
    finally:
        c2.close()


# ---- the host class -------------------------------------------------------------------------------------------------------------------
def test_host_class(tmp_path):
    """PathTracer.TemporalFrame renders the guide planes itself and equals the context's rule; ReadTemporal, GetView"""
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer, camera_from_scene
    pts, scene, _ = S.build_config("C1", str(tmp_path), width=64, height=48, depth=4)
    pt = PathTracer(device=0)
    pt.LoadSceneFile(pts)
    pt.SetSeed(3)
    c = pt.context()
    prm = ptk.temporal_defaults(extent_of(pt.StagedScene()))
    chain = Chain(prm)
    cam = camera_from_scene(scene)
    for k, deg in enumerate((0.0, 2.0, 4.0)):
        cm = orbit(cam, deg)
        pt.SetCamera(cm["pos"], cm["dir"], cm["up"])
        pt.ResetImage()
        pt.RenderFrames(4)
        pt.TemporalFrame()
        got = pt.ReadTemporal()
        assert view_equal(pt.GetView(), c.get_view().as_dict())
        want = chain.step(c)
        assert same2(got, want), (k, diff(got, want))
        assert pt.GetSamples() == 4
    assert chain.found.sum() > 500 and got[1][chain.found].max() == 12.0 and got[1][chain.found].min() >= 8.0
    pt.TemporalFrame(reset=True)
    assert same2(pt.ReadTemporal(), chain.step(c, reset=True))
    # DenoiseFrame() behind it shares the guide planes TemporalFrame() rendered
    pt.DenoiseFrame()
    assert np.isfinite(pt.ReadDenoised()).all()
    pt.TemporalFrame()
    assert same2(pt.ReadTemporal(), chain.step(c))


# ---- the feature does its job ---------------------------------------------------------------------------------------------------------
def test_an_orbit_is_less_noisy_with_history(ctx):
    """An 8-step orbit of 1 degree per step at 4 spp: against a 4096-spp render of the last view the reprojected frame has a lower
    RMSE over the valid pixels than the plain 4-spp last frame - more samples of view-independent radiance, not a tuned number."""
    from pbrpathtracer_amd import ptk
    arrays, cam = setup(ctx)
    prm = ptk.temporal_defaults(extent_of(arrays))
    chain = Chain(prm)
    for k in range(8):
        frame(ctx, orbit(cam, float(k + 1)), seed=100 + k)
        (got, n), want = chain.call(ctx)
        assert same2((got, n), want)
    plain = current_of(ctx)[0]
    valid = chain.hist[2] >= 0
    ctx.reset(); ctx.render(0, 4096, 999)
    truth = (ctx.read_accum() / f32(4096)).astype(f32)
    rmse = lambda a: float(np.sqrt(np.mean((a[valid].astype(np.float64) - truth[valid]) ** 2)))
    found = chain.found.sum() / valid.sum()
    print("orbit: RMSE plain %.5f, temporal %.5f, ratio %.3f; found history %.3f; mean count %.1f"
          % (rmse(plain), rmse(got), rmse(got) / rmse(plain), found, n[valid].mean()))
    assert found >= 0.5
    assert rmse(got) < rmse(plain)
