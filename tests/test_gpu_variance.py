"""Temporal luminance moments, the variance made of them and the denoiser behind them (include/ptk.h ptk_reproject_moments,
ptk_temporal_frame_moments, ptk_variance_planes, ptk_temporal_variance, ptk_denoise_temporal) on the GPU: every output array_equal -
dtype and shape included - to tests/variance_rule.py, the numpy float32 restatement of the header's rule.  The planes entries over
sizes that split blocks and push taps over every edge; the frame entry chained over camera and object moves beside a context that
runs the plain entries; the history rules between the three frame entries; the variance and the denoiser over the context's own
planes; what the calls must not touch; refusals; the host class and the command line."""
import ctypes as C
import os

import numpy as np
import pytest

import feature_truth as FT
import motion_cases as MC
import motion_rule as MR
import ray_cases as RC
import temporal_rule as TR
import variance_rule as VR

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD_ARG, LIMIT = -1, -4            # PTK_ERR_BAD_ARG, PTK_ERR_LIMIT
W, H = 64, 48
SEED = 5
SIZES = [(1, 1), (5, 3), (67, 35), (130, 70)]


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


@pytest.fixture
def fresh():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def same(got, want):
    """array_equal with dtype and shape; NaN == NaN (an invalid pixel may hold one and keeps its bits)"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def same_all(got, want):
    return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def where_differ(got, want):
    return [np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:3].tolist() for g, w in zip(got, want)]


def on_device(ctx, planes):
    import torch
    dev = torch.device("cuda", ctx.device_ordinal())
    t = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in planes]
    torch.cuda.synchronize()
    return t


def host(tensors):
    return [t.cpu().numpy() for t in tensors]


# ---- the planes entries: moments through the reprojection -----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_reproject_moments_equals_the_mirror(ctx, w, h):
    case = VR.moments_case(w, h, seed=w + h)
    cur, hist, hm, view = case["current"], case["history"], case["hist_moments"], case["hist_view"]
    prev = MC.primed_planes(cur, seed=w, extent=case["extent"])
    inv = cur[2] < 0
    tcur, thist, tprev = on_device(ctx, cur), on_device(ctx, hist + (hm,)), on_device(ctx, prev)
    talbedo, = on_device(ctx, [case["albedo"]])
    for moving in (False, True):
        for albedo in (False, True):
            for match, max_history in ((1, 64.0), (0, 1.0)):
                p = TR.params(case["extent"] / 100.0, 0.9, max_history, match)
                A = case["albedo"] if albedo else None
                pv = prev if moving else None
                want = VR.reproject_moments(view, cur, hist, hm, p, albedo=A, prev=pv, want_found=True)
                got = ctx.reproject_moments(view, cur, hist + (hm,), p, albedo=A, prev=pv)
                dgot = ctx.reproject_moments(view, tcur, thist, p, albedo=talbedo if albedo else None, prev=tprev if moving else None)
                ctx.synchronize()
                tag = (w, h, moving, albedo, match)
                assert same_all(got, want[:3]), (tag, where_differ(got, want))
                assert same_all(host(dgot), want[:3]), tag
                # colour and count: the bits of the entries without moments, invalid pixels included
                plain = ctx.reproject_planes_moving(view, cur, prev[0], prev[1], hist, p) if moving else ctx.reproject_planes(view, cur, hist, p)
                assert np.array_equal(bits(got[0]), bits(plain[0])) and np.array_equal(bits(got[1]), bits(plain[1])), tag
                assert (got[2][inv] == 0).all() and np.isfinite(got[2][~inv]).all(), tag
                if w >= 67:
                    found = want[3]
                    assert found.sum() > 0.5 * (~inv).sum() and ((~inv) & ~found).sum() > 20, tag
                    assert not np.array_equal(got[2][found], VR.no_history(cur, A)[2][found])


# ---- the planes entries: variance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_variance_planes_equal_the_mirror(ctx, w, h):
    planes = VR.variance_case(w, h, seed=w * h)
    mom, n, f, ident, pos, nrm = planes
    tplanes = on_device(ctx, planes)
    if w >= 67:
        valid = ident >= 0
        assert (valid & (n == 0)).sum() > 20 and (valid & (f == 0) & (n > 0)).sum() > 20 and (valid & np.isnan(mom[..., 0])).sum() > 20
    for radius in (1, 2, 3):
        for prefilter in (0, 1):
            vp = VR.params(TR.EXTENT, radius=radius, prefilter=prefilter)
            raw, (none, temporal, spatial) = VR.raw_variance(*planes, vp, want_branch=True)
            if w >= 67:
                assert temporal.sum() >= 100 and spatial.sum() >= 100 and none.sum() >= 100
            want = VR.variance(*planes, vp)
            got = ctx.variance_planes(*planes, vp)
            dgot = ctx.variance_planes(*tplanes, vp)
            ctx.synchronize()
            tag = (w, h, radius, prefilter)
            assert same(got, want), (tag, where_differ([got], [want]))
            assert same(dgot.cpu().numpy(), want), tag
            assert (got[none] == 0).all(), tag
            t = ctx.last_variance_ms()
            assert t["variance_ms"] > 0 and (t["prefilter_ms"] > 0) == bool(prefilter)


def test_zero_sized_images_do_nothing(ctx):
    from pbrpathtracer_amd import ptk
    prm = ptk.temporal_defaults(1.0); vp = ptk.variance_defaults(1.0)
    view = ptk._view(TR.view_of(TR.orbit_camera(0.0), 4, 4))
    for w, h in ((0, 7), (5, 0)):
        desc = ptk.ReprojectDesc(w, h, C.pointer(view))
        assert ctx.L.ptk_reproject_moments(ctx.h, C.byref(desc), C.byref(prm)) == ptk.PTK_OK
        assert ctx.L.ptk_reproject_moments_device(ctx.h, C.byref(desc), C.byref(prm)) == ptk.PTK_OK
        assert ctx.L.ptk_variance_planes(ctx.h, w, h, *[None] * 6, C.byref(vp), None) == ptk.PTK_OK
        assert ctx.L.ptk_variance_planes_device(ctx.h, w, h, *[None] * 6, C.byref(vp), None) == ptk.PTK_OK


# ---- the frame entry ------------------------------------------------------------------------------------------------------------------
def feature_mask(moving=False, denoise=True):
    from pbrpathtracer_amd import ptk
    m = (1 << ptk.FEAT_MATERIAL) | (1 << ptk.FEAT_POSITION) | (1 << ptk.FEAT_NORMAL) | (1 << ptk.FEAT_ALBEDO)
    if moving:
        m |= (1 << ptk.FEAT_TRIANGLE) | (1 << ptk.FEAT_BARY)
    if denoise:
        m |= (1 << ptk.FEAT_TRIANGLE) | (1 << ptk.FEAT_EMISSION)
    return m


def stage(ctx, arrays, cam, w=W, h=H, depth=4):
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(w, h, depth); ctx.set_tile(0, 1); ctx.reset()


def extent_of(arrays):
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


def frame(ctx, cam, spp=2, seed=SEED, mask=None):
    ctx.set_camera(**cam); ctx.reset(); ctx.render(0, spp, seed)
    ctx.render_features(feature_mask(True) if mask is None else mask, 0, seed)


def current_of(ctx):
    """the current frame as the context reports it: accumulator, counts, the three guide planes - and the albedo"""
    from pbrpathtracer_amd import ptk
    color, count = TR.frame_inputs(ctx.read_accum(), ctx.read_sample_counts())
    cur = (color, count, ctx.read_feature(ptk.FEAT_MATERIAL), ctx.read_feature(ptk.FEAT_POSITION), ctx.read_feature(ptk.FEAT_NORMAL))
    return cur, ctx.read_feature(ptk.FEAT_ALBEDO)


def got_of(ctx):
    return ctx.read_temporal() + (ctx.read_temporal_variance(variance=False)[0],)


class Chain:
    """the mirror chained over the frame calls of a context: moments calls, and the plain calls between them"""

    def __init__(self, prm):
        self.prm, self.hist, self.mom, self.view, self.found, self.frame_count = prm, None, None, None, None, None

    def step(self, ctx, moments=True, reset=False, tables=None):
        """The mirror's (colour, count, moments) - (colour, count) for a plain call - for the context's current frame.  tables:
        (current, previous or None) vertex tables, the MOVING rule."""
        from pbrpathtracer_amd import ptk
        cur, albedo = current_of(ctx)
        view = ctx.get_view().as_dict()
        use = self.hist is not None and not reset and (not moments or self.mom is not None)
        prev = None
        if tables is not None:
            four = tuple(ctx.read_feature(k) for k in (ptk.FEAT_TRIANGLE, ptk.FEAT_BARY, ptk.FEAT_POSITION, ptk.FEAT_NORMAL))
            prev = MR.render_motion(self.view if use else None, four, tables[0], tables[1])[:2]
        if not use:
            out, n, mom = VR.no_history(cur, albedo); self.found = np.zeros(n.shape, bool)
        else:
            hm = self.mom if self.mom is not None else np.zeros(cur[1].shape + (2,), f32)
            out, n, mom, self.found = VR.reproject_moments(self.view, cur, self.hist, hm, self.prm, albedo=albedo, prev=prev, want_found=True)
        self.hist, self.view, self.mom, self.frame_count = (out, n) + cur[2:], view, (mom if moments else None), cur[1]
        return (out, n, mom) if moments else (out, n)

    def variance(self, vp):
        return VR.variance(self.mom, self.hist[1], self.frame_count, self.hist[2], self.hist[3], self.hist[4], vp)


def test_frame_chain_over_camera_moves(fresh):
    """C1 at 64 x 48, four orbit steps of two samples: the moments entry equals the mirror chain, its colour and count equal a
    second context's ptk_temporal_frame, and the variance of the context's planes equals ptk_variance_planes_device over them and
    the mirror.  (Contexts of their own: a first call has no history without being told so.)"""
    from pbrpathtracer_amd import ptk
    ctx = fresh
    arrays, cam = RC.scene("s_cornell")
    stage(ctx, arrays, cam)
    other = ptk.Context(0)
    try:
        stage(other, arrays, cam)
        prm = ptk.temporal_defaults(extent_of(arrays)); vp = ptk.variance_defaults(extent_of(arrays))
        chain = Chain(prm)
        for k, deg in enumerate((0.0, 2.0, 4.0, 5.0)):
            for c in (ctx, other):
                frame(c, MC.orbit(cam, deg))
            ctx.temporal_frame(prm, render_features=False, moments=True)
            other.temporal_frame(prm, render_features=False)
            got = got_of(ctx)
            want = chain.step(ctx)
            assert same_all(got, want), (k, where_differ(got, want))
            assert same_all(got[:2], other.read_temporal()), k
            valid = chain.hist[2] >= 0
            assert valid.sum() > 500 and (~valid).any() and (got[2][~valid] == 0).all()
            if k:
                assert chain.found.sum() > 0.5 * valid.sum()
            # the variance: the frame entry, the mirror, and the planes entry over the context's own planes
            for v in (vp, ptk.VarianceParams(1, 0, 2.0, vp.max_plane_dist, vp.min_normal_dot)):
                ctx.temporal_variance(v)
                mom, var = ctx.read_temporal_variance()
                want_var = chain.variance(v)
                assert same(mom, want[2]) and same(var, want_var), (k, where_differ([var], [want_var]))
                planes = on_device(ctx, (want[2], want[1], chain.frame_count) + chain.hist[2:])
                dvar = ctx.variance_planes(*planes, v)
                ctx.synchronize()
                assert same(dvar.cpu().numpy(), var), k
            raw, (none, temporal, spatial) = VR.raw_variance(chain.mom, chain.hist[1], chain.frame_count, *chain.hist[2:], vp, want_branch=True)
            assert spatial.sum() > 500 if k < 3 else (temporal.sum() > 200 and spatial.sum() > 20), k
            assert var[valid].max() > 0
        # the device pointers are those planes
        a, b, px = ctx.temporal_variance_device_ptr()
        assert a and b and px == W * H and ctx.temporal_variance_device_ptr(variance=False)[1] is None
        assert a != b
        # the convenience path renders the planes itself
        ctx.set_camera(**MC.orbit(cam, 7.0)); ctx.reset(); ctx.render(0, 2, SEED)
        ctx.temporal_frame(prm, seed=SEED, moments=True)
        assert same_all(got_of(ctx), chain.step(ctx))
        # ... equal again after an adaptive render, with per-pixel counts
        ctx.set_camera(**MC.orbit(cam, 8.0))
        ctx.render_adaptive(0.05, 4, 4, 16, SEED)
        assert len(np.unique(ctx.read_sample_counts())) >= 2
        ctx.temporal_frame(prm, seed=SEED, moments=True)
        got = got_of(ctx)
        want = chain.step(ctx)
        assert same_all(got, want), where_differ(got, want)
        ctx.temporal_variance(vp)
        assert same(ctx.read_temporal_variance()[1], chain.variance(vp))
    finally:
        other.close()


def card_table(k):
    arrays, first, n = MC.quality_scene()
    t = np.ascontiguousarray(arrays["verts"], f32).reshape(-1, 9).copy()
    t[first:first + n] = MC.card_verts(k)
    return t


def test_frame_chain_over_a_moved_card(fresh):
    from pbrpathtracer_amd import ptk
    ctx = fresh
    arrays, first, ncard = MC.quality_scene()
    cam = MC.QUALITY_CAM
    stage(ctx, arrays, cam)
    other = ptk.Context(0)
    try:
        stage(other, arrays, cam)
        prm = ptk.temporal_defaults(MC.EXTENT); vp = ptk.variance_defaults(MC.EXTENT)
        chain = Chain(prm)
        for k, deg in enumerate((0.0, 1.0, 2.0, 3.0)):
            for c in (ctx, other):
                if k:
                    c.snapshot_geometry(); c.update_geometry(first, MC.card_verts(k))
                frame(c, MC.orbit(cam, deg))
            ctx.temporal_frame(prm, render_features=False, moving=True, moments=True)
            other.temporal_frame(prm, render_features=False, moving=True)
            got = got_of(ctx)
            want = chain.step(ctx, tables=(card_table(k), card_table(k - 1) if k else None))
            assert same_all(got, want), (k, where_differ(got, want))
            assert same_all(got[:2], other.read_temporal()), k
            assert same_all(ctx.read_motion(), other.read_motion()), k
            tri = ctx.read_feature(ptk.FEAT_TRIANGLE)
            card = (tri >= first) & (tri < first + ncard)
            assert card.sum() > 100
            if k:
                assert chain.found[card].mean() > 0.5 and (got[1][chain.found & card] >= 4.0).all()
        ctx.temporal_variance(vp)
        assert same(ctx.read_temporal_variance()[1], chain.variance(vp))
    finally:
        other.close()


def test_frame_tile_split(ctx):
    """rank 0 of 2: the pixels this rank does not own have n_p = 0, take the history's moments as they are and a frame count of 0"""
    from pbrpathtracer_amd import ptk
    arrays, cam = RC.scene("s_cornell")
    stage(ctx, arrays, cam)
    prm = ptk.temporal_defaults(extent_of(arrays)); vp = ptk.variance_defaults(extent_of(arrays))
    chain = Chain(prm)
    frame(ctx, cam)
    ctx.temporal_frame(prm, reset=True, render_features=False, moments=True)
    assert same_all(got_of(ctx), chain.step(ctx, reset=True))
    owned = np.ascontiguousarray(FT.owned_mask(W, H, 0, 2)[::-1])
    try:
        ctx.set_camera(**MC.orbit(cam, 2.0)); ctx.render_features(feature_mask(), 0, SEED)
        ctx.set_tile(0, 2); ctx.reset(); ctx.render(0, 2, SEED)
        ctx.temporal_frame(prm, render_features=False, moments=True)
        got = got_of(ctx)
        assert np.array_equal(ctx.read_sample_counts() > 0, owned)
        want = chain.step(ctx)
        assert same_all(got, want), where_differ(got, want)
        took = chain.found & ~owned
        assert took.sum() > 100 and (got[1][took] == 2.0).all() and (got[2][took] != 0).any()
        ctx.temporal_variance(vp)
        assert same(ctx.read_temporal_variance()[1], chain.variance(vp))
    finally:
        ctx.set_tile(0, 1)


def test_history_rules_between_the_frame_entries(ctx):
    from pbrpathtracer_amd import ptk
    arrays, cam = RC.scene("s_cornell")
    stage(ctx, arrays, cam)
    prm = ptk.temporal_defaults(extent_of(arrays)); vp = ptk.variance_defaults(extent_of(arrays))
    chain = Chain(prm)
    frame(ctx, cam)
    ctx.temporal_frame(prm, reset=True, render_features=False, moments=True)
    assert same_all(got_of(ctx), chain.step(ctx, reset=True))
    frame(ctx, MC.orbit(cam, 1.0))
    ctx.temporal_frame(prm, render_features=False, moments=True)
    got = got_of(ctx)
    assert same_all(got, chain.step(ctx)) and chain.found.sum() > 300 and (got[1][chain.found] == 4.0).all()
    # RESET: the frame's own bits
    ctx.temporal_frame(prm, reset=True, render_features=False, moments=True)
    got = got_of(ctx)
    cur, albedo = current_of(ctx)
    assert same_all(got, chain.step(ctx, reset=True)) and same_all(got, VR.no_history(cur, albedo))
    # a plain entry behind a moments call continues the colour history with the bits it would have had, and invalidates the moments
    frame(ctx, MC.orbit(cam, 2.0))
    ctx.temporal_frame(prm, render_features=False)
    got = ctx.read_temporal()
    want = chain.step(ctx, moments=False)
    assert same_all(got, want) and chain.found.sum() > 300 and (got[1][chain.found] == 4.0).all()
    buf = np.full((H, W, 2), 7.25, f32)
    assert ctx.L.ptk_read_temporal_variance(ctx.h, buf.ctypes.data, None) == BAD_ARG and (buf == 7.25).all()
    assert ctx.L.ptk_temporal_variance(ctx.h, C.byref(vp)) == BAD_ARG
    assert ctx.L.ptk_temporal_variance_device_ptr(ctx.h, None, None, None) == BAD_ARG
    # ... and the next moments call starts over, colour included
    frame(ctx, MC.orbit(cam, 3.0))
    ctx.temporal_frame(prm, render_features=False, moments=True)
    got = got_of(ctx)
    cur, albedo = current_of(ctx)
    assert same_all(got, chain.step(ctx)) and same_all(got, VR.no_history(cur, albedo)) and not chain.found.any()
    # the one after it has that frame for its history; moving and static calls share it
    frame(ctx, MC.orbit(cam, 4.0))
    ctx.temporal_frame(prm, render_features=False, moments=True, moving=True)
    got = got_of(ctx)
    table = np.ascontiguousarray(arrays["verts"], f32).reshape(-1, 9)
    assert same_all(got, chain.step(ctx, tables=(table, None))) and chain.found.sum() > 300
    # the variance is asked for behind the moments call it belongs to
    var = np.full((H, W), 7.25, f32)
    assert ctx.L.ptk_read_temporal_variance(ctx.h, None, var.ctypes.data) == BAD_ARG and (var == 7.25).all()
    dprm = ptk.denoise_defaults(extent_of(arrays), variance=True)
    assert ctx.L.ptk_denoise_temporal(ctx.h, C.byref(dprm), ptk.DENOISE_VARIANCE) == BAD_ARG
    ctx.temporal_variance(vp)
    assert same(ctx.read_temporal_variance()[1], chain.variance(vp))
    # another resolution: nothing to read, and the next call starts over
    ctx.set_frame(48, 32, 4)
    buf = np.full((32, 48, 2), 7.25, f32)
    assert ctx.L.ptk_read_temporal_variance(ctx.h, buf.ctypes.data, None) == BAD_ARG and (buf == 7.25).all()
    assert ctx.L.ptk_temporal_variance(ctx.h, C.byref(vp)) == BAD_ARG
    assert ctx.L.ptk_temporal_frame_moments(ctx.h, C.byref(prm), 0) == BAD_ARG          # (no feature planes at this resolution yet)
    frame(ctx, MC.orbit(cam, 4.0))
    ctx.temporal_frame(prm, render_features=False, moments=True)
    got = got_of(ctx)
    cur, albedo = current_of(ctx)
    assert got[0].shape == (32, 48, 3) and same_all(got, VR.no_history(cur, albedo))


# ---- the denoiser behind it -----------------------------------------------------------------------------------------------------------
def test_denoise_temporal_equals_denoise_planes(ctx):
    from pbrpathtracer_amd import ptk
    arrays, cam = RC.scene("s_cornell")
    stage(ctx, arrays, cam)
    ext = extent_of(arrays)
    prm = ptk.temporal_defaults(ext); vp = ptk.variance_defaults(ext)
    for k in range(3):
        frame(ctx, MC.orbit(cam, float(k)))
        ctx.temporal_frame(prm, reset=not k, render_features=False, moments=True)
    ctx.temporal_variance(vp)
    color, count = ctx.read_temporal()
    var = ctx.read_temporal_variance()[1]
    tri, emission = ctx.read_feature(ptk.FEAT_TRIANGLE), ctx.read_feature(ptk.FEAT_EMISSION)
    guides = [ctx.read_feature(k) for k in (ptk.FEAT_NORMAL, ptk.FEAT_POSITION, ptk.FEAT_ALBEDO)]
    mask = VR.denoise_mask(count, tri, emission)
    assert (mask == 0).sum() > 500 and (mask < 0).any()
    results = []
    for variance in (False, True):
        dprm = ptk.denoise_defaults(ext, variance=variance)
        ctx.denoise_temporal(dprm, variance=variance)
        got = ctx.read_denoised()
        want = ctx.denoise_planes(color, mask, guides[0], guides[1], dprm, albedo=guides[2], variance=var if variance else None)
        assert same(got, want), variance
        assert not np.array_equal(got, color) and np.isfinite(got).all()
        rgb = ctx.resolve_denoised_rgb8()
        assert rgb.shape == (H, W, 3) and rgb.max() > 0
        results.append(got)
    assert not np.array_equal(results[0], results[1])
    # a plain temporal result is served as well - without the flag
    frame(ctx, MC.orbit(cam, 3.0))
    ctx.temporal_frame(prm, render_features=False)
    dprm = ptk.denoise_defaults(ext)
    assert ctx.L.ptk_denoise_temporal(ctx.h, C.byref(dprm), ptk.DENOISE_VARIANCE) == BAD_ARG
    ctx.denoise_temporal(dprm, variance=False)
    color, count = ctx.read_temporal()
    mask = VR.denoise_mask(count, ctx.read_feature(ptk.FEAT_TRIANGLE), ctx.read_feature(ptk.FEAT_EMISSION))
    guides = [ctx.read_feature(k) for k in (ptk.FEAT_NORMAL, ptk.FEAT_POSITION, ptk.FEAT_ALBEDO)]
    assert same(ctx.read_denoised(), ctx.denoise_planes(color, mask, guides[0], guides[1], dprm, albedo=guides[2]))


# ---- what the calls leave alone -------------------------------------------------------------------------------------------------------
def test_frame_state_is_left_alone(ctx):
    from pbrpathtracer_amd import ptk
    arrays, cam = RC.scene("s_cornell")
    stage(ctx, arrays, cam)
    ext = extent_of(arrays)
    prm = ptk.temporal_defaults(ext); vp = ptk.variance_defaults(ext); dprm = ptk.denoise_defaults(ext, variance=True)
    mask = feature_mask(True)

    def state(adaptive):
        s = dict(accum=ctx.read_accum(), rgb8=ctx.resolve_rgb8(), samples=np.array(ctx.samples()))
        s.update({nm: ctx.read_feature(k) for k, nm in enumerate(ptk.FEAT_NAMES) if (mask >> k) & 1})
        if adaptive:
            s.update(counts=ctx.read_sample_counts(), moments=ctx.read_moments())
        return s

    def the_entries():
        for moving in (False, True):
            ctx.temporal_frame(prm, render_features=False, moments=True, moving=moving)
            ctx.temporal_variance(vp)
            ctx.read_temporal_variance()
            ctx.denoise_temporal(dprm)
            ctx.read_denoised()

    ctx.render(0, 8, SEED)
    ctx.render_features(mask, 0, SEED)
    before = state(False)
    the_entries()
    after = state(False)
    for k in before:
        assert same(before[k], after[k]), k
    ctx.render(8, 4, SEED)
    twelve = ctx.read_accum()
    ctx.reset(); ctx.render(0, 12, SEED)
    assert ctx.samples() == 12 and same(twelve, ctx.read_accum())
    ctx.render_adaptive(0.05, 8, 4, 24, SEED)
    ctx.render_features(mask, 0, SEED)
    before = state(True)
    the_entries()
    after = state(True)
    for k in before:
        assert same(before[k], after[k]), k


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
BAD_TEMPORAL = [dict(max_plane_dist=v) for v in (0.0, -1.0, float("nan"), float("inf"))] + \
    [dict(min_normal_dot=v) for v in (-1.5, 1.5, float("nan"), float("inf"))] + \
    [dict(max_history=v) for v in (0.5, 0.0, -1.0, float("nan"), float("inf"))]
BAD_VARIANCE = [dict(radius=v) for v in (0, 4, -1)] + [dict(prefilter=v) for v in (2, -1)] + \
    [dict(min_frames=v) for v in (1.5, 0.0, -2.0, float("nan"), float("inf"))] + \
    [dict(max_plane_dist=v) for v in (0.0, -1.0, float("nan"), float("inf"))] + \
    [dict(min_normal_dot=v) for v in (-1.5, 1.5, float("nan"), float("inf"))]
BAD_DENOISE = [dict(iterations=v) for v in (0, 9)] + [dict(normal_squarings=v) for v in (-1, 8)] + \
    [dict(sigma_z=v) for v in (0.0, float("nan"))] + [dict(sigma_l=v) for v in (-1.0, float("inf"))]


def test_refusals(ctx):
    from pbrpathtracer_amd import ptk
    L = ctx.L
    w, h = 9, 7
    case = VR.moments_case(w, h, 3)
    prev = MC.primed_planes(case["current"], seed=3)
    ins = [np.ascontiguousarray(a) for a in case["current"] + prev + (case["albedo"],) + case["history"] + (case["hist_moments"],)]
    outs = [np.full((h, w, 3), 7.25, f32), np.full((h, w), 7.25, f32), np.full((h, w, 2), 7.25, f32)]
    view = ptk._view(case["hist_view"])
    good = TR.params(0.05)
    ptr = lambda a: None if a is None else a.ctypes.data
    tins = on_device(ctx, ins); touts = on_device(ctx, outs)
    dptr = lambda t: None if t is None else t.data_ptr()

    def moments_call(prm, ww=w, hh=h, drop=(), v=True, p=True, d=True, c=ctx.h, device=False):
        a = [None if k in drop else (dptr(x) if device else ptr(x)) for k, x in enumerate((tins + touts) if device else (ins + outs))]
        desc = ptk.ReprojectDesc(ww, hh, C.pointer(view) if v else None, *a)
        fn = L.ptk_reproject_moments_device if device else L.ptk_reproject_moments
        return fn(c, C.byref(desc) if d else None, C.byref(prm) if p else None)

    prm = ptk._temporal_params(good)
    for device in (False, True):
        assert moments_call(prm, device=device) == ptk.PTK_OK
        for o in outs:
            o[...] = 7.25
        touts = on_device(ctx, outs)
        for bad in BAD_TEMPORAL:
            assert moments_call(ptk._temporal_params(dict(good, **bad)), device=device) == BAD_ARG, bad
        assert moments_call(prm, ww=-1, device=device) == BAD_ARG and moments_call(prm, hh=-1, device=device) == BAD_ARG
        assert moments_call(prm, v=False, device=device) == BAD_ARG and moments_call(prm, p=False, device=device) == BAD_ARG
        assert moments_call(prm, d=False, device=device) == BAD_ARG and moments_call(prm, c=None, device=device) == BAD_ARG
        for k in range(17):
            if k not in (5, 6, 7):                    # prev_position, prev_normal, albedo: optional ...
                assert moments_call(prm, drop=(k,), device=device) == BAD_ARG, k
        # ... but the two planes of the previous geometry go together
        assert moments_call(prm, drop=(5,), device=device) == BAD_ARG and moments_call(prm, drop=(6,), device=device) == BAD_ARG
        assert moments_call(prm, ww=1 << 15, hh=1 << 14, device=device) == LIMIT and moments_call(prm, ww=1, hh=262141, device=device) == LIMIT
        ctx.synchronize()
        for o in (host(touts) if device else outs):
            assert (o == 7.25).all()
    assert moments_call(prm, drop=(5, 6, 7)) == ptk.PTK_OK and not (outs[2] == 7.25).any()

    # the variance planes entries
    planes = [np.ascontiguousarray(a) for a in VR.variance_case(w, h, 3)]
    out = np.full((h, w), 7.25, f32)
    tplanes = on_device(ctx, planes); tout, = on_device(ctx, [out])
    vgood = VR.params(1.0)

    def variance_call(vp, ww=w, hh=h, drop=None, p=True, o=True, c=ctx.h, device=False):
        a = [None if k == drop else (dptr(x) if device else ptr(x)) for k, x in enumerate(tplanes if device else planes)]
        fn = L.ptk_variance_planes_device if device else L.ptk_variance_planes
        return fn(c, ww, hh, *a, C.byref(vp) if p else None, (dptr(tout) if device else ptr(out)) if o else None)

    vp = ptk._variance_params(vgood)
    for device in (False, True):
        for bad in BAD_VARIANCE:
            assert variance_call(ptk._variance_params(dict(vgood, **bad)), device=device) == BAD_ARG, bad
        assert variance_call(vp, ww=-1, device=device) == BAD_ARG and variance_call(vp, hh=-1, device=device) == BAD_ARG
        assert variance_call(vp, p=False, device=device) == BAD_ARG and variance_call(vp, o=False, device=device) == BAD_ARG
        assert variance_call(vp, c=None, device=device) == BAD_ARG
        for k in range(6):
            assert variance_call(vp, drop=k, device=device) == BAD_ARG, k
        assert variance_call(vp, ww=1 << 15, hh=1 << 14, device=device) == LIMIT and variance_call(vp, ww=1, hh=262141, device=device) == LIMIT
    ctx.synchronize()
    assert (out == 7.25).all() and (tout.cpu().numpy() == 7.25).all()

    # the frame entries: a history and a variance that refused calls must leave as they are
    arrays, cam = RC.scene("s_cornell")
    stage(ctx, arrays, cam, 48, 32)
    ext = extent_of(arrays)
    fprm = ptk.temporal_defaults(ext); fvp = ptk.variance_defaults(ext); dprm = ptk.denoise_defaults(ext, variance=True)
    chain = Chain(fprm)
    frame(ctx, cam)
    ctx.temporal_frame(fprm, reset=True, render_features=False, moments=True)
    kept = got_of(ctx)
    assert same_all(kept, chain.step(ctx, reset=True))
    ctx.temporal_variance(fvp)
    ctx.denoise_temporal(dprm)
    kept_var, kept_den = ctx.read_temporal_variance()[1], ctx.read_denoised()
    for bad in BAD_TEMPORAL:
        assert L.ptk_temporal_frame_moments(ctx.h, C.byref(ptk._temporal_params(dict(good, **bad))), 0) == BAD_ARG, bad
    for bad in BAD_VARIANCE:
        assert L.ptk_temporal_variance(ctx.h, C.byref(ptk._variance_params(dict(vgood, **bad)))) == BAD_ARG, bad
    for bad in BAD_DENOISE:
        assert L.ptk_denoise_temporal(ctx.h, C.byref(ptk._denoise_params(dict(dprm.as_dict(), **bad))), 0) == BAD_ARG, bad
    for flags in (4, 8, 0x80000001):
        assert L.ptk_temporal_frame_moments(ctx.h, C.byref(fprm), flags) == BAD_ARG, flags
    assert L.ptk_denoise_temporal(ctx.h, C.byref(dprm), 2) == BAD_ARG
    assert L.ptk_temporal_frame_moments(ctx.h, None, 0) == BAD_ARG and L.ptk_temporal_frame_moments(None, C.byref(fprm), 0) == BAD_ARG
    assert L.ptk_temporal_variance(ctx.h, None) == BAD_ARG and L.ptk_temporal_variance(None, C.byref(fvp)) == BAD_ARG
    assert L.ptk_denoise_temporal(ctx.h, None, 0) == BAD_ARG and L.ptk_denoise_temporal(None, C.byref(dprm), 0) == BAD_ARG
    assert L.ptk_read_temporal_variance(None, None, None) == BAD_ARG and L.ptk_temporal_variance_device_ptr(None, None, None, None) == BAD_ARG
    assert L.ptk_last_variance_ms(None, None, None) == BAD_ARG
    # a missing guide plane: ALBEDO for the static entry, BARY under MOVING, EMISSION for the denoiser
    ctx.render_features(feature_mask(True) & ~(1 << ptk.FEAT_ALBEDO), 0, SEED)
    assert L.ptk_temporal_frame_moments(ctx.h, C.byref(fprm), 0) == BAD_ARG
    assert L.ptk_temporal_frame_moments(ctx.h, C.byref(fprm), ptk.TEMPORAL_MOVING) == BAD_ARG
    assert L.ptk_denoise_temporal(ctx.h, C.byref(dprm), 0) == BAD_ARG
    ctx.render_features(feature_mask(True) & ~(1 << ptk.FEAT_BARY) & ~(1 << ptk.FEAT_EMISSION), 0, SEED)
    assert L.ptk_temporal_frame_moments(ctx.h, C.byref(fprm), ptk.TEMPORAL_MOVING) == BAD_ARG
    assert L.ptk_denoise_temporal(ctx.h, C.byref(dprm), ptk.DENOISE_VARIANCE) == BAD_ARG
    assert same_all(got_of(ctx), kept) and same(ctx.read_temporal_variance()[1], kept_var) and same(ctx.read_denoised(), kept_den)
    # ... and the history is as it was: the next good call blends with it
    frame(ctx, MC.orbit(cam, 2.0))
    assert L.ptk_temporal_frame_moments(ctx.h, C.byref(fprm), 0) == ptk.PTK_OK
    assert same_all(got_of(ctx), chain.step(ctx)) and chain.found.sum() > 150
    # a context without a frame, and one that never reprojected
    c2 = ptk.Context(0)
    try:
        assert c2.L.ptk_temporal_frame_moments(c2.h, C.byref(fprm), 0) == BAD_ARG
        assert c2.L.ptk_temporal_variance(c2.h, C.byref(fvp)) == BAD_ARG and c2.L.ptk_denoise_temporal(c2.h, C.byref(dprm), 0) == BAD_ARG
        stage(c2, arrays, cam, 48, 32)
        c2.render(0, 2, SEED); c2.render_features(feature_mask(True), 0, SEED)
        assert c2.L.ptk_temporal_variance(c2.h, C.byref(fvp)) == BAD_ARG
        assert c2.L.ptk_denoise_temporal(c2.h, C.byref(dprm), 0) == BAD_ARG               # no temporal result
        buf = np.full((32, 48, 2), 7.25, f32)
        assert c2.L.ptk_read_temporal_variance(c2.h, buf.ctypes.data, None) == BAD_ARG and (buf == 7.25).all()
        # the planes entries need no scene, no camera and no frame
        c3 = ptk.Context(0)
        got = c3.variance_planes(*planes, vgood)
        c3.close()
        assert same(got, VR.variance(*planes, vgood))
    finally:
        c2.close()


# ---- the host class and the command line ----------------------------------------------------------------------------------------------
def test_host_class(tmp_path):
    """PathTracer.TemporalFrameMoments renders the guide planes itself and equals the context's rule; TemporalVariance,
    ReadTemporalVariance and DenoiseTemporal over its result"""
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer, camera_from_scene
    pts, scene, _ = S.build_config("C1", str(tmp_path), width=W, height=H, depth=4)
    pt = PathTracer(device=0)
    pt.LoadSceneFile(pts)
    pt.SetSeed(3)
    c = pt.context()
    ext = extent_of(pt.StagedScene())
    prm = ptk.temporal_defaults(ext); vp = ptk.variance_defaults(ext)
    chain = Chain(prm)
    cam = camera_from_scene(scene)
    for k, deg in enumerate((0.0, 2.0, 4.0)):
        cm = MC.orbit(cam, deg)
        pt.SetCamera(cm["pos"], cm["dir"], cm["up"])
        pt.ResetImage()
        pt.RenderFrames(2)
        pt.TemporalFrameMoments()
        got = pt.ReadTemporal() + (pt.ReadTemporalVariance(variance=False)[0],)
        want = chain.step(c)
        assert same_all(got, want), (k, where_differ(got, want))
        assert pt.GetSamples() == 2
    assert chain.found.sum() > 500
    pt.TemporalVariance()
    mom, var = pt.ReadTemporalVariance()
    assert same(mom, want[2]) and same(var, chain.variance(vp))
    color, count = pt.ReadTemporal()
    mask = VR.denoise_mask(count, c.read_feature(ptk.FEAT_TRIANGLE), c.read_feature(ptk.FEAT_EMISSION))
    guides = [c.read_feature(k) for k in (ptk.FEAT_NORMAL, ptk.FEAT_POSITION, ptk.FEAT_ALBEDO)]
    for variance in (True, False):
        pt.DenoiseTemporal(variance=variance)
        dprm = ptk.denoise_defaults(ext, variance)
        want_den = c.denoise_planes(color, mask, guides[0], guides[1], dprm, albedo=guides[2], variance=var if variance else None)
        assert same(pt.ReadDenoised(), want_den), variance
    assert pt.ResolveDenoised().max() > 0 and pt.LastError() == ""
    # the moving mode under TrackMotion, and a plain call between two moments calls
    pt.TrackMotion(True)
    M = pt.GetObjectTransform(0); M[3][:3] += np.array([0.1, 0.0, 0.0], f32)
    staged0 = pt.StagedScene()
    pt.SetObjectTransform(0, M)
    pt.ResetImage(); pt.RenderFrames(2)
    pt.TemporalFrameMoments(moving=True)
    got = pt.ReadTemporal() + (pt.ReadTemporalVariance(variance=False)[0],)
    assert same_all(got, chain.step(c, tables=(pt.StagedScene()["verts"], staged0["verts"])))
    pt.TemporalFrame()
    assert same_all(pt.ReadTemporal(), chain.step(c, moments=False))
    with pytest.raises(ptk.PtkError):
        pt.TemporalVariance()
    pt.TemporalFrameMoments(reset=True)
    assert same_all(pt.ReadTemporal() + (pt.ReadTemporalVariance(variance=False)[0],), chain.step(c, reset=True))


def test_command_line(tmp_path):
    from pbrpathtracer_amd import render, scenes as S
    pts, _, _ = S.build_config("C1", str(tmp_path), width=W, height=H, depth=4)
    png, npy, plain = (str(tmp_path / n) for n in ("out.png", "out.npy", "plain.npy"))
    base = [pts, "--orbit", "4", "--orbit-degrees", "4", "--spp", "2", "--temporal", "--denoise"]
    assert render.main(base + ["--temporal-variance", "-o", png, "--npy", npy]) == 0 and os.path.getsize(png) > 0
    image = np.load(npy)
    assert image.shape == (H, W, 3) and image.dtype == f32 and np.isfinite(image).all() and image.max() > 0.1
    assert render.main(base + ["-o", png, "--npy", plain]) == 0
    assert not np.array_equal(image, np.load(plain))
    assert render.main(base + ["--temporal-variance", "--move-object", "0", "--move-by", "0.2", "0.1", "0", "-o", png, "--npy", npy]) == 0
    moved = np.load(npy)
    assert moved.shape == (H, W, 3) and np.isfinite(moved).all() and not np.array_equal(moved, image)
    # the options go together
    assert render.main([pts, "--orbit", "2", "--temporal", "--temporal-variance"]) == 1
    assert render.main([pts, "--orbit", "2", "--denoise", "--temporal-variance"]) == 1
    assert render.main([pts, "--spp", "1", "--temporal-variance"]) == 1
