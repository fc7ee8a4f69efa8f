"""Guided upsampling (include/ptk.h ptk_render_guides, ptk_upsample_planes, ptk_upsample_frame) on the GPU.  The guide planes at a
resolution of their own are array_equal to ptk_render_features of a context framed at that resolution, and leave the frame alone;
the planes entries, host and device, and the frame entry over its three sources are array_equal - dtype and shape included - to
tests/upsample_rule.py, the numpy float32 restatement of the header's rule; refusals; chaining into the display transform;
upscale.fill_holes; the host class."""
import ctypes as C

import numpy as np
import pytest

import display_rule as DR
import ray_cases as RC
import temporal_rule as TR
import upsample_rule as UR

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD_ARG, LIMIT = -1, -4     # PTK_ERR_BAD_ARG, PTK_ERR_LIMIT
# (W, H) from (w, h): a multiple of the 64x4 block and of the 16x16 tile in neither; ragged in both; smaller than a tile; one low pixel
PAIRS = [((96, 54), (48, 27)), ((100, 50), (33, 17)), ((11, 8), (7, 5)), ((5, 3), (1, 1))]
PLANE_PAIRS = PAIRS + [((96, 54), (96, 54)), ((48, 27), (96, 54))]


def new_ctx():
    from pbrpathtracer_amd import ptk
    return ptk.Context(0)


@pytest.fixture(scope="module")
def ctx():
    c = new_ctx()
    yield c
    c.close()


def same(got, want):
    """array_equal with dtype and shape; NaN == NaN (an invalid pixel may hold one)"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def same2(got, want):
    return same(got[0], want[0]) and same(got[1], want[1])


def extent_of(arrays):
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


# ---- guide planes -------------------------------------------------------------------------------------------------------------------
def features_at(arrays, cam, W, H, sample, seed):
    """all ten planes of ptk_render_features from a context of its own framed at W x H"""
    c = new_ctx()
    try:
        c.upload_scene(arrays); c.set_camera(**cam); c.set_frame(W, H, 4)
        c.render_features(0x3ff, sample, seed)
        return [c.read_feature(k) for k in range(10)]
    finally:
        c.close()


@pytest.mark.parametrize("case", ["s_cornell", "random300"])
def test_guides_equal_the_features_of_a_context_framed_at_their_size(case):
    """random300 draws stochastic opacity and has normal maps: the RNG pixel must be the top-down index at the guides' size"""
    from pbrpathtracer_amd import ptk
    arrays, cam = RC.scene(case)
    if case == "random300":
        t = ptk.normalise_arrays(arrays)["materials"]["tex"][np.unique(ptk.normalise_arrays(arrays)["material"])]
        assert (t[:, 1] >= 0).any() and (t[:, 5] >= 0).any(), "the case is expected to have a normal map and an opacity map"
    sample, seed = 3, 9
    c = new_ctx()
    try:
        c.upload_scene(arrays)
        hits = 0
        for k, ((W, H), (w, h)) in enumerate(PAIRS):
            frameless = None
            if k == 0:                                                     # a frame need not be set
                c.set_camera(**cam)
                c.render_guides(W, H, 0x3ff, sample, seed)
                frameless = [c.read_guide(f) for f in range(10)]
            c.set_frame(w, h, 4)
            c.set_camera(**cam)                                            # pending: no render in between
            c.render_guides(W, H, 0x3ff, sample, seed)
            want = features_at(arrays, cam, W, H, sample, seed)
            for f in range(10):
                got = c.read_guide(f)
                assert same(got, want[f]), (case, W, H, f, np.argwhere(got != want[f])[:3].tolist())
                assert frameless is None or same(frameless[f], want[f]), (case, "no frame", f)
            hits += int((want[ptk.FEAT_TRIANGLE] >= 0).sum())
            view = c.guide_view().as_dict(); wv = TR.view_of(cam, W, H)
            for key in ("pos", "right", "up", "top_left"):
                assert np.array_equal(np.asarray(view[key], f32).view(np.uint32), np.asarray(wv[key], f32).view(np.uint32)), (W, H, key)
            assert f32(view["delta_x"]) == wv["delta_x"] and f32(view["delta_y"]) == wv["delta_y"]
            ptr, nbytes = c.guide_device_ptr(ptk.FEAT_POSITION)
            assert ptr and nbytes == W * H * 12
        assert hits > 1000, "nothing in view: a poor test"
        # a mask of some planes: the others are refused, the size is the guides'
        c.render_guides(11, 8, (1 << ptk.FEAT_MATERIAL) | (1 << ptk.FEAT_NORMAL), sample, seed)
        assert c.read_guide(ptk.FEAT_MATERIAL).shape == (8, 11)
        with pytest.raises(ptk.PtkError):
            c.read_guide(ptk.FEAT_ALBEDO)
    finally:
        c.close()


def test_guides_leave_the_frame_alone():
    arrays, cam = RC.scene("s_cornell")
    results = []
    for with_guides in (True, False):
        c = new_ctx()
        try:
            c.upload_scene(arrays); c.set_camera(**cam); c.set_frame(48, 27, 4); c.reset()
            c.render(0, 2, 5)
            c.render_features(0x3ff, 0, 5)
            if with_guides:
                c.render_guides(100, 50, 0x3ff, 1, 7)
            state = [c.read_accum()] + [c.read_feature(k) for k in range(10)] + [np.int64(c.samples())]
            c.render(2, 2, 5)
            state += [c.read_accum(), np.int64(c.samples())]
            results.append(state)
        finally:
            c.close()
    assert len(results[0]) == len(results[1])
    for a, b in zip(*results):
        assert same(np.asarray(a), np.asarray(b))
    assert results[0][-1] == 4 and results[0][-2].max() > 0


# ---- the planes entries -------------------------------------------------------------------------------------------------------------
def crafted(W, H, w, h, seed):
    """Low and high planes of the analytic scene under one camera, made to meet every arm of the rule: noisy colours, random albedo,
    poisoned invalid low pixels (NaN colour and position), low pixels pushed off their surface (the plane test), low normals
    turned away (the normal test), and - where the low image has room - foreign ids in its four corner pixels, so that a high
    corner pixel finds nothing in ring 0 and takes ring 1 from a 4x4 block that hangs over two edges."""
    rng = np.random.default_rng(seed)
    cam = TR.orbit_camera(10)
    lid, lp, ln = TR.trace_analytic(TR.view_of(cam, w, h), w, h)
    hid, hp, hn = TR.trace_analytic(TR.view_of(cam, W, H), W, H)
    lid, lp, ln = lid.copy(), lp.copy(), ln.copy()
    color = (TR.ALBEDO[np.maximum(lid, 0)] * rng.uniform(0.5, 1.5, (h, w, 3))).astype(f32)
    lalb = rng.uniform(0.0, 1.0, (h, w, 3)).astype(f32); halb = rng.uniform(0.0, 1.0, (H, W, 3)).astype(f32)
    if w >= 4 and h >= 4:
        pick = rng.random((h, w))
        off = (pick < 0.05) & (lid >= 0)
        lp[off] += ln[off] * f32(0.2)
        turned = (pick > 0.95) & (lid >= 0)
        ln[turned] = -ln[turned]
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            lid[y, x] = 99
    inv = lid < 0
    color[inv] = np.nan; lp[inv] = np.nan
    return (color, lid, lp, ln, lalb), (hid, hp, hn, halb)


def variants(lo, hi):
    for albedo in (False, True):
        for wide in (0, 1):
            l = lo if albedo else lo[:4] + (None,)
            g = hi if albedo else hi[:3] + (None,)
            yield (albedo, wide), l, g, UR.params(TR.EXTENT / 100.0, 0.9, wide)


@pytest.mark.parametrize("big,small", PLANE_PAIRS)
def test_planes_equal_the_mirror(ctx, big, small):
    import torch
    (W, H), (w, h) = big, small
    lo, hi = crafted(W, H, w, h, seed=W + 3 * w)
    dev = torch.device("cuda", ctx.device_ordinal())
    to = lambda planes: [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in planes]
    for tag, l, g, p in variants(lo, hi):
        want = UR.upsample(l, g, p)
        got = ctx.upsample_planes(l, g, p)
        assert same2(got, want), (big, small, tag, np.argwhere(got[1] != want[1])[:3].tolist(),
                                   np.argwhere(~((got[0] == want[0]) | (np.isnan(got[0]) & np.isnan(want[0]))))[:3].tolist())
        tl, tg = to(l), to(g)
        torch.cuda.synchronize()
        dgot = ctx.upsample_planes(tl, tg, p)
        ctx.synchronize()
        assert same2([t.cpu().numpy() for t in dgot], want), (big, small, tag)
        # what the poisoned pixels hold reaches no valid high pixel that found its surface
        ok = (g[0] >= 0) & (want[1] < 2)
        assert np.isfinite(got[0][ok]).all()
    ms = ctx.last_upsample_ms()
    assert ms["pack_ms"] >= 0 and ms["kernel_ms"] > 0


def test_crafted_inputs_reach_every_arm():
    """every class, every reason a ring-0 tap is dropped for, ring 1 and ring 1 at an image corner occur in the cases above"""
    total = dict(outside=0, id=0, plane=0, normal=0, weight=0, ring1_taken=0, ring1_pixels_at_corner=0)
    classes = np.zeros(3, np.int64)
    for (W, H), (w, h) in PLANE_PAIRS:
        lo, hi = crafted(W, H, w, h, seed=W + 3 * w)
        _, cls, reasons = UR.upsample(lo, hi, UR.params(TR.EXTENT / 100.0, 0.9, 1), want_reasons=True)
        for k in total:
            total[k] += reasons[k]
        classes += np.bincount(cls.reshape(-1), minlength=3)
        assert (lo[1] < 0).any() or w * h < 16
    print(total, classes.tolist())
    assert all(n > 0 for n in total.values()), total
    assert (classes > 0).all()


def test_zero_sized_images_do_nothing(ctx):
    import torch
    p = UR.params(0.1)
    for (w, h, W, H) in ((0, 0, 4, 4), (4, 4, 0, 0), (0, 3, 2, 2), (0, 0, 0, 0)):
        lo = (np.zeros((h, w, 3), f32), np.zeros((h, w), np.int32), np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32), None)
        hi = (np.zeros((H, W), np.int32), np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32), None)
        out, cls = ctx.upsample_planes(lo, hi, p)
        assert out.shape == (H, W, 3) and cls.shape == (H, W)
    dev = torch.device("cuda", ctx.device_ordinal())
    lo = (torch.zeros((0, 0, 3), device=dev), torch.zeros((0, 0), dtype=torch.int32, device=dev), torch.zeros((0, 0, 3), device=dev),
          torch.zeros((0, 0, 3), device=dev), None)
    hi = (torch.zeros((2, 2), dtype=torch.int32, device=dev), torch.zeros((2, 2, 3), device=dev), torch.zeros((2, 2, 3), device=dev), None)
    out, cls = ctx.upsample_planes(lo, hi, p)
    assert tuple(out.shape) == (2, 2, 3)


# ---- the frame entry ----------------------------------------------------------------------------------------------------------------
w0, h0, W0, H0 = 48, 32, 96, 64


def setup(c, w=w0, h=h0):
    arrays, cam = RC.scene("s_cornell")
    c.upload_scene(arrays); c.set_camera(**cam); c.set_frame(w, h, 4); c.set_tile(0, 1); c.reset()
    return arrays, cam


def guides_of(c, read):
    from pbrpathtracer_amd import ptk
    return tuple(read(k) for k in (ptk.FEAT_MATERIAL, ptk.FEAT_POSITION, ptk.FEAT_NORMAL, ptk.FEAT_ALBEDO))


def rule_of_frame(c, source, p):
    """the rule fed with what the context's readers return"""
    from pbrpathtracer_amd import ptk
    if source == ptk.UPSAMPLE_ACCUM:
        color = UR.frame_inputs(source, s1=c.read_accum(), counts=c.read_sample_counts())
    elif source == ptk.UPSAMPLE_DENOISED:
        color = UR.frame_inputs(source, denoised=c.read_denoised())
    else:
        color = UR.frame_inputs(source, temporal=c.read_temporal()[0])
    ident, pos, nrm, alb = guides_of(c, c.read_feature)
    return UR.upsample((color, ident, pos, nrm, alb), guides_of(c, c.read_guide), p)


def test_frame_entry_over_its_three_sources(ctx):
    from pbrpathtracer_amd import ptk
    arrays, _ = setup(ctx)
    ext = extent_of(arrays)
    ctx.render(0, 4, 5)
    ctx.render_features(0x3ff, 0, 5)
    ctx.denoise_frame(ptk.denoise_defaults(ext), render_features=False)
    ctx.temporal_frame(ptk.temporal_defaults(ext), reset=True, render_features=False)
    ctx.render_guides(W0, H0, ptk.UPSAMPLE_GUIDES, 0, 5)
    seen = np.zeros(3, np.int64)
    for source in (ptk.UPSAMPLE_ACCUM, ptk.UPSAMPLE_DENOISED, ptk.UPSAMPLE_TEMPORAL):
        for p in (ptk.upsample_defaults(ext), UR.params(ext / 400.0, 0.99, 0)):
            ctx.upsample_frame(source, p)
            got = ctx.read_upsampled()
            want = rule_of_frame(ctx, source, p)
            assert same2(got, want), (source, np.argwhere(got[1] != want[1])[:3].tolist())
            seen += np.bincount(got[1].reshape(-1), minlength=3)
    assert got[0].shape == (H0, W0, 3) and seen[0] > 0 and seen[2] > 0
    color, cls, width, height = ctx.upsampled_device_ptr()
    assert color and cls and (width, height) == (W0, H0)
    # the sources differ, so the three were not one
    ctx.upsample_frame(ptk.UPSAMPLE_ACCUM, ptk.upsample_defaults(ext))
    assert not np.array_equal(ctx.read_upsampled()[0], got[0], equal_nan=True)
    assert ctx.samples() == 4


def test_frame_entry_after_an_adaptive_render(ctx):
    from pbrpathtracer_amd import ptk
    arrays, _ = setup(ctx)
    ext = extent_of(arrays)
    res = ctx.render_adaptive(0.05, 2, 2, 8, 11)
    counts = ctx.read_sample_counts()
    assert res["rounds"] > 1 and len(np.unique(counts)) > 1, "the render is expected to leave per-pixel counts"
    ctx.render_features(ptk.UPSAMPLE_GUIDES, 0, 11)
    ctx.render_guides(W0, H0, ptk.UPSAMPLE_GUIDES, 0, 11)
    p = ptk.upsample_defaults(ext)
    ctx.upsample_frame(ptk.UPSAMPLE_ACCUM, p)
    got = ctx.read_upsampled()
    assert same2(got, rule_of_frame(ctx, ptk.UPSAMPLE_ACCUM, p))
    # ... and the same after a plain render into the same context
    ctx.reset(); ctx.render(0, 3, 11)
    ctx.upsample_frame(ptk.UPSAMPLE_ACCUM, p)
    assert same2(ctx.read_upsampled(), rule_of_frame(ctx, ptk.UPSAMPLE_ACCUM, p))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    from pbrpathtracer_amd import ptk
    L = ctx.L
    w, h, W, H = 7, 5, 11, 8
    lo, hi = crafted(W, H, w, h, seed=1)
    lo = [np.ascontiguousarray(a) for a in lo]; hi = [np.ascontiguousarray(a) for a in hi]
    out = np.full((H, W, 3), 7.0, f32); cls = np.full((H, W), 7, np.int32)
    good = ptk.UpsampleParams(0.1, 0.9, 1)
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(prm=good, l=lo, g=hi, size=(w, h, W, H), o=(out, cls), c=ctx.h):
        return L.ptk_upsample_planes(c, size[0], size[1], *(ptr(a) for a in l), size[2], size[3], *(ptr(a) for a in g),
                                     C.byref(prm) if prm is not None else None, ptr(o[0]), ptr(o[1]))

    nan = float("nan")
    for bad in (ptk.UpsampleParams(0.0, 0.9, 1), ptk.UpsampleParams(nan, 0.9, 1), ptk.UpsampleParams(float("inf"), 0.9, 1),
                ptk.UpsampleParams(-1.0, 0.9, 1), ptk.UpsampleParams(0.1, 1.5, 1), ptk.UpsampleParams(0.1, nan, 1),
                ptk.UpsampleParams(0.1, -1.01, 1), ptk.UpsampleParams(0.1, 0.9, 2), ptk.UpsampleParams(0.1, 0.9, -1), None):
        assert call(prm=bad) == BAD_ARG
    assert call(l=lo[:4] + [None]) == BAD_ARG and call(g=hi[:3] + [None]) == BAD_ARG         # one albedo plane alone
    for k in range(4):
        assert call(l=[None if j == k else a for j, a in enumerate(lo)]) == BAD_ARG
    for k in range(3):
        assert call(g=[None if j == k else a for j, a in enumerate(hi)]) == BAD_ARG
    assert call(o=(None, cls)) == BAD_ARG and call(o=(out, None)) == BAD_ARG
    assert call(size=(-1, h, W, H)) == BAD_ARG and call(size=(w, h, W, -2)) == BAD_ARG
    assert call(size=(1 << 15, 1 << 14, W, H)) == LIMIT and call(size=(w, h, 1, 4 * 65535 + 1)) == LIMIT
    assert call(c=None) == BAD_ARG
    assert (out == 7.0).all() and (cls == 7).all()
    assert call(size=(0, h, W, H)) == ptk.PTK_OK and call(size=(w, h, W, 0)) == ptk.PTK_OK
    assert (out == 7.0).all() and (cls == 7).all()
    assert call() == ptk.PTK_OK and same2((out, cls), UR.upsample(lo, hi, good))

    # the frame entry and the guides
    c = new_ctx()
    try:
        prm = ptk.upsample_defaults(5.0)
        with pytest.raises(ptk.PtkError):
            c.render_guides(8, 8)                                          # no scene
        arrays, cam = RC.scene("s_cornell")
        c.upload_scene(arrays); c.set_camera(**cam)
        with pytest.raises(ptk.PtkError):
            c.read_upsampled()
        with pytest.raises(ptk.PtkError):
            c.guide_view()
        with pytest.raises(ptk.PtkError):
            c.upsample_frame(ptk.UPSAMPLE_ACCUM, prm)                      # no frame
        c.set_frame(w0, h0, 4); c.reset(); c.render(0, 1, 3)
        with pytest.raises(ptk.PtkError):
            c.upsample_frame(ptk.UPSAMPLE_ACCUM, prm)                      # no feature planes
        c.render_features(ptk.UPSAMPLE_GUIDES, 0, 3)
        with pytest.raises(ptk.PtkError):
            c.upsample_frame(ptk.UPSAMPLE_ACCUM, prm)                      # no guides
        assert L.ptk_render_guides(c.h, -1, 4, 0, 0, 1) == BAD_ARG and L.ptk_render_guides(c.h, 4, 4, 0, 0, 1 << 10) == BAD_ARG
        assert L.ptk_render_guides(c.h, 1 << 15, 1 << 14, 0, 0, 1) == LIMIT
        assert L.ptk_render_guides(c.h, 0, 4, 0, 0, 1) == ptk.PTK_OK
        c.render_guides(W0, H0, ptk.UPSAMPLE_GUIDES & ~(1 << ptk.FEAT_ALBEDO))
        with pytest.raises(ptk.PtkError):
            c.upsample_frame(ptk.UPSAMPLE_ACCUM, prm)                      # a guide plane is missing
        c.render_guides(W0, H0 + 1)
        with pytest.raises(ptk.PtkError):
            c.upsample_frame(ptk.UPSAMPLE_ACCUM, prm)                      # W*h != H*w
        c.render_guides(W0, H0)
        for source in (ptk.UPSAMPLE_DENOISED, ptk.UPSAMPLE_TEMPORAL, 3, -1):
            with pytest.raises(ptk.PtkError):
                c.upsample_frame(source, prm)                              # the source does not exist
        with pytest.raises(ptk.PtkError):
            c.upsample_frame(ptk.UPSAMPLE_ACCUM, ptk.UpsampleParams(0.0, 0.9, 1))
        c.upsample_frame(ptk.UPSAMPLE_ACCUM, prm)
        kept = c.read_upsampled()
        c.render_features(1 << ptk.FEAT_MATERIAL, 0, 3)
        with pytest.raises(ptk.PtkError):
            c.upsample_frame(ptk.UPSAMPLE_ACCUM, prm)                      # the last ptk_render_features lacks three planes
        c.render_features(ptk.UPSAMPLE_GUIDES, 0, 3)
        c.set_tile(0, 2)
        with pytest.raises(ptk.PtkError):
            c.upsample_frame(ptk.UPSAMPLE_ACCUM, prm)                      # a tile split
        with pytest.raises(ptk.PtkError):
            c.render_guides(W0, H0)
        assert same2(c.read_upsampled(), kept), "a refused call leaves the result alone"
        c.set_tile(0, 1)
        c.set_frame(w0 + 16, h0, 4)                                        # the planes go with the resolution they were rendered at
        with pytest.raises(ptk.PtkError):
            c.upsample_frame(ptk.UPSAMPLE_ACCUM, prm)
    finally:
        c.close()


# ---- chaining -----------------------------------------------------------------------------------------------------------------------
def test_the_result_chains_into_the_display_transform(ctx):
    import torch
    from pbrpathtracer_amd import ptk
    arrays, _ = setup(ctx)
    ctx.render(0, 4, 5)
    ctx.render_features(ptk.UPSAMPLE_GUIDES, 0, 5)
    ctx.render_guides(W0, H0)
    ctx.upsample_frame(ptk.UPSAMPLE_ACCUM, ptk.upsample_defaults(extent_of(arrays)))
    color, _, width, height = ctx.upsampled_device_ptr()
    rgb = torch.zeros((height, width, 3), dtype=torch.uint8, device=torch.device("cuda", ctx.device_ordinal()))
    torch.cuda.synchronize()
    p = DR.params(mode=DR.MANUAL, exposure=1.5)
    prm = ptk.display_defaults(**p)
    ctx._chk(ctx.L.ptk_display_planes_device(ctx.h, width, height, C.c_void_p(color), C.byref(prm), C.c_void_p(rgb.data_ptr()), None),
             "ptk_display_planes_device")
    ctx.synchronize()
    want, _ = DR.display(ctx.read_upsampled()[0], p, ptk.display_srgb_table(), None)
    got = rgb.cpu().numpy()
    assert same(got, want) and len(np.unique(got)) > 50


# ---- upscale.fill_holes -------------------------------------------------------------------------------------------------------------
def test_fill_holes_writes_exactly_the_holes(ctx):
    from pbrpathtracer_amd import ptk, upscale
    arrays, _ = setup(ctx)
    ctx.render(0, 4, 5)
    ctx.render_features(ptk.UPSAMPLE_GUIDES, 0, 5)
    ctx.render_guides(W0, H0)
    ctx.upsample_frame(ptk.UPSAMPLE_ACCUM, UR.params(extent_of(arrays) / 100.0, 0.9, 0))      # (no ring 1: more holes)
    color, cls = ctx.read_upsampled()
    holes = cls == 2
    assert 0 < holes.sum() < holes.size // 4
    spp = 8
    out, info = upscale.fill_holes(ctx, color, cls, ctx.guide_view(), spp, 4, seed=21, first_sample=2, key_base=1000)
    assert out is not color and out.dtype == f32
    assert np.array_equal(np.stack([info["rows"], info["cols"]], 1), np.argwhere(holes))
    assert np.array_equal(out[~holes].view(np.uint32), color[~holes].view(np.uint32))
    sums = ctx.trace_rays(info["origins"], info["dirs"], 4, 2, spp, 21, key_base=1000)
    assert same(sums, info["sums"]) and same(out[holes], (sums / f32(spp)).astype(f32))
    assert (out[holes] != color[holes]).any() and np.isfinite(out[holes]).all()
    assert upscale.low_resolution(W0, H0, 2.0) == (w0, h0) and upscale.low_resolution(100, 50, 3.0) == (34, 17)
    with pytest.raises(ValueError):
        upscale.low_resolution(97, 64, 2.0)
    assert np.allclose(sum(upscale.class_shares(cls)), 1.0)


# ---- the host class, through the C host layer ---------------------------------------------------------------------------------------
def test_host_class(tmp_path):
    """PathTracer.RenderGuides / UpsampleFrame go through pth_* and give the frame entry's bits"""
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    pts, _, _ = S.build_config("C1", str(tmp_path), width=w0, height=h0, depth=4)
    pt = PathTracer(device=0)
    pt.LoadSceneFile(pts)
    pt.SetSeed(3)
    pt.RenderFrames(4)
    with pytest.raises(ptk.PtkError):
        pt.UpsampleFrame()                                                 # no guides yet
    pt.RenderGuides(W0, H0)
    pt.UpsampleFrame()
    got = pt.ReadUpsampled()
    c = pt.context()
    prm = ptk.upsample_defaults(extent_of(pt.StagedScene()))
    want = rule_of_frame(c, ptk.UPSAMPLE_ACCUM, prm)
    assert same2(got, want) and got[0].shape == (H0, W0, 3)
    assert same(pt.ReadGuide(ptk.FEAT_NORMAL), c.read_guide(ptk.FEAT_NORMAL))
    c.upsample_frame(ptk.UPSAMPLE_ACCUM, prm)
    assert same2(c.read_upsampled(), got)
    pt.DenoiseFrame()
    pt.UpsampleFrame(ptk.UPSAMPLE_DENOISED, UR.params(prm.max_plane_dist, 0.95, 0))
    assert same2(pt.ReadUpsampled(), rule_of_frame(c, ptk.UPSAMPLE_DENOISED, UR.params(prm.max_plane_dist, 0.95, 0)))
    assert pt.GetSamples() == 4
    with pytest.raises(ptk.PtkError):
        pt.UpsampleFrame(ptk.UPSAMPLE_TEMPORAL)


def test_command_line(tmp_path, capsys):
    from pbrpathtracer_amd import render, scenes as S
    from pbrpathtracer_amd.pathtracer import image_load
    pts, _, _ = S.build_config("C1", str(tmp_path), width=W0, height=H0, depth=4)
    png = str(tmp_path / "up.png")
    assert render.main([pts, "--spp", "4", "--seed", "3", "--upscale", "2", "-o", png]) == 0
    assert image_load(png).shape[:2] == (H0, W0)
    text = capsys.readouterr().out
    assert f"traced {w0}x{h0}" in text and f"shown {W0}x{H0}" in text and "bilinear" in text and "holes" in text
    assert render.main([pts, "--spp", "2", "--upscale", "2", "--denoise", "--display", "aces", "--fill-holes", "4", "-o", png]) == 0
    assert "holes traced at 4 spp" in capsys.readouterr().out and image_load(png)[..., :3].any()
    assert render.main([pts, "--spp", "1", "--fill-holes", "4"]) == 1
    assert render.main([pts, "--spp", "1", "--upscale", "0.5"]) == 1
    assert render.main([pts, "--spp", "1", "--upscale", "2", "--orbit", "2"]) == 1
    assert render.main([pts, "--spp", "1", "--upscale", "1000", "-o", png]) == 1
    assert "aspect ratio" in capsys.readouterr().err
