"""Temporal reprojection over moving geometry (include/ptk.h ptk_geometry_snapshot, ptk_render_motion, ptk_reproject_planes_moving,
ptk_temporal_frame_moving) on the GPU: every output array_equal - dtype, shape and NaN positions included - to tests/motion_rule.py,
the numpy float32 restatement of the header's rule.  The planes entry over sizes that split blocks; ptk_render_motion over the scenes
and motions of tests/motion_cases.py; what happens without a snapshot; the snapshot's place among queued updates; the frame entry
chained over camera and object moves; what the calls must not touch; refusals; the host class and the command line; and one check
that the feature does its job."""
import ctypes as C
import os

import numpy as np
import pytest

import motion_cases as MC
import motion_rule as MR
import ray_cases as RC
import temporal_rule as TR

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD_ARG = -1            # PTK_ERR_BAD_ARG
W, H = MC.W, MC.H
SEED = 5


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
    """array_equal with dtype and shape; NaN == NaN"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def same_all(got, want):
    return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def where_differ(got, want):
    return [np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:3].tolist() for g, w in zip(got, want)]


def masks():
    from pbrpathtracer_amd import ptk
    four = (1 << ptk.FEAT_TRIANGLE) | (1 << ptk.FEAT_BARY) | (1 << ptk.FEAT_POSITION) | (1 << ptk.FEAT_NORMAL)
    return four, four | (1 << ptk.FEAT_MATERIAL)


def four_planes(ctx):
    from pbrpathtracer_amd import ptk
    return tuple(ctx.read_feature(k) for k in (ptk.FEAT_TRIANGLE, ptk.FEAT_BARY, ptk.FEAT_POSITION, ptk.FEAT_NORMAL))


def current_of(ctx):
    """the current frame as the context reports it: accumulator, counts and the three guide planes of the reprojection"""
    from pbrpathtracer_amd import ptk
    color, count = TR.frame_inputs(ctx.read_accum(), ctx.read_sample_counts())
    return (color, count, ctx.read_feature(ptk.FEAT_MATERIAL), ctx.read_feature(ptk.FEAT_POSITION), ctx.read_feature(ptk.FEAT_NORMAL))


def extent_of(arrays):
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


# ---- the planes entries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 35), (130, 70)])
def test_planes_equal_the_mirror(ctx, w, h):
    import torch
    case = TR.random_case(w, h, seed=w + h)
    cur, hist, view = case["current"], case["history"], case["hist_view"]
    Xp, npr = MC.primed_planes(cur, w, case["extent"])
    dev = torch.device("cuda", ctx.device_ordinal())
    to = lambda planes: [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in planes]
    tcur, thist, tprimed = to(cur), to(hist), to((Xp, npr))
    torch.cuda.synchronize()
    inv = cur[2] < 0
    for match in (0, 1):
        for max_history in (1.0, 64.0):
            p = TR.params(case["extent"] / 100.0, 0.9, max_history, match)
            tag = (w, h, match, max_history)
            want = MR.reproject_moving(view, cur, Xp, npr, hist, p, want_found=True)
            got = ctx.reproject_planes_moving(view, cur, Xp, npr, hist, p)
            dgot = ctx.reproject_planes_moving(view, tcur, tprimed[0], tprimed[1], thist, p)
            ctx.synchronize()
            assert same_all(got, want[:2]), (tag, where_differ(got, want))
            assert same_all([t.cpu().numpy() for t in dgot], want[:2]), tag
            assert np.array_equal(bits(got[0])[inv], bits(cur[0])[inv]) and np.array_equal(bits(got[1])[inv], bits(cur[1])[inv])
            assert np.isfinite(got[0][~inv]).all() and np.isfinite(got[1][~inv]).all()
            # primed = unprimed: the plain rule, and the plain entry on the same context
            plain = TR.reproject(view, cur, hist, p, want_found=True)
            got0 = ctx.reproject_planes_moving(view, cur, cur[3], cur[4], hist, p)
            assert same_all(got0, plain[:2]), tag
            assert same_all(got0, ctx.reproject_planes(view, cur, hist, p)), tag
            if w >= 67:
                assert want[2].sum() > 300 and not np.array_equal(want[2], plain[2]), tag


def test_zero_sized_image_does_nothing(ctx):
    from pbrpathtracer_amd import ptk
    prm = ptk.temporal_defaults(1.0)
    view = ptk._view(TR.view_of(TR.orbit_camera(0.0), 4, 4))
    none = [None] * 12
    assert ctx.L.ptk_reproject_planes_moving(ctx.h, 0, 7, C.byref(view), *none, C.byref(prm), None, None) == ptk.PTK_OK
    assert ctx.L.ptk_reproject_planes_moving_device(ctx.h, 5, 0, C.byref(view), *none, C.byref(prm), None, None) == ptk.PTK_OK


# ---- ptk_render_motion over scenes and motions --------------------------------------------------------------------------------------
def stage(ctx, arrays, cam, w=W, h=H, depth=4):
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(w, h, depth); ctx.set_tile(0, 1); ctx.reset()


@pytest.mark.parametrize("name", MC.MOTIONS)
@pytest.mark.parametrize("case", MC.SCENES)
def test_render_motion_equals_the_mirror(ctx, case, name):
    """snapshot, update_geometry, render, features, motion: the outputs equal the mirror fed with the read-back feature planes and
    the two vertex tables"""
    arrays, cam = RC.scene(case)
    first, was, now, _ = MC.motion(case, name)
    prev, cur = MC.tables(case, name)
    four, _ = masks()
    stage(ctx, arrays, cam)
    ctx.update_geometry(first, was)                 # the state the snapshot is taken in (the uploaded one for most motions)
    ctx.snapshot_geometry()
    ctx.update_geometry(first, now)
    ctx.render(0, 1, SEED)
    ctx.render_features(four, 0, SEED)
    view = TR.view_of(MC.previous_camera(case), W, H)
    ctx.render_motion(view)
    got = ctx.read_motion()
    planes = four_planes(ctx)
    want = MR.render_motion(view, planes, cur, prev)
    assert same_all(got, want), (case, name, where_differ(got, want))
    _, _, (miss, unmoved, moved) = MR.previous(*planes, cur, prev, want_cases=True)
    assert miss.any() and unmoved.any() and moved.any(), (case, name)
    assert np.isnan(got[2][miss]).all()
    still = ~moved
    assert np.array_equal(bits(got[0])[still], bits(planes[2])[still]) and np.array_equal(bits(got[1])[still], bits(planes[3])[still])
    if name == "rigid":
        assert (moved & np.isfinite(got[2]).all(axis=-1)).sum() >= 100
    # no view: NaN everywhere, X' and n' all the same
    ctx.render_motion(None)
    none = ctx.read_motion()
    assert same_all(none[:2], want[:2]) and np.isnan(none[2]).all()
    # any pointer of the reader may be null
    only = np.empty((H, W, 2), f32)
    assert ctx.L.ptk_read_motion(ctx.h, None, None, only.ctypes.data) == 0 and np.isnan(only).all()
    assert ctx.L.ptk_read_motion(ctx.h, None, None, None) == 0
    a = C.c_void_p(); b = C.c_void_p(); m = C.c_void_p(); n = C.c_size_t()
    assert ctx.L.ptk_motion_device_ptr(ctx.h, C.byref(a), C.byref(b), C.byref(m), C.byref(n)) == 0
    assert a.value and b.value == a.value + 12 * W * H and m.value == a.value + 24 * W * H and n.value == W * H
    assert ctx.motion_device_ptr() == (a.value, b.value, m.value, n.value)
    t = ctx.last_motion_ms()
    assert t["motion_ms"] > 0 and t["temporal_ms"] == 0


# ---- without a snapshot ---------------------------------------------------------------------------------------------------------------
def frame(ctx, cam, spp=4, seed=SEED, mask=None):
    ctx.set_camera(**cam); ctx.reset(); ctx.render(0, spp, seed)
    ctx.render_features(masks()[1] if mask is None else mask, 0, seed)


def test_no_snapshot_means_nothing_moved(fresh):
    from pbrpathtracer_amd import ptk
    arrays, cam = RC.scene("s_cornell")
    a, b = fresh, ptk.Context(0)
    try:
        prm = ptk.temporal_defaults(extent_of(arrays))
        for c in (a, b):
            stage(c, arrays, cam, 96, 54)
        # geometry that moved before the first frame, and no snapshot: nothing to compare with
        first, was, now, _ = MC.motion("s_cornell", "rigid")
        for c in (a, b):
            c.update_geometry(first, now)
        for k, deg in enumerate((0.0, 2.0, 5.0)):
            for c in (a, b):
                frame(c, MC.orbit(cam, deg))
            a.temporal_frame(prm, render_features=False, moving=True)
            b.temporal_frame(prm, render_features=False)
            ga, gb = a.read_temporal(), b.read_temporal()
            assert same_all(ga, gb), k
            planes = four_planes(a)
            pp, pn, mv = a.read_motion()
            assert np.array_equal(bits(pp), bits(planes[2])) and np.array_equal(bits(pn), bits(planes[3]))
            if k == 0:
                assert np.isnan(mv).all()
            else:
                assert same(mv, MR.motion(last_view, planes[0], planes[2])) and np.isfinite(mv).any()
            last_view = a.get_view().as_dict()
        assert not same(ga[0], current_of(a)[0])                           # (there was history to blend)
    finally:
        b.close()


# ---- the snapshot's place among queued updates -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("caller_stream", [False, True])
def test_snapshot_is_ordered_among_updates(caller_stream):
    """snapshot, update A, update B, render, features, motion with nothing waited for in between: previous = the state at the
    snapshot, current = after B; then snapshot, update, snapshot, update: previous = the middle state"""
    import torch
    from pbrpathtracer_amd import ptk
    case = "random300"
    arrays, cam = RC.scene(case)
    base = np.ascontiguousarray(arrays["verts"], f32).reshape(-1, 9)
    first, _, now_a, _ = MC.motion(case, "rigid")
    _, _, now_b, _ = MC.motion(case, "jitter")
    _, _, now_c, _ = MC.motion(case, "scale")
    n = len(now_a)

    def table(now):
        t = base.copy(); t[first:first + n] = now
        return t

    four, _ = masks()
    view = TR.view_of(MC.previous_camera(case), W, H)
    stream = torch.cuda.Stream() if caller_stream else None
    c = ptk.Context(0)
    try:
        if stream is not None:
            c.set_stream(stream.cuda_stream)
        stage(c, arrays, cam)
        c.update_geometry(first, base[first:first + n])        # (the one-off topology download happens here)
        c.snapshot_geometry()
        c.update_geometry(first, now_a)
        c.update_geometry(first, now_b)
        c.render(0, 1, SEED); c.render_features(four, 0, SEED); c.render_motion(view)
        got = c.read_motion()
        planes = four_planes(c)
        want = MR.render_motion(view, planes, table(now_b), base)
        assert same_all(got, want), where_differ(got, want)
        assert not same_all(got[:2], MR.render_motion(view, planes, table(now_b), table(now_a))[:2])
        c.snapshot_geometry()
        c.update_geometry(first, now_c)
        c.snapshot_geometry()
        c.update_geometry(first, now_a)
        c.render(0, 1, SEED); c.render_features(four, 0, SEED); c.render_motion(view)
        got = c.read_motion()
        planes = four_planes(c)
        want = MR.render_motion(view, planes, table(now_a), table(now_c))
        assert same_all(got, want), where_differ(got, want)
        assert not same_all(got[:2], MR.render_motion(view, planes, table(now_a), table(now_b))[:2])
    finally:
        c.synchronize()
        c.close()


# ---- the frame entry ------------------------------------------------------------------------------------------------------------------
class Chain:
    """the mirror chained over the frame calls of a context, in either mode"""

    def __init__(self, prm):
        self.prm, self.hist, self.view, self.found = prm, None, None, None

    def step(self, ctx, cur_table, prev_table, moving=True, reset=False):
        """the mirror's result for the context's current frame, and - in moving mode - the motion planes the call leaves"""
        cur = current_of(ctx)
        view = ctx.get_view().as_dict()
        use = self.hist is not None and not reset
        planes = four_planes(ctx) if moving else None
        if moving:
            motion = MR.render_motion(self.view if use else None, planes, cur_table, prev_table)
        if not use:
            out, n = TR.no_history(cur); self.found = np.zeros(n.shape, bool)
        elif moving:
            out, n, self.found = MR.reproject_moving(self.view, cur, motion[0], motion[1], self.hist, self.prm, want_found=True)
        else:
            out, n, self.found = TR.reproject(self.view, cur, self.hist, self.prm, want_found=True)
        self.hist, self.view = (out, n) + cur[2:], view
        return ((out, n), motion) if moving else (out, n)


def card_table(k):
    arrays, first, n = MC.quality_scene()
    t = np.ascontiguousarray(arrays["verts"], f32).reshape(-1, 9).copy()
    t[first:first + n] = MC.card_verts(k)
    return t


def move_card(ctx, k):
    _, first, _ = MC.quality_scene()
    ctx.snapshot_geometry()
    ctx.update_geometry(first, MC.card_verts(k))


def card_pixels(ctx):
    from pbrpathtracer_amd import ptk
    _, first, n = MC.quality_scene()
    tri = ctx.read_feature(ptk.FEAT_TRIANGLE)
    return (tri >= first) & (tri < first + n)


def test_frame_chain_over_camera_and_object_moves(fresh):
    """(a context of its own: its first call has no history without being told so)"""
    from pbrpathtracer_amd import ptk
    ctx = fresh
    arrays, _, _ = MC.quality_scene()
    cam = MC.QUALITY_CAM
    stage(ctx, arrays, cam, 96, 54)
    prm = ptk.temporal_defaults(MC.EXTENT)
    chain = Chain(prm)
    for k, deg in enumerate((0.0, 1.0, 2.0, 4.0)):
        if k:
            move_card(ctx, k)
        frame(ctx, MC.orbit(cam, deg))
        ctx.temporal_frame(prm, render_features=False, moving=True)
        got, gm = ctx.read_temporal(), ctx.read_motion()
        want, wm = chain.step(ctx, card_table(k), card_table(k - 1) if k else None)
        assert same_all(got, want), (k, where_differ(got, want))
        assert same_all(gm, wm), (k, where_differ(gm, wm))
        card = card_pixels(ctx)
        assert card.sum() > 200
        if k:
            assert chain.found[card].mean() > 0.5 and (got[1][chain.found & card] >= 8.0).all()
            assert np.isfinite(gm[2][card]).all() and np.abs(gm[2][card]).max() > 1.0
            assert not np.array_equal(gm[0][card], current_of(ctx)[3][card])
        else:
            assert np.isnan(gm[2]).all()
        t = ctx.last_motion_ms()
        assert t["motion_ms"] > 0 and t["temporal_ms"] > 0
    # the convenience path renders the five planes itself
    move_card(ctx, 4)
    ctx.set_camera(**MC.orbit(cam, 5.0)); ctx.reset(); ctx.render(0, 4, SEED)
    ctx.temporal_frame(prm, seed=SEED, moving=True)
    want, wm = chain.step(ctx, card_table(4), card_table(3))
    assert same_all(ctx.read_temporal(), want) and same_all(ctx.read_motion(), wm)


def test_frame_tile_split(ctx):
    import feature_truth as FT
    from pbrpathtracer_amd import ptk
    arrays, _, _ = MC.quality_scene()
    cam = MC.QUALITY_CAM
    w, h = 96, 54
    stage(ctx, arrays, cam, w, h)
    prm = ptk.temporal_defaults(MC.EXTENT)
    chain = Chain(prm)
    frame(ctx, cam)
    ctx.temporal_frame(prm, reset=True, render_features=False, moving=True)
    want, _ = chain.step(ctx, card_table(0), None, reset=True)
    assert same_all(ctx.read_temporal(), want)
    owned = np.ascontiguousarray(FT.owned_mask(w, h, 0, 2)[::-1])
    try:
        # guide planes of the whole frame, samples on this rank's tiles only: the other pixels have nc = 0 and take the history
        move_card(ctx, 1)
        ctx.set_camera(**MC.orbit(cam, 1.0)); ctx.render_features(masks()[1], 0, SEED)
        ctx.set_tile(0, 2); ctx.reset(); ctx.render(0, 4, SEED)
        ctx.temporal_frame(prm, render_features=False, moving=True)
        got, gm = ctx.read_temporal(), ctx.read_motion()
        assert np.array_equal(ctx.read_sample_counts() > 0, owned)
        want, wm = chain.step(ctx, card_table(1), card_table(0))
        assert same_all(got, want), where_differ(got, want)
        assert same_all(gm, wm)
        took = chain.found & ~owned
        assert took.sum() > 500 and (got[1][took] == 4.0).all()
        assert (chain.found & card_pixels(ctx) & ~owned).any() and (chain.found & card_pixels(ctx) & owned).any()
        # guide planes of the split frame: the pixels of the other rank are misses
        move_card(ctx, 2)
        frame(ctx, MC.orbit(cam, 2.0))
        ctx.temporal_frame(prm, render_features=False, moving=True)
        got, gm = ctx.read_temporal(), ctx.read_motion()
        want, wm = chain.step(ctx, card_table(2), card_table(1))
        assert same_all(got, want), where_differ(got, want)
        assert same_all(gm, wm)
        assert (chain.hist[2][~owned] < 0).all() and np.isnan(gm[2][~owned]).all() and (chain.found & owned).sum() > 500
    finally:
        ctx.set_tile(0, 1)


def test_the_two_frame_entries_share_one_history(ctx):
    from pbrpathtracer_amd import ptk
    arrays, _, _ = MC.quality_scene()
    cam = MC.QUALITY_CAM
    stage(ctx, arrays, cam, 96, 54)
    prm = ptk.temporal_defaults(MC.EXTENT)
    chain = Chain(prm)
    for k, moving in enumerate((False, True, False, True)):
        if k:
            move_card(ctx, k)
        frame(ctx, MC.orbit(cam, float(k)))
        ctx.temporal_frame(prm, reset=k == 0, render_features=False, moving=moving)
        got = ctx.read_temporal()
        want = chain.step(ctx, card_table(k), card_table(k - 1) if k else None, moving=moving, reset=k == 0)
        if moving:
            want, wm = want
            assert same_all(ctx.read_motion(), wm), k
        assert same_all(got, want), (k, where_differ(got, want))
        if k:
            # the card has history only where the call followed it
            card = card_pixels(ctx)
            assert (chain.found[card].mean() > 0.5) == moving, (k, float(chain.found[card].mean()))
            assert chain.found[~card].sum() > 1000


def test_reset_and_a_resolution_change_drop_the_history(ctx):
    from pbrpathtracer_amd import ptk
    arrays, _, _ = MC.quality_scene()
    cam = MC.QUALITY_CAM
    w, h = 96, 54
    stage(ctx, arrays, cam, w, h)
    prm = ptk.temporal_defaults(MC.EXTENT)
    chain = Chain(prm)
    for k in range(2):
        if k:
            move_card(ctx, k)
        frame(ctx, MC.orbit(cam, float(k)))
        ctx.temporal_frame(prm, reset=k == 0, render_features=False, moving=True)
        want, wm = chain.step(ctx, card_table(k), card_table(k - 1) if k else None, reset=k == 0)
        got = ctx.read_temporal()
        assert same_all(got, want) and same_all(ctx.read_motion(), wm)
    cur = current_of(ctx)
    assert not np.array_equal(got[0], cur[0])
    ctx.temporal_frame(prm, reset=True, render_features=False, moving=True)
    want, wm = chain.step(ctx, card_table(1), card_table(0), reset=True)
    got, gm = ctx.read_temporal(), ctx.read_motion()
    assert same_all(got, want) and same_all(got, cur[:2])
    # (no history: no view to take motion vectors under; X' and n' are computed all the same)
    assert same_all(gm, wm) and np.isnan(gm[2]).all() and not np.array_equal(gm[0], cur[3])
    # ... and the call after it has that frame for its history
    move_card(ctx, 2)
    frame(ctx, MC.orbit(cam, 2.0))
    ctx.temporal_frame(prm, render_features=False, moving=True)
    want, wm = chain.step(ctx, card_table(2), card_table(1))
    got = ctx.read_temporal()
    assert same_all(got, want) and (got[1][chain.found] == 8.0).all() and chain.found.any()
    # another resolution: nothing to read, and the next call starts over
    ctx.set_frame(48, 32, 4)
    buf = np.full((32, 48, 3), 7.25, f32)
    assert ctx.L.ptk_read_motion(ctx.h, buf.ctypes.data, None, None) == BAD_ARG and (buf == 7.25).all()
    assert ctx.L.ptk_motion_device_ptr(ctx.h, None, None, None, None) == BAD_ARG
    assert ctx.L.ptk_temporal_frame_moving(ctx.h, C.byref(prm), 0) == BAD_ARG      # (no feature planes at this resolution yet)
    assert ctx.L.ptk_render_motion(ctx.h, None) == BAD_ARG
    frame(ctx, MC.orbit(cam, 2.0))
    ctx.temporal_frame(prm, render_features=False, moving=True)
    got = ctx.read_temporal()
    assert got[0].shape == (32, 48, 3) and same_all(got, current_of(ctx)[:2]) and np.isnan(ctx.read_motion()[2]).all()


# ---- what the calls leave alone -------------------------------------------------------------------------------------------------------
def test_frame_state_is_left_alone(ctx):
    import torch
    from pbrpathtracer_amd import ptk
    arrays, first, n = MC.quality_scene()
    cam = MC.QUALITY_CAM
    w, h = 96, 54
    stage(ctx, arrays, cam, w, h)
    prm = ptk.temporal_defaults(MC.EXTENT)
    mask = masks()[1] | (1 << ptk.FEAT_ALBEDO) | (1 << ptk.FEAT_EMISSION)
    case = TR.random_case(w, h, seed=3)
    primed = MC.primed_planes(case["current"], 3, case["extent"])
    dev = torch.device("cuda", ctx.device_ordinal())
    tplanes = [[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in planes] for planes in (case["current"], primed, case["history"])]

    def state(adaptive):
        s = dict(accum=ctx.read_accum(), rgb8=ctx.resolve_rgb8(), samples=np.array(ctx.samples()), denoised=ctx.read_denoised())
        s.update({nm: ctx.read_feature(k) for k, nm in enumerate(ptk.FEAT_NAMES) if (mask >> k) & 1})
        if adaptive:
            s.update(counts=ctx.read_sample_counts(), moments=ctx.read_moments())
        return s

    def the_four_entries():
        ctx.snapshot_geometry()
        ctx.render_motion(ctx.get_view())
        ctx.read_motion()
        ctx.reproject_planes_moving(case["hist_view"], case["current"], primed[0], primed[1], case["history"], TR.params(0.05))
        ctx.reproject_planes_moving(case["hist_view"], tplanes[0], tplanes[1][0], tplanes[1][1], tplanes[2], TR.params(0.05))
        for _ in range(2):
            ctx.temporal_frame(prm, render_features=False, moving=True)
            ctx.read_temporal()

    ctx.render(0, 8, SEED)
    ctx.render_features(mask, 0, SEED)
    ctx.denoise_frame(ptk.denoise_defaults(MC.EXTENT), render_features=False)
    before = state(False)
    the_four_entries()
    after = state(False)
    for k in before:
        assert same(before[k], after[k]), k
    ctx.render(8, 4, SEED)
    twelve = ctx.read_accum()
    ctx.reset(); ctx.render(0, 12, SEED)
    assert ctx.samples() == 12 and same(twelve, ctx.read_accum())
    ctx.render_adaptive(0.05, 8, 4, 24, SEED)
    ctx.render_features(mask, 0, SEED)
    ctx.denoise_frame(ptk.denoise_defaults(MC.EXTENT), render_features=False)
    before = state(True)
    the_four_entries()
    after = state(True)
    for k in before:
        assert same(before[k], after[k]), k
    # ptk_upload_scene drops the snapshot: the card has moved since it was taken, and after an upload nothing has
    ctx.update_geometry(first, MC.card_verts(3))
    ctx.render_features(mask, 0, SEED)
    ctx.render_motion(None)
    planes = four_planes(ctx)
    assert not np.array_equal(ctx.read_motion()[0], planes[2])
    ctx.upload_scene(dict(arrays, verts=card_table(3)))
    ctx.render_features(mask, 0, SEED)
    ctx.render_motion(None)
    pp, pn, _ = ctx.read_motion()
    planes = four_planes(ctx)
    assert card_pixels(ctx).sum() > 200
    assert np.array_equal(bits(pp), bits(planes[2])) and np.array_equal(bits(pn), bits(planes[3]))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import torch
    from pbrpathtracer_amd import ptk
    L = ctx.L
    w, h = 9, 7
    case = TR.random_case(w, h, 3)
    primed = MC.primed_planes(case["current"], 3, case["extent"])
    planes = [np.ascontiguousarray(a) for a in case["current"] + primed + case["history"]]
    out = np.full((h, w, 3), 7.25, f32); out_n = np.full((h, w), 7.25, f32)
    view = ptk._view(case["hist_view"])
    ptr = lambda a: None if a is None else a.ctypes.data
    good = TR.params(0.05)

    def planes_call(prm, ww=w, hh=h, drop=None, v=True, p=True, o=(out, out_n), c=ctx.h):
        a = [None if k == drop else ptr(x) for k, x in enumerate(planes)]
        return L.ptk_reproject_planes_moving(c, ww, hh, C.byref(view) if v else None, *a, C.byref(prm) if p else None, ptr(o[0]), ptr(o[1]))

    # the frame entry's history and the motion planes, which refused calls must leave as they are
    arrays, _, _ = MC.quality_scene()
    cam = MC.QUALITY_CAM
    stage(ctx, arrays, cam, 48, 32)
    fprm = ptk.temporal_defaults(MC.EXTENT)
    chain = Chain(fprm)
    frame(ctx, cam)
    ctx.temporal_frame(fprm, reset=True, render_features=False, moving=True)
    kept, kept_motion = chain.step(ctx, card_table(0), None, reset=True)
    assert same_all(ctx.read_temporal(), kept) and same_all(ctx.read_motion(), kept_motion)
    move_card(ctx, 1)
    for bad in (dict(max_plane_dist=0.0), dict(max_plane_dist=float("nan")), dict(min_normal_dot=1.5), dict(max_history=0.5),
                dict(max_history=float("inf"))):
        prm = ptk._temporal_params(dict(good, **bad))
        assert planes_call(prm) == BAD_ARG, bad
        assert L.ptk_temporal_frame_moving(ctx.h, C.byref(prm), 0) == BAD_ARG, bad
    prm = ptk._temporal_params(good)
    assert planes_call(prm, ww=-1) == BAD_ARG and planes_call(prm, hh=-1) == BAD_ARG
    assert planes_call(prm, v=False) == BAD_ARG and planes_call(prm, p=False) == BAD_ARG and planes_call(prm, c=None) == BAD_ARG
    for k in range(12):
        assert planes_call(prm, drop=k) == BAD_ARG, k
    assert planes_call(prm, o=(None, out_n)) == BAD_ARG and planes_call(prm, o=(out, None)) == BAD_ARG
    assert (out == 7.25).all() and (out_n == 7.25).all()
    # the device entry refuses alike
    dev = torch.device("cuda", ctx.device_ordinal())
    d_out = torch.full((h, w, 3), 7.25, device=dev); d_n = torch.full((h, w), 7.25, device=dev)
    t = [torch.from_numpy(a).to(dev) for a in planes]
    dp = lambda x: C.c_void_p(x.data_ptr())
    bad = ptk._temporal_params(dict(good, max_history=0.0))
    entry = L.ptk_reproject_planes_moving_device
    assert entry(ctx.h, w, h, C.byref(view), *map(dp, t), C.byref(bad), dp(d_out), dp(d_n)) == BAD_ARG
    assert entry(ctx.h, w, h, None, *map(dp, t), C.byref(prm), dp(d_out), dp(d_n)) == BAD_ARG
    assert entry(ctx.h, w, h, C.byref(view), *map(dp, t[:5]), None, *map(dp, t[6:]), C.byref(prm), dp(d_out), dp(d_n)) == BAD_ARG
    assert entry(ctx.h, w, h, C.byref(view), *map(dp, t), C.byref(prm), None, dp(d_n)) == BAD_ARG
    ctx.synchronize()
    assert (d_out == 7.25).all().item() and (d_n == 7.25).all().item()
    # frame entry: unknown flag bits, null params, null context
    assert L.ptk_temporal_frame_moving(ctx.h, C.byref(fprm), 2) == BAD_ARG
    assert L.ptk_temporal_frame_moving(ctx.h, C.byref(fprm), 0x80000001) == BAD_ARG
    assert L.ptk_temporal_frame_moving(ctx.h, None, 0) == BAD_ARG and L.ptk_temporal_frame_moving(None, C.byref(fprm), 0) == BAD_ARG
    assert L.ptk_geometry_snapshot(None) == BAD_ARG and L.ptk_render_motion(None, None) == BAD_ARG
    assert L.ptk_read_motion(None, None, None, None) == BAD_ARG and L.ptk_motion_device_ptr(None, None, None, None, None) == BAD_ARG
    assert L.ptk_last_motion_ms(None, None, None) == BAD_ARG
    # a missing guide plane, each of the five in turn
    _, five = masks()
    for k in (ptk.FEAT_MATERIAL, ptk.FEAT_TRIANGLE, ptk.FEAT_BARY, ptk.FEAT_POSITION, ptk.FEAT_NORMAL):
        ctx.render_features(five & ~(1 << k), 0, SEED)
        assert L.ptk_temporal_frame_moving(ctx.h, C.byref(fprm), 0) == BAD_ARG, k
        if k != ptk.FEAT_MATERIAL:
            assert L.ptk_render_motion(ctx.h, None) == BAD_ARG, k
    assert same_all(ctx.read_temporal(), kept) and same_all(ctx.read_motion(), kept_motion)
    buf = [np.full((32, 48, 3), 7.25, f32), np.full((32, 48, 3), 7.25, f32), np.full((32, 48, 2), 7.25, f32)]
    # ... and the history and the snapshot are as they were: the next good call follows the card and blends
    frame(ctx, MC.orbit(cam, 1.0))
    assert L.ptk_temporal_frame_moving(ctx.h, C.byref(fprm), 0) == ptk.PTK_OK
    want, wm = chain.step(ctx, card_table(1), card_table(0))
    assert same_all(ctx.read_temporal(), want) and same_all(ctx.read_motion(), wm)
    assert chain.found[card_pixels(ctx)].mean() > 0.5
    # a stale resolution
    ctx.set_frame(40, 24, 4)
    assert L.ptk_temporal_frame_moving(ctx.h, C.byref(fprm), 0) == BAD_ARG and L.ptk_render_motion(ctx.h, None) == BAD_ARG
    assert L.ptk_read_motion(ctx.h, *(b.ctypes.data for b in buf)) == BAD_ARG and all((b == 7.25).all() for b in buf)
    # a context without a scene, then without a frame, then without planes
    c2 = ptk.Context(0)
    try:
        assert c2.L.ptk_geometry_snapshot(c2.h) == BAD_ARG                          # before ptk_upload_scene
        assert c2.L.ptk_render_motion(c2.h, None) == BAD_ARG
        assert c2.L.ptk_temporal_frame_moving(c2.h, C.byref(fprm), 0) == BAD_ARG
        c2.upload_scene(arrays); c2.set_camera(**cam)
        assert c2.L.ptk_geometry_snapshot(c2.h) == ptk.PTK_OK
        assert c2.L.ptk_render_motion(c2.h, None) == BAD_ARG                        # no frame
        assert c2.L.ptk_temporal_frame_moving(c2.h, C.byref(fprm), 0) == BAD_ARG
        c2.set_frame(48, 32, 4)
        assert c2.L.ptk_render_motion(c2.h, None) == BAD_ARG                        # no feature planes
        assert c2.L.ptk_temporal_frame_moving(c2.h, C.byref(fprm), 0) == BAD_ARG
        assert c2.L.ptk_read_motion(c2.h, *(b.ctypes.data for b in buf)) == BAD_ARG and all((b == 7.25).all() for b in buf)
        # a scene without triangles: PTK_OK, nothing to keep
        empty = {k: (np.asarray(v)[:0].copy() if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material") else np.asarray(v).copy())
                 for k, v in arrays.items()}
        empty["lights"] = np.zeros(0, np.int32)
        c2.upload_scene(empty)
        assert c2.L.ptk_geometry_snapshot(c2.h) == ptk.PTK_OK
        # the planes entry needs no scene, no camera and no frame
        c3 = ptk.Context(0)
        got = c3.reproject_planes_moving(case["hist_view"], case["current"], primed[0], primed[1], case["history"], good)
        c3.close()
        assert same_all(got, MR.reproject_moving(case["hist_view"], case["current"], primed[0], primed[1], case["history"], good))
    finally:
        c2.close()


# ---- the host class and the command line ----------------------------------------------------------------------------------------------
def test_host_class_tracks_motion(tmp_path):
    """TrackMotion(true) with two batches of SetObjectTransform before one TemporalFrameMoving: one snapshot, taken ahead of the first
    batch - the result equals the mirror's for (geometry of the last temporal call, geometry now), and the context-level
    sequence snapshot, update, update"""
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer, camera_from_scene
    pts, scene, _ = S.build_config("C1", str(tmp_path), width=W, height=H, depth=4)
    pt = PathTracer(device=0)
    pt.LoadSceneFile(pts)
    pt.SetSeed(3)
    pt.TrackMotion(True)
    c = pt.context()
    staged0 = pt.StagedScene()
    prm = ptk.temporal_defaults(extent_of(staged0))
    chain = Chain(prm)
    cam = camera_from_scene(scene)
    base = pt.GetObjectTransform(0)
    pt.ResetImage(); pt.RenderFrames(4)
    pt.TemporalFrameMoving(reset=True)
    want, wm = chain.step(c, staged0["verts"], None, reset=True)
    assert same_all(pt.ReadTemporal(), want) and same_all(pt.ReadMotion(), wm)

    def shifted(dx, dy):
        M = base.copy(); M[3][:3] += np.array([dx, dy, 0.0], f32)
        return M

    pt.SetObjectTransform(0, shifted(0.3, 0.0))
    pt.Pick(0, 0)                                   # a render call applies the first batch ...
    staged1 = pt.StagedScene()
    pt.SetObjectTransform(0, shifted(0.05, 0.04))
    pt.ResetImage(); pt.RenderFrames(4)             # ... and this one the second
    staged2 = pt.StagedScene()
    assert c.geometry_info()["updates"] == 2 and not np.array_equal(staged1["verts"], staged2["verts"])
    pt.TemporalFrameMoving()
    got, gm = pt.ReadTemporal(), pt.ReadMotion()
    want, wm = chain.step(c, staged2["verts"], staged0["verts"])
    assert same_all(got, want), where_differ(got, want)
    assert same_all(gm, wm), where_differ(gm, wm)
    assert pt.GetSamples() == 4 and pt.LastError() == ""
    hit = c.read_feature(ptk.FEAT_TRIANGLE) >= 0
    assert chain.found.sum() > 0.5 * hit.sum() and np.isfinite(gm[2][hit]).all() and np.abs(gm[2][hit]).max() > 0.5
    assert not same_all(gm[:2], MR.render_motion(None, four_planes(c), staged2["verts"], staged1["verts"])[:2])
    # the context-level sequence with a single snapshot
    b = ptk.Context(0)
    try:
        stage(b, staged0, cam)
        b.render(0, 4, 3); b.render_features(masks()[1], 0, 3)
        b.temporal_frame(prm, reset=True, render_features=False, moving=True)
        b.snapshot_geometry()
        for s in (staged1, staged2):
            b.update_geometry(0, s["verts"], s["normals"], s["tbn"])
        b.reset(); b.render(0, 4, 3); b.render_features(masks()[1], 0, 3)
        b.temporal_frame(prm, render_features=False, moving=True)
        assert same_all(b.read_temporal(), got) and same_all(b.read_motion(), gm)
    finally:
        b.close()
    # nothing moved since the last temporal call: the old snapshot is not this history's
    pt.ResetImage(); pt.RenderFrames(4)
    pt.TemporalFrameMoving()
    want, wm = chain.step(c, staged2["verts"], None)
    assert same_all(pt.ReadTemporal(), want) and same_all(pt.ReadMotion(), wm)
    assert np.array_equal(bits(pt.ReadMotion()[0]), bits(c.read_feature(ptk.FEAT_POSITION)))


def test_command_line_moves_an_object(tmp_path):
    from pbrpathtracer_amd import render, scenes as S
    pts, _, _ = S.build_config("C1", str(tmp_path), width=W, height=H, depth=4)
    png, npy, mv = (str(tmp_path / n) for n in ("out.png", "out.npy", "motion.npy"))
    rc = render.main([pts, "--orbit", "3", "--orbit-degrees", "3", "--spp", "2", "--temporal", "--move-object", "0", "--move-by", "0.2", "0.1", "0",
                      "-o", png, "--npy", npy, "--motion-vectors", mv])
    assert rc == 0 and os.path.getsize(png) > 0
    image, motion = np.load(npy), np.load(mv)
    assert image.shape == (H, W, 3) and image.dtype == f32 and np.isfinite(image).all()
    assert motion.shape == (H, W, 2) and motion.dtype == f32
    finite = np.isfinite(motion).all(axis=-1)
    assert finite.sum() > 500 and np.abs(motion[finite]).max() > 0.5
    # the options go together
    assert render.main([pts, "--orbit", "2", "--move-object", "0"]) == 1
    assert render.main([pts, "--orbit", "2", "--temporal", "--motion-vectors", mv]) == 1
    assert render.main([pts, "--orbit", "2", "--spp", "1", "--temporal", "--move-object", "7", "--move-by", "0", "0", "0", "-o", png]) == 1


# ---- the feature does its job ---------------------------------------------------------------------------------------------------------
def test_a_sliding_card_keeps_its_history(ctx):
    """The scene of tests/test_motion_cpu.py's check (motion_cases.quality_scene): a striped, tilted card slides through the Cornell box
    by 1/50 of the extent per frame for 8 frames at 4 spp.  Over the card's pixels in the last frame, against a 4096-spp render of the
    final state: moving mode is less noisy than the plain last frame and than ptk_temporal_frame without reset, finds history on at
    least half of the card's pixels, and on more of them than ptk_temporal_frame does.  Orderings, not tuned numbers.
    (Measured on an MI355X: see DESIGN.md 4.20.)"""
    from pbrpathtracer_amd import ptk
    arrays, first, n = MC.quality_scene()
    cam = MC.QUALITY_CAM
    prm = ptk.temporal_defaults(MC.EXTENT)
    stale = ptk.Context(0)
    try:
        for c in (ctx, stale):
            stage(c, arrays, cam, W, H, MC.QUALITY_DEPTH)
        for k in range(MC.FRAMES):
            for c, moving in ((ctx, True), (stale, False)):
                if k:
                    move_card(c, k)
                frame(c, cam, MC.QUALITY_SPP, MC.QUALITY_SEED + k)
                c.temporal_frame(prm, reset=k == 0, render_features=False, moving=moving)
        got_m, n_m = ctx.read_temporal()
        got_s, n_s = stale.read_temporal()
    finally:
        stale.close()
    plain = current_of(ctx)[0]
    card = card_pixels(ctx)
    ctx.reset(); ctx.render(0, 4096, 999)
    truth = (ctx.read_accum() / f32(4096)).astype(f32)
    rmse = lambda a: float(np.sqrt(np.mean((a[card].astype(np.float64) - truth[card]) ** 2)))
    found_m = float((n_m[card] > MC.QUALITY_SPP).mean()); found_s = float((n_s[card] > MC.QUALITY_SPP).mean())
    print("sliding card: RMSE plain %.4f, moving %.4f (ratio %.3f), stale %.4f (ratio %.3f); found history: moving %.3f, stale %.3f; card pixels %d"
          % (rmse(plain), rmse(got_m), rmse(got_m) / rmse(plain), rmse(got_s), rmse(got_m) / rmse(got_s), found_m, found_s, int(card.sum())))
    assert card.sum() >= 100
    assert rmse(got_m) < rmse(plain)
    assert rmse(got_m) < rmse(got_s)
    assert found_m >= 0.5
    assert found_s < found_m
