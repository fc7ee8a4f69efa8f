"""The host contract around the kernels (include/ptk.h), bit for bit against the CPU oracle: resuming
from a saved accumulator (ptk_write_accum), renders ordered on a caller's stream with no host wait (ptk_set_stream), the
device-resident views (ptk_accum_device_ptr, ptk_rgb8_device_ptr, ptk_gathered_device_ptr) and the scheduling options that
"only tune scheduling, never a result".  Per-sample values of adaptive renders come from tests/adaptive_rule.py."""
import ctypes as C

import numpy as np
import pytest

import adaptive_rule as AR
from conftest import load_golden, scene_from_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def _scene(kind, aperture=None):
    """(arrays, camera, depth): a golden scene ("s_cornell", ...; aperture None = the scene's own) or a random_scene by tree kind."""
    if kind.startswith("s_"):
        z = load_golden(f"tier_{kind}.npz")
        cam, proj = z["cam"], z["proj"]
        return scene_from_golden(z), dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]),
                                          focal_dist=float(z["focal_dist"]),
                                          aperture=float(z["aperture"]) if aperture is None else aperture), int(z["depth"])
    from test_gpu_random_scenes import random_scene
    seed, n = {"flat": (12, 16), "host_bvh": (14, 300), "device_bvh": (16, 6000), "bvh_1500": (18, 1500)}[kind]
    arrays, cam = random_scene(seed, n, True)
    return arrays, cam, 5


class _Oracle:
    def __init__(self, oracle_mod, arrays, cam):
        self.o = oracle_mod.Oracle(arrays)
        self.cam = self.camera(oracle_mod, cam)

    @staticmethod
    def camera(oracle_mod, cam):
        return oracle_mod.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])

    def render(self, W, H, D, first, spp, seed, total=None, cam=None, rank=0, world=1):
        """(accumulator, 8-bit image) after adding samples [first, first + spp) to `total` (zeros if None; not modified)."""
        t = np.zeros((H, W, 3), np.float32) if total is None else np.array(total, np.float32, copy=True)
        return self.o.render(self.cam if cam is None else cam, W, H, D, first, spp, seed, total=t, rank=rank, world=world)

    def close(self):
        self.o.close()


def _setup(c, arrays, cam, W, H, D):
    c.upload_scene(arrays); c.set_camera(**cam); c.set_frame(W, H, D); c.set_tile(0, 1); c.reset()


def _hip():
    """The HIP runtime this process already has loaded (torch's copy, which libptk.so shares: tests/conftest.py)."""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln)
    L = C.CDLL(path)
    L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.hipStreamSynchronize.argtypes = [C.c_void_p]
    return L


def _read_device(ptr, shape, dtype, stream=None):
    """Copy device memory to the host on `stream` (a HIP stream handle; None = the null stream) and wait for it."""
    out = np.empty(shape, dtype)
    L = _hip()
    assert L.hipMemcpyAsync(out.ctypes.data, ptr, out.nbytes, 2, stream) == 0        # hipMemcpyDeviceToHost
    assert L.hipStreamSynchronize(stream) == 0
    return out


# ---- 1. resume from a saved accumulator (ptk_write_accum) -----------------------------------------------------------------------

@pytest.mark.parametrize("kind,aperture,W,H", [("s_cornell", 0.0, 70, 50), ("s_cornell", 0.06, 61, 45), ("s_glass", 0.0, 53, 37),
                                               ("s_opacity", None, 48, 40), ("host_bvh", None, 40, 29), ("device_bvh", None, 40, 32)])
def test_write_accum_resumes_a_split_render(oracle_mod, kind, aperture, W, H):
    """The oracle's accumulator of samples [0, k) written into a fresh context, then render(k, m): the oracle's [0, k + m),
    float and 8-bit.  Pinhole cameras run with the primary-hit cache, thin-lens ones with the lens cull."""
    from pbrpathtracer_amd import ptk
    arrays, cam, D = _scene(kind, aperture)
    k, m, seed = 5, 6, 21
    o = _Oracle(oracle_mod, arrays, cam)
    first, _ = o.render(W, H, D, 0, k, seed)
    ref, ref8 = o.render(W, H, D, 0, k + m, seed)
    o.close()
    assert (first != 0).any(axis=2).mean() > 0.2
    c = ptk.Context(0)
    try:
        c.upload_scene(arrays); c.set_camera(**cam); c.set_frame(W, H, D)
        c.write_accum(first, k)
        assert c.samples() == k
        assert np.array_equal(c.read_accum(), first)
        c.render(k, m, seed)
        assert c.samples() == k + m
        got = c.read_accum()
        assert np.array_equal(got, ref), (kind, float(np.abs(got - ref).max()))
        assert np.array_equal(c.resolve_rgb8(), ref8)
        assert (c.read_sample_counts() == k + m).all()
    finally:
        c.close()


@pytest.mark.parametrize("aperture", [0.0, 0.06])
def test_written_light_stays_where_the_next_render_traces_nothing(ctx, oracle_mod, aperture):
    """An accumulator rendered from one camera, written back under a camera that has moved: the pixels that are now sure misses
    (pinhole, cached camera hits) or lens-culled (thin lens) are never traced, keep the written light unchanged and resolve to
    written / (k + m) (pathtracer.cpp:802-812) - through ptk_resolve_rgb8 and in a bound page-locked hand-off buffer.  Then the
    reverse: zeros written where that buffer shows light are black pixels that hold nothing, which the accumulate kernel skips
    unless the write asked for a full frame: the buffer must read 0 there after the next render."""
    from pbrpathtracer_amd import ptk
    arrays, cam, D = _scene("s_cornell", aperture)
    W, H, k, m, m2, seed = 64, 48, 4, 3, 2, 5
    cam2 = dict(cam); cam2["pos"] = np.array(cam["pos"], np.float32) + np.array([0.8, 0.3, 0.0], np.float32)
    o = _Oracle(oracle_mod, arrays, cam)
    ocam2 = _Oracle.camera(oracle_mod, cam2)
    written, _ = o.render(W, H, D, 0, k, seed)
    added, _ = o.render(W, H, D, k, m + m2, seed, cam=ocam2)                    # what camera 2 adds in both renders below
    ref, ref8 = o.render(W, H, D, k, m, seed, total=written, cam=ocam2)
    dark = (added == 0).all(axis=2) & (written != 0).any(axis=2)                  # lit before, nothing added now
    assert dark.sum() >= 100, "the camera move leaves too few lit pixels untraced: a poor test"
    written2 = ref.copy(); written2[dark] = 0.0                                   # the reverse case: zeros where the frame shows light
    ref2, ref2_8 = o.render(W, H, D, k + m, m2, seed, total=written2, cam=ocam2)
    o.close()
    _setup(ctx, arrays, cam, W, H, D)
    raw = ptk.load().ptk_host_alloc(W * H * 3)
    out = np.ctypeslib.as_array(C.cast(raw, C.POINTER(C.c_uint8)), shape=(H, W, 3))
    dev = np.zeros((H, W, 3), np.uint8)
    try:
        ctx.bind_out_image(out)
        ctx.set_camera(**cam2)
        ctx.write_accum(written, k)
        ctx.render(k, m, seed)
        got = ctx.read_accum()
        assert np.array_equal(got, ref)
        assert np.array_equal(got[dark], written[dark])
        ctx.resolve_rgb8(out)
        want8 = AR.resolve_rgb8(written, np.full((H, W), k + m, np.uint32))
        assert np.array_equal(out[dark], want8[dark]) and np.array_equal(out, ref8)
        ctx.L.ptk_resolve_rgb8(ctx.h, dev.ctypes.data)                            # (not the bound buffer: a copy of the device image)
        assert np.array_equal(dev, ref8)
        assert out[dark].any(), "the bound buffer shows no light in the untraced pixels: a poor test"
        ctx.write_accum(written2, k + m)
        ctx.render(k + m, m2, seed)
        ctx.resolve_rgb8(out)
        assert np.array_equal(ctx.read_accum(), ref2)
        assert not out[dark].any(), "the bound buffer still shows light the accumulator no longer holds"
        assert np.array_equal(out, ref2_8)
        ctx.L.ptk_resolve_rgb8(ctx.h, dev.ctypes.data)
        assert np.array_equal(dev, ref2_8)
    finally:
        ctx.bind_out_image(None)
        ptk.load().ptk_host_free(raw)


def test_write_accum_under_a_tile_split(ctx, oracle_mod):
    """set_tile(r, w): the owned pixels follow the fold from the written values, the others keep them."""
    arrays, cam, D = _scene("s_cornell", 0.0)
    W, H, k, m, seed = 70, 50, 3, 4, 8
    o = _Oracle(oracle_mod, arrays, cam)
    written, _ = o.render(W, H, D, 0, k, seed)
    full, _ = o.render(W, H, D, 0, k + m, seed)
    for rank, world in ((1, 3), (0, 2)):
        ref, _ = o.render(W, H, D, k, m, seed, total=written, rank=rank, world=world)
        _setup(ctx, arrays, cam, W, H, D); ctx.set_tile(rank, world)
        try:
            ctx.write_accum(written, k)
            ctx.render(k, m, seed)
            got = ctx.read_accum()
        finally:
            ctx.set_tile(0, 1)
        own = AR.owned_mask(W, H, rank, world)
        assert own.any() and (~own).any()
        assert np.array_equal(got, ref), (rank, world)
        assert np.array_equal(got[~own], written[~own])
        assert np.array_equal(got[own], full[own])
    o.close()


def test_write_accum_after_an_adaptive_render(ctx, oracle_mod):
    """After an adaptive render ptk_render is refused (the accumulator has no single sample count); ptk_write_accum makes it
    valid again and the split render is the oracle's."""
    from pbrpathtracer_amd import ptk
    arrays, cam, D = _scene("s_glass", 0.0)
    W, H, k, m, seed = 53, 37, 4, 4, 3
    o = _Oracle(oracle_mod, arrays, cam)
    first, _ = o.render(W, H, D, 0, k, seed)
    ref, ref8 = o.render(W, H, D, 0, k + m, seed)
    o.close()
    _setup(ctx, arrays, cam, W, H, D)
    ctx.render_adaptive(0.2, 4, 2, 8, seed)
    with pytest.raises(ptk.PtkError, match="adaptive"):
        ctx.render(8, 1, seed)
    ctx.write_accum(first, k)
    assert ctx.samples() == k
    ctx.render(k, m, seed)
    assert ctx.samples() == k + m
    assert np.array_equal(ctx.read_accum(), ref) and np.array_equal(ctx.resolve_rgb8(), ref8)
    assert (ctx.read_sample_counts() == k + m).all()


def test_write_accum_refusals(ctx):
    """Before ptk_set_frame and with samples < 0: an error, not a crash; a refused write leaves accumulator and count alone."""
    from pbrpathtracer_amd import ptk
    buf = np.ones((4, 4, 3), np.float32)
    fresh = ptk.Context(0)
    try:
        assert fresh.L.ptk_write_accum(fresh.h, buf.ctypes.data, 1) != 0
        assert b"set_frame" in fresh.L.ptk_last_error(fresh.h)
    finally:
        fresh.close()
    arrays, cam, D = _scene("s_cornell", 0.0)
    _setup(ctx, arrays, cam, 20, 12, D)
    ctx.render(0, 2, 1)
    before = ctx.read_accum()
    with pytest.raises(ptk.PtkError):
        ctx.write_accum(np.ones((12, 20, 3), np.float32), -1)
    assert ctx.samples() == 2 and np.array_equal(ctx.read_accum(), before)


def test_write_accum_writes_the_bound_accumulator(ctx, oracle_mod):
    """With a caller's accumulator bound (ptk_bind_accum), ptk_write_accum writes that one; the internal one is left alone."""
    import torch
    arrays, cam, D = _scene("s_cornell", 0.06)
    W, H, k, m, seed = 61, 45, 3, 3, 4
    o = _Oracle(oracle_mod, arrays, cam)
    first, _ = o.render(W, H, D, 0, k, seed)
    ref, ref8 = o.render(W, H, D, 0, k + m, seed)
    o.close()
    _setup(ctx, arrays, cam, W, H, D)
    ctx.render(0, 2, 99)
    internal = ctx.read_accum()
    t = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0"); torch.cuda.synchronize()
    try:
        ctx.bind_accum(t.data_ptr())
        ctx.write_accum(first, k)
        assert np.array_equal(t.cpu().numpy().reshape(H, W, 3), first)
        ctx.render(k, m, seed)
        ctx.synchronize()
        assert np.array_equal(t.cpu().numpy().reshape(H, W, 3), ref)
        assert np.array_equal(ctx.read_accum(), ref) and np.array_equal(ctx.resolve_rgb8(), ref8)
    finally:
        ctx.bind_accum(None)
    assert np.array_equal(ctx.read_accum(), internal)


# ---- 2. renders on a caller's stream (ptk_set_stream) ----------------------------------------------------------------------------

def test_caller_stream_sees_every_batch_in_order(oracle_mod):
    """A torch stream as the context's stream, a torch tensor as the accumulator: renders queued with no host wait, each followed
    by a clone of the tensor on the caller's stream; snapshot i must be the oracle's accumulator of every sample rendered so far -
    the accumulate kernels run on the caller's stream behind trace kernels on two alternating internal streams.  Halfway the
    context moves to a second caller stream, still without a host wait, right after the longest batch: the short batch that
    follows traces on the other internal stream and finishes first, but must add to the accumulator after it.  Then an adaptive
    render and a one-rank native gather on that stream; closing the context leaves the caller's streams alone."""
    import torch
    from pbrpathtracer_amd import ptk
    arrays, cam, D = _scene("s_cornell", 0.0)
    W, H, seed = 96, 64, 13
    spps = [1, 1, 1, 9, 1, 1, 1, 1]                          # batch i: samples [first[i], first[i] + spps[i])
    first, n, spp = np.concatenate([[0], np.cumsum(spps)[:-1]]).tolist(), len(spps), 2
    o = _Oracle(oracle_mod, arrays, cam)
    refs, acc = [], np.zeros((H, W, 3), np.float32)
    for i in range(n):
        acc, _ = o.render(W, H, D, first[i], spps[i], seed, total=acc)
        refs.append(acc)
    ref2, _ = o.render(W, H, D, 0, 2 * spp, seed)
    ref3, _ = o.render(W, H, D, 0, 3 * spp, seed)
    STEP, MIN_SPP, MAX_SPP, THR = 2, 4, 8, 0.2
    want = AR.adaptive(AR.oracle_samples(o.o, o.cam, W, H, D, MAX_SPP, seed), THR, MIN_SPP, STEP, MAX_SPP)
    o.close()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0"); torch.cuda.synchronize()
    c = ptk.Context(0)
    try:
        c.set_stream(s1.cuda_stream)
        _setup(c, arrays, cam, W, H, D)
        c.bind_accum(t.data_ptr())
        c.render(0, spp, seed); c.reset()                    # (the first render allocates its buffers, which waits)
        snaps = []
        for i in range(n):
            if i == n // 2:
                c.set_stream(s2.cuda_stream)
            c.render(first[i], spps[i], seed)
            with torch.cuda.stream(s1 if i < n // 2 else s2):
                snaps.append(t.clone())
        torch.cuda.synchronize()
        for i in range(n):
            assert np.array_equal(snaps[i].cpu().numpy().reshape(H, W, 3), refs[i]), i
        # an adaptive render and the exchange on the second caller stream
        r = c.render_adaptive(THR, MIN_SPP, STEP, MAX_SPP, seed)
        with torch.cuda.stream(s2):
            snap = t.clone()
        s2.synchronize()
        assert r["max_count"] == int(want["n"].max())
        assert np.array_equal(snap.cpu().numpy().reshape(H, W, 3), want["S1"])
        assert np.array_equal(c.read_sample_counts(), want["n"]) and np.array_equal(c.resolve_rgb8(), want["rgb8"])
        c.comm_init(ptk.comm_unique_id(), 0, 1)
        c.reset(); c.render(0, 2 * spp, seed)
        c.gather_accum(0)
        c.render(2 * spp, spp, seed)                         # queued at once: overlaps the exchange
        c.gather_wait()
        assert np.array_equal(c.read_gathered(), ref2)
        with torch.cuda.stream(s2):
            snap = t.clone()
        s2.synchronize()
        assert np.array_equal(snap.cpu().numpy().reshape(H, W, 3), ref3)
        c.comm_destroy()
    finally:
        c.close()
    # the caller's streams outlive the context
    for s in (s1, s2):
        with torch.cuda.stream(s):
            x = t * 2.0
        s.synchronize()
        assert torch.equal(x, t + t)


# ---- 3. device-resident views ----------------------------------------------------------------------------------------------------

def test_device_views_are_refused_before_set_frame():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    try:
        for view in (c.accum_device_ptr, c.rgb8_device_ptr, c.gathered_device_ptr):
            with pytest.raises(ptk.PtkError):
                view()
    finally:
        c.close()


def test_accum_device_ptr_is_the_accumulator(ctx, oracle_mod):
    """The internal accumulator's address, W*H*12 bytes, the same across renders and resets; the bound tensor's while one is
    bound; its contents are what ptk_read_accum returns."""
    import torch
    arrays, cam, D = _scene("s_opacity")
    W, H, spp, seed = 61, 45, 4, 6
    o = _Oracle(oracle_mod, arrays, cam)
    ref, _ = o.render(W, H, D, 0, spp, seed)
    o.close()
    _setup(ctx, arrays, cam, W, H, D)
    p, b = ctx.accum_device_ptr()
    assert p and b == W * H * 12
    ctx.render(0, spp, seed)
    ctx.synchronize()
    assert np.array_equal(_read_device(p, (H, W, 3), np.float32), ref)
    assert np.array_equal(ctx.read_accum(), ref)
    ctx.reset(); ctx.render(0, 1, seed)
    assert ctx.accum_device_ptr() == (p, b)
    t = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0"); torch.cuda.synchronize()
    try:
        ctx.bind_accum(t.data_ptr())
        assert ctx.accum_device_ptr() == (t.data_ptr(), b)
    finally:
        ctx.bind_accum(None)
    assert ctx.accum_device_ptr() == (p, b)


def test_rgb8_device_ptr_holds_the_resolved_frame(ctx, oracle_mod):
    """The device 8-bit image after a plain and after an adaptive render: ptk_resolve_rgb8's frame and the oracle's."""
    arrays, cam, D = _scene("s_cornell", 0.06)
    W, H, spp, seed = 53, 37, 6, 17
    STEP, MIN_SPP, MAX_SPP, THR = 2, 4, 8, 0.2
    o = _Oracle(oracle_mod, arrays, cam)
    _, ref8 = o.render(W, H, D, 0, spp, seed)
    want = AR.adaptive(AR.oracle_samples(o.o, o.cam, W, H, D, MAX_SPP, seed), THR, MIN_SPP, STEP, MAX_SPP)
    o.close()
    _setup(ctx, arrays, cam, W, H, D)
    p, b = ctx.rgb8_device_ptr()
    assert p and b == W * H * 3
    ctx.render(0, spp, seed)
    ctx.synchronize()
    img = _read_device(p, (H, W, 3), np.uint8)
    assert np.array_equal(img, ref8) and np.array_equal(img, ctx.resolve_rgb8())
    ctx.render_adaptive(THR, MIN_SPP, STEP, MAX_SPP, seed)
    assert ctx.rgb8_device_ptr() == (p, b)
    ctx.synchronize()
    img = _read_device(p, (H, W, 3), np.uint8)
    assert np.array_equal(img, want["rgb8"]) and np.array_equal(img, ctx.resolve_rgb8())
    assert np.array_equal(ctx.read_sample_counts(), want["n"])
    ctx.reset()


def test_gathered_device_ptr_holds_the_gathered_image(ctx, oracle_mod):
    """After a one-rank native gather and ptk_gather_wait the device view holds ptk_read_gathered's image; after ptk_set_frame
    with another resolution it is refused, as ptk_read_gathered is."""
    from pbrpathtracer_amd import ptk
    arrays, cam, D = _scene("host_bvh")
    W, H, spp, seed = 45, 38, 5, 2
    o = _Oracle(oracle_mod, arrays, cam)
    ref, _ = o.render(W, H, D, 0, spp, seed)
    o.close()
    _setup(ctx, arrays, cam, W, H, D)
    ctx.comm_init(ptk.comm_unique_id(), 0, 1)
    try:
        ctx.render(0, spp, seed)
        ctx.gather_accum(0)
        ctx.gather_wait()
        p, b = ctx.gathered_device_ptr()
        assert p and b == W * H * 12
        img = _read_device(p, (H, W, 3), np.float32)
        assert np.array_equal(img, ctx.read_gathered()) and np.array_equal(img, ref)
        ctx.set_frame(W + 16, H, D)
        with pytest.raises(ptk.PtkError, match="another resolution"):
            ctx.gathered_device_ptr()
        with pytest.raises(ptk.PtkError, match="another resolution"):
            ctx.read_gathered()
    finally:
        ctx.comm_destroy()


# ---- 4. scheduling options are never a result ------------------------------------------------------------------------------------

DEFAULTS = {"shade_threshold": 0, "gen_threshold": 16, "flat_shade_weight": 8, "flat_gen_weight": 64, "overlap": 1, "persistent": -1}
SCHEDULING = ([("shade_threshold", v) for v in (1, 8, 64, 4096)] + [("gen_threshold", v) for v in (0, 1, 64, 4096)] +
              [("flat_shade_weight", v) for v in (1, 4096)] + [("flat_gen_weight", v) for v in (1, 4096)] + [("overlap", 0)])


@pytest.mark.parametrize("kind,W,H", [("bvh_1500", 56, 40), ("s_cornell", 61, 45)])
def test_scheduling_options_never_change_the_image(ctx, oracle_mod, kind, W, H):
    """Every scheduling lambda and FLAT block weight at its extremes, and overlap off, one at a time under persistent 0 and 1:
    the oracle's image bit for bit (a BVH random scene with textures, and the 12-triangle Cornell box the FLAT kernel takes)."""
    arrays, cam, D = _scene(kind)
    spp, seed = 5, 31
    o = _Oracle(oracle_mod, arrays, cam)
    ref, ref8 = o.render(W, H, D, 0, spp, seed)
    o.close()
    _setup(ctx, arrays, cam, W, H, D)
    try:
        for persistent in (0, 1):
            ctx.set_option("persistent", persistent)
            for name, value in SCHEDULING:
                ctx.set_option(name, value)
                try:
                    ctx.reset(); ctx.render(0, spp, seed)
                    got = ctx.read_accum()
                    assert np.array_equal(got, ref), (kind, persistent, name, value, float(np.abs(got - ref).max()))
                    assert np.array_equal(ctx.resolve_rgb8(), ref8), (kind, persistent, name, value)
                finally:
                    ctx.set_option(name, DEFAULTS[name])
    finally:
        ctx.set_option("persistent", DEFAULTS["persistent"])


def test_register_out_image_writes_an_ordinary_buffer(ctx, oracle_mod):
    """register_out_image = 1: an ordinary (pageable) numpy buffer is page-locked in place and written by the accumulate kernel
    itself; every frame is the oracle's 8-bit image.  Unbound before the buffer goes."""
    arrays, cam, D = _scene("s_glass", 0.0)
    W, H, spp, seed, frames = 53, 37, 2, 9, 3
    o = _Oracle(oracle_mod, arrays, cam)
    refs8, acc = [], None
    for f in range(frames):
        acc, r8 = o.render(W, H, D, f * spp, spp, seed, total=acc)
        refs8.append(r8)
    o.close()
    _setup(ctx, arrays, cam, W, H, D)
    backing = np.full(W * H * 3 + 8192, 77, np.uint8)
    start = (-backing.ctypes.data) % 4096
    out = backing[start:start + W * H * 3].reshape(H, W, 3)                       # page-aligned, ordinary memory
    ctx.set_option("register_out_image", 1)
    try:
        ctx.bind_out_image(out)
        for f in range(frames):
            ctx.render(f * spp, spp, seed)
            ctx.synchronize()
            assert np.array_equal(out, refs8[f]), f                               # written by the kernel: no resolve yet
            ctx.resolve_rgb8(out)
            assert np.array_equal(out, refs8[f]), f
    finally:
        ctx.bind_out_image(None)
        ctx.set_option("register_out_image", 0)
