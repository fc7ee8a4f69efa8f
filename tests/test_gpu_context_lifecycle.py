"""What a context owns and what its last-call timers remember (pbrpathtracer_amd/csrc/ptk_own.h, ptk_ctx.h).

1. Every last_*_ms of a context that has a scene and a frame but has made no query reads zero and raises nothing.
2. The timed state of the query entries: after a call of 64 rays or points the time reads finite and above zero; a call of count 0
   behind it - legal, with nothing to do - returns before the entry touches its timer, so the entry goes on reading the time of
   the call before, bit for bit.
3. No context leaks its device buffers: the device memory in use (torch.cuda.mem_get_info) after 12 contexts, each created, used
   and closed, is within 64 MiB of what it was after one warm-up context.  A memory reading cannot see a small leak, so a context
   sizes its work to make every buffer below at least 8 MiB: one of them leaked per context shows as 96 MiB or more.

   Frame 1024 x 768 (786432 pixels), 1 spp, depth 1:
     temporal history 112 B/px = 84 MiB; temporal moments 52 B/px = 39 MiB; the a-trous images 64 B/px = 48 MiB; motion planes
     32 B/px = 24 MiB; denoised frame 12 B/px = 9 MiB; adaptive S2 12 B/px = 9 MiB; each three-channel feature plane 12 B/px =
     9 MiB; primary table, hit cache and directions 16 B/px = 12 MiB each; accumulator 12 B/px = 9 MiB; each sample buffer of a
     render at least 16 B/px = 12 MiB; the upsample call's packed low image 64 B/px = 48 MiB.
   Guides 2048 x 1536 (3145728 pixels): primary table 16 B/px = 48 MiB; three-channel planes 12 B/px = 36 MiB each; material plane
     4 B/px = 12 MiB; upsampled result 16 B/px = 48 MiB.
   2^19 rays at 1 spp (then an adaptive query of 2 spp): ray sample buffer 16 B per ray-sample, a chunk of slots per ray, at least
     8 MiB; adaptive buffer 56 B/ray = 28 MiB.
   Lightmap 2048 x 1024 (2097152 texels) with one dilation pass: owner plane 4 B/texel = 8 MiB; dilation image and plane
     16 B/texel = 32 MiB; compacted rays 44 B per covered texel.
   2048 probes x 1024 directions (2097152 rays), tables kept in the context: ray block 24 B/ray = 48 MiB; radiance table 12 B/ray =
     24 MiB; depth table 4 B/ray = 8 MiB.

   Too small for a memory reading to see, and held by the structure of ptk_ctx alone (every member an owner, ptk_destroy frees
   nothing by hand): the one- and two-channel feature planes (3 - 6 MiB), the adaptive counts (3 MiB), the 8-bit images (2.25 MiB),
   the closest-point counters, the display histogram, the probes' basis table, the surface table and the refit tables of a
   32-triangle scene, the geometry staging buffer, the live and adaptive quadrant lists, the queue blocks, the page-locked words,
   the streams, and all events."""
import numpy as np
import pytest

import ray_cases as RC

pytestmark = pytest.mark.gpu

MiB = float(2 ** 20)
LAST = ("rays", "hits", "closest", "crossings", "multihit", "surface", "denoise", "display", "upsample", "temporal", "motion", "variance",
        "bake", "rays_adaptive", "probes", "probe_visibility")


def cornell(c, w, h, depth):
    arrays, cam = RC.scene("s_cornell")
    c.upload_scene(arrays); c.set_camera(**cam); c.set_frame(w, h, depth)
    return arrays, cam


def values(got):
    if isinstance(got, dict):
        got = tuple(got.values())
    return np.atleast_1d(np.asarray(got, np.float64))


def extent_of(arrays):
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


@pytest.fixture(scope="module")
def fresh():
    """a scene and a frame, no query yet; the tests of part 1 only read it"""
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    cornell(c, 48, 32, 1)
    yield c
    c.close()


@pytest.mark.parametrize("name", LAST)
def test_last_ms_before_any_call_reads_zero(fresh, name):
    got = values(getattr(fresh, f"last_{name}_ms")())
    print(name, got)
    assert len(got) >= 1 and np.array_equal(got, np.zeros_like(got)), (name, got)


@pytest.mark.parametrize("name", ("hits", "closest", "crossings", "multihit"))
def test_last_ms_after_a_call_and_after_an_empty_call(name):
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    try:
        arrays, _ = cornell(c, 48, 32, 1)
        ro, rd = RC.rays_in_box(arrays, 64, 5)
        L, h = c.L, c.h
        i32, f32 = np.zeros(16, np.int32), np.zeros(16, np.float32)
        i8 = np.zeros(16, np.int8)
        p = lambda a: a.ctypes.data
        if name == "hits":
            c.intersect_rays(ro, rd)
            empty = lambda: L.ptk_intersect_rays(h, 0, None, None, 0, 0, 0, p(i32), p(f32), p(f32), p(i32))
        elif name == "closest":
            c.closest_points(ro)
            empty = lambda: L.ptk_closest_points(h, 0, None, None, p(i32), p(f32), p(f32), p(f32))
        elif name == "crossings":
            c.crossings_rays(ro, rd)
            empty = lambda: L.ptk_crossings_rays(h, 0, None, None, None, p(i32), p(i32))
        else:
            c.multihit_rays(ro, rd, 4)
            empty = lambda: L.ptk_multihit_rays(h, 0, None, None, None, 4, p(i32), p(i32), p(f32), p(f32), p(i8))
        last = getattr(c, f"last_{name}_ms")
        t = last()
        print(name, "after 64:", t)
        assert np.isfinite(t) and t > 0.0, (name, t)
        assert empty() == ptk.PTK_OK
        t0 = last()
        print(name, "after 0:", t0)
        # (the empty call returns ahead of the timer: the entry still reads the call before it, from the same two events)
        assert t0 == t, (name, t, t0)
    finally:
        c.close()


def use_everything(k):
    """one context: created, one call of each family at the sizes of the docstring, closed; returns the device memory in use (MiB)
    just before it closes"""
    import torch
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    try:
        arrays, _ = cornell(c, 1024, 768, 1)
        ext = extent_of(arrays)
        dev = torch.device("cuda", c.device_ordinal())
        c.render(0, 1, 3 + k)
        c.render_adaptive(0.5, 2, 2, 2, 3 + k)
        c.denoise_frame(ptk.denoise_defaults(ext))
        c.snapshot_geometry()
        c.update_geometry(0, np.asarray(arrays["verts"], np.float32).reshape(-1, 9)[:1])
        c.temporal_frame(ptk.temporal_defaults(ext), moving=True, moments=True)
        c.temporal_variance(ptk.variance_defaults(ext))
        c.render_motion(c.get_view())
        c.display_frame()
        c.render_guides(2048, 1536)
        c.upsample_frame(ptk.UPSAMPLE_ACCUM, ptk.upsample_defaults(ext))
        ro, rd = (torch.from_numpy(a).to(dev) for a in RC.rays_in_box(arrays, 1 << 19, 7))
        c.trace_rays(ro, rd, 1, 0, 1, 5)
        c.trace_rays_adaptive(ro, rd, 1, 0.5, 2, 2, 2, 5)
        img, owner = c.bake_lightmap(2048, 1024, 1e-3, 1, 0, 1, 5, device=True)
        c.dilate_lightmap(img, owner, 1)
        rng = np.random.default_rng(11)
        v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
        pos = torch.from_numpy(rng.uniform(v.min(axis=0), v.max(axis=0), (2048, 3)).astype(np.float32)).to(dev)
        c.bake_probes(pos, rd[:1024].contiguous(), 1, 0, 1, 5, 1.0, want_radiance=False)
        c.bake_probe_visibility(pos, rd[:1024].contiguous(), 4, 2.0 * ext, want_depth=False)
        c.sample_surface(1 << 19, seed=5, device=True)
        c.synchronize()
        free, total = torch.cuda.mem_get_info(0)
        return (total - free) / MiB
    finally:
        c.close()


def test_contexts_give_their_device_memory_back():
    import torch
    torch.cuda.init()

    def used():
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        free, total = torch.cuda.mem_get_info(0)
        return (total - free) / MiB

    before = used()
    use_everything(0)                   # (first use of every path: code objects, the runtime's pools, torch's allocator)
    base = used()
    held = [use_everything(1 + k) - base for k in range(12)]
    end = used()
    print(f"device memory in use: {before:.0f} MiB before, {base:.0f} MiB behind the warm-up context, {end:.0f} MiB behind 12 more; "
          f"a context held {min(held):.0f} .. {max(held):.0f} MiB at its end")
    # (the buffers of the docstring add up to 729 MiB, with four three-channel feature planes and two sample buffers: a context
    # that held less did not make them, and the reading below would say nothing)
    assert min(held) > 729.0, held
    assert end - base < 64.0, (base, end)
