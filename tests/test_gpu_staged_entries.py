"""The host entries that stage their arrays through device memory (csrc/ptk_stage.h) against their `_device` twins, bit for bit: the
twin is fed torch tensors on the context's GPU, the host entry numpy arrays, and both must write the same bytes - for every
combination of optional outputs, with and without the *_ACCUMULATE load of the output, and at ray counts whose byte arrays end off a
16-byte boundary.  The host arrays of a call are cut from one slab filled with a guard byte, with a band of it around each: what a
call was not given - an optional array it got NULL for, the bands - must come back untouched.  What the twins compute is held to the
oracle and the mirrors elsewhere (test_gpu_rays, _hits, _bake, _probes, _rays_adaptive); the scene is the Cornell box of those tests."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bake_cases as BC
import probe_cases as PC
import ray_cases as RC
import rays_adaptive_rule as RA

pytestmark = pytest.mark.gpu

F32, I32, U32, U8 = np.float32, np.int32, np.uint32, np.uint8
N, DEPTH, SEED, SAMPLE, FIRST, SPP = 65, 4, (1 << 40) + 9, 3, 2, 4
W = H = 16
GUARD, BAND = 0xA5, 64


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    c.upload_scene(RC.scene("s_cornell")[0])
    yield c
    c.close()


@pytest.fixture(scope="module")
def rays():
    """(ro, rd) of N rays through the scene; shared, not to be modified"""
    return RC.rays_in_box(RC.scene("s_cornell")[0], N, 5)


@pytest.fixture(scope="module")
def uvs():
    return BC.grid_atlas(len(RC.scene("s_cornell")[0]["verts"]), W, H, 1)


class Slab:
    """Host arrays of one call, cut from one buffer of guard bytes."""

    def __init__(self, *specs):
        """specs: (shape, dtype) per array, in order"""
        self.spans, at = [], BAND
        for shape, dtype in specs:
            nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
            self.spans.append((at, nbytes))
            at = (at + nbytes + BAND + 63) // 64 * 64
        self.buf = np.full(at + BAND, GUARD, U8)
        self.arrays = [np.frombuffer(self.buf, dtype, int(np.prod(shape)), off).reshape(shape) for (shape, dtype), (off, _) in zip(specs, self.spans)]

    def ptr(self, k, given=True):
        return self.arrays[k].ctypes.data if given else None

    def untouched_outside(self, given):
        """every byte outside the arrays the call was given still holds the guard"""
        free = np.ones(len(self.buf), bool)
        for k, (off, nbytes) in enumerate(self.spans):
            if given[k]:
                free[off:off + nbytes] = False
        return bool((self.buf[free] == GUARD).all())


def same(got, want):
    """bit equality of a numpy array with a numpy array or a tensor of the twin"""
    if hasattr(want, "cpu"):
        want = want.cpu().numpy()
    return got.dtype.itemsize == want.dtype.itemsize and got.shape == want.shape and got.tobytes() == want.tobytes()


def dev(a):
    """a tensor of the array on the GPU; the caller holds it for the length of the call that gets its pointer"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def empty(shape, dtype):
    import torch
    t = torch.full(shape, 7, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    return t


def dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def call(ctx, name, *args):
    ctx._chk(getattr(ctx.L, name)(ctx.h, *args), name)


def test_intersect_rays_every_combination(ctx, rays):
    import torch
    ro, rd = rays
    want = (empty((N,), torch.int32), empty((N,), torch.float32), empty((N, 2), torch.float32), empty((N,), torch.int32))
    t_ro, t_rd = dev(ro), dev(rd)
    call(ctx, "ptk_intersect_rays_device", N, dptr(t_ro), dptr(t_rd), SAMPLE, SEED, 0, *(dptr(t) for t in want))
    ctx.synchronize()
    hit = want[0].cpu().numpy() >= 0
    assert hit.any() and not hit.all()
    specs = (((N,), I32), ((N,), F32), ((N, 2), F32), ((N,), I32))
    masks = [m for m in itertools.product((False, True), repeat=4) if any(m)]
    assert len(masks) == 15
    for given in masks:
        s = Slab(*specs)
        call(ctx, "ptk_intersect_rays", N, ro.ctypes.data, rd.ctypes.data, SAMPLE, SEED, 0, *(s.ptr(k, given[k]) for k in range(4)))
        for k in range(4):
            assert not given[k] or same(s.arrays[k], want[k]), (given, k)
        assert s.untouched_outside(given), given


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("bounded", [False, True])
def test_occluded_rays(ctx, rays, n, bounded):
    import torch
    ro, rd = rays[0][:n].copy(), rays[1][:n].copy()
    tmax = np.random.default_rng(n).uniform(0.0, BC.extent(RC.scene("s_cornell")[0]), n).astype(F32) if bounded else None
    want = empty((n,), torch.uint8)
    t_ro, t_rd, t_tmax = dev(ro), dev(rd), (dev(tmax) if bounded else None)
    call(ctx, "ptk_occluded_rays_device", n, dptr(t_ro), dptr(t_rd), dptr(t_tmax), SAMPLE, SEED, 0, dptr(want))
    ctx.synchronize()
    s = Slab(((n,), U8))
    call(ctx, "ptk_occluded_rays", n, ro.ctypes.data, rd.ctypes.data, tmax.ctypes.data if bounded else None, SAMPLE, SEED, 0, s.ptr(0))
    assert same(s.arrays[0], want) and s.untouched_outside([True])
    assert set(np.unique(s.arrays[0])) <= {0, 1}
    if n == N and not bounded:
        assert 0 < int(s.arrays[0].sum()) < n


def test_bake_coverage_every_combination(ctx, uvs):
    import torch
    specs = (((H, W), I32), ((H, W, 2), F32), ((H, W, 3), F32))
    full = Slab(*specs)
    call(ctx, "ptk_bake_coverage", W, H, uvs.ctypes.data, *(full.ptr(k) for k in range(3)))
    assert full.untouched_outside([True] * 3)
    covered = full.arrays[0] >= 0
    assert covered.any() and not covered.all()
    # (coverage has no device entry of its own: its owner plane is the lightmap bake's)
    out, owner, t_uvs = empty((H, W, 3), torch.float32), empty((H, W), torch.int32), dev(uvs)
    call(ctx, "ptk_bake_lightmap_device", W, H, dptr(t_uvs), BC.offset_of(RC.scene("s_cornell")[0]), DEPTH, FIRST, 1, SEED, 0, 0, dptr(out), dptr(owner))
    ctx.synchronize()
    assert same(full.arrays[0], owner)
    masks = [m for m in itertools.product((False, True), repeat=3) if any(m)]
    assert len(masks) == 7
    for given in masks:
        s = Slab(*specs)
        call(ctx, "ptk_bake_coverage", W, H, uvs.ctypes.data, *(s.ptr(k, given[k]) for k in range(3)))
        for k in range(3):
            assert not given[k] or same(s.arrays[k], full.arrays[k]), (given, k)
        assert s.untouched_outside(given), given


@pytest.mark.parametrize("mode", ["owner", "no_owner", "accumulate"])
def test_bake_lightmap(ctx, uvs, mode):
    import torch
    from pbrpathtracer_amd import ptk
    off = BC.offset_of(RC.scene("s_cornell")[0])
    flags = ptk.BAKE_ACCUMULATE if mode == "accumulate" else 0
    before = np.random.default_rng(3).uniform(0.0, 2.0, (H, W, 3)).astype(F32)
    out, owner, t_uvs = (dev(before) if flags else empty((H, W, 3), torch.float32)), empty((H, W), torch.int32), dev(uvs)
    call(ctx, "ptk_bake_lightmap_device", W, H, dptr(t_uvs), off, DEPTH, FIRST, SPP, SEED, 0, flags, dptr(out), dptr(owner))
    ctx.synchronize()
    given = [True, mode != "no_owner"]
    s = Slab(((H, W, 3), F32), ((H, W), I32))
    if flags:
        s.arrays[0][:] = before
    call(ctx, "ptk_bake_lightmap", W, H, uvs.ctypes.data, off, DEPTH, FIRST, SPP, SEED, 0, flags, s.ptr(0), s.ptr(1, given[1]))
    assert same(s.arrays[0], out) and (not given[1] or same(s.arrays[1], owner))
    assert s.untouched_outside(given)
    lit = s.arrays[0][owner.cpu().numpy() >= 0]
    assert (lit != 0).any()
    if flags:
        assert not same(s.arrays[0], before)


@pytest.mark.parametrize("accumulate", [False, True])
def test_trace_rays(ctx, rays, accumulate):
    import torch
    from pbrpathtracer_amd import ptk
    ro, rd = rays
    flags = ptk.RAYS_ACCUMULATE if accumulate else 0
    before = np.random.default_rng(4).uniform(0.0, 2.0, (N, 3)).astype(F32)
    out = dev(before) if accumulate else empty((N, 3), torch.float32)
    t_ro, t_rd = dev(ro), dev(rd)
    call(ctx, "ptk_trace_rays_device", N, dptr(t_ro), dptr(t_rd), DEPTH, FIRST, SPP, SEED, 0, flags, dptr(out))
    ctx.synchronize()
    s = Slab(((N, 3), F32))
    if accumulate:
        s.arrays[0][:] = before
    call(ctx, "ptk_trace_rays", N, ro.ctypes.data, rd.ctypes.data, DEPTH, FIRST, SPP, SEED, 0, flags, s.ptr(0))
    assert same(s.arrays[0], out) and s.untouched_outside([True])
    assert (s.arrays[0] != (before if accumulate else 0)).any()


@pytest.mark.parametrize("sumsq", [True, False])
def test_trace_rays_adaptive(ctx, rays, sumsq):
    import torch
    from pbrpathtracer_amd import ptk
    ro, rd = rays
    args = (DEPTH, RA.THRESHOLD, RA.MIN_SPP, RA.STEP, RA.MAX_SPP, SEED, 0, 0)
    s1, s2, cnt = empty((N, 3), torch.float32), (empty((N, 3), torch.float32) if sumsq else None), empty((N,), torch.int32)
    r_dev, r_host = ptk.RaysAdaptiveResult(), ptk.RaysAdaptiveResult()
    t_ro, t_rd = dev(ro), dev(rd)
    call(ctx, "ptk_trace_rays_adaptive_device", N, dptr(t_ro), dptr(t_rd), *args, dptr(s1), dptr(s2), dptr(cnt), C.byref(r_dev))
    ctx.synchronize()
    given = [True, sumsq, True]
    s = Slab(((N, 3), F32), ((N, 3), F32), ((N,), U32))
    call(ctx, "ptk_trace_rays_adaptive", N, ro.ctypes.data, rd.ctypes.data, *args, s.ptr(0), s.ptr(1, sumsq), s.ptr(2), C.byref(r_host))
    assert same(s.arrays[0], s1) and same(s.arrays[2], cnt) and (not sumsq or same(s.arrays[1], s2))
    assert s.untouched_outside(given)
    assert r_host.as_dict() == r_dev.as_dict() and r_host.as_dict()["ray_samples"] == int(s.arrays[2].sum()) > 0


@pytest.mark.parametrize("with_owner", [True, False])
def test_bake_lightmap_adaptive(ctx, uvs, with_owner):
    import torch
    from pbrpathtracer_amd import ptk
    args = (BC.offset_of(RC.scene("s_cornell")[0]), DEPTH, RA.THRESHOLD, RA.MIN_SPP, RA.STEP, RA.MAX_SPP, SEED, 0, 0)
    out, cnt = empty((H, W, 3), torch.float32), empty((H, W), torch.int32)
    owner, t_uvs = (empty((H, W), torch.int32) if with_owner else None), dev(uvs)
    r_dev, r_host = ptk.RaysAdaptiveResult(), ptk.RaysAdaptiveResult()
    call(ctx, "ptk_bake_lightmap_adaptive_device", W, H, dptr(t_uvs), *args, dptr(out), dptr(cnt), dptr(owner), C.byref(r_dev))
    ctx.synchronize()
    given = [True, True, with_owner]
    s = Slab(((H, W, 3), F32), ((H, W), U32), ((H, W), I32))
    call(ctx, "ptk_bake_lightmap_adaptive", W, H, uvs.ctypes.data, *args, s.ptr(0), s.ptr(1), s.ptr(2, with_owner), C.byref(r_host))
    assert same(s.arrays[0], out) and same(s.arrays[1], cnt) and (not with_owner or same(s.arrays[2], owner))
    assert s.untouched_outside(given)
    assert r_host.as_dict() == r_dev.as_dict() and r_host.as_dict()["ray_samples"] == int(s.arrays[1].sum()) > 0


@pytest.mark.parametrize("mode", ["radiance", "no_radiance", "accumulate"])
def test_bake_probes(ctx, mode):
    import torch
    from pbrpathtracer_amd import probes, ptk
    P, D = 3, 5
    pos, dirs = RC.rays_in_box(RC.scene("s_cornell")[0], P, 7)[0], probes.fibonacci_dirs(D)
    flags = ptk.PROBES_ACCUMULATE if mode == "accumulate" else 0
    args = (DEPTH, FIRST, SPP, SEED, 0, flags, probes.sh_weight(D, SPP))
    before = np.random.default_rng(5).uniform(0.0, 2.0, (P, D, 3)).astype(F32)
    rad = None if mode == "no_radiance" else (dev(before) if flags else empty((P, D, 3), torch.float32))
    coefs, t_pos, t_dirs = empty((P, 9, 3), torch.float32), dev(pos), dev(dirs)
    call(ctx, "ptk_bake_probes_device", P, dptr(t_pos), D, dptr(t_dirs), *args, dptr(rad), dptr(coefs))
    ctx.synchronize()
    given = [mode != "no_radiance", True]
    s = Slab(((P, D, 3), F32), ((P, 9, 3), F32))
    if flags:
        s.arrays[0][:] = before
    call(ctx, "ptk_bake_probes", P, pos.ctypes.data, D, dirs.ctypes.data, *args, s.ptr(0, given[0]), s.ptr(1))
    assert same(s.arrays[1], coefs) and (not given[0] or same(s.arrays[0], rad))
    assert s.untouched_outside(given)
    assert (s.arrays[1] != 0).any()


def test_probes_irradiance(ctx):
    import torch
    dims, origin, spacing = (2, 2, 2), (-1.0, 0.5, 2.0), (1.5, 0.75, 2.0)
    g = ((C.c_int32 * 3)(*dims), (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing))
    coefs = np.random.default_rng(6).normal(0.0, 1.0, (2, 2, 2, 9, 3)).astype(F32)
    pts, nrm = PC.queries(dims, origin, spacing, N, 8)
    want, t_coefs, t_pts, t_nrm = empty((N, 3), torch.float32), dev(coefs), dev(pts), dev(nrm)
    call(ctx, "ptk_probes_irradiance_device", *g, dptr(t_coefs), N, dptr(t_pts), dptr(t_nrm), dptr(want))
    ctx.synchronize()
    s = Slab(((N, 3), F32))
    call(ctx, "ptk_probes_irradiance", *g, coefs.ctypes.data, N, pts.ctypes.data, nrm.ctypes.data, s.ptr(0))
    assert same(s.arrays[0], want) and s.untouched_outside([True])
    assert np.isfinite(s.arrays[0]).any() and (s.arrays[0] != 0).any()


@pytest.mark.parametrize("passes", [1, 2])
def test_lightmap_dilate(ctx, passes):
    rng = np.random.default_rng(passes)
    owner = np.where(rng.uniform(size=(H, W)) < 0.15, rng.integers(0, 50, (H, W)), -1).astype(I32)
    img = np.where((owner >= 0)[..., None], rng.uniform(0, 3, (H, W, 3)), 0).astype(F32)
    t_img, t_own = dev(img), dev(owner)
    call(ctx, "ptk_lightmap_dilate_device", W, H, passes, dptr(t_img), dptr(t_own))
    ctx.synchronize()
    s = Slab(((H, W, 3), F32), ((H, W), I32))
    s.arrays[0][:] = img; s.arrays[1][:] = owner
    call(ctx, "ptk_lightmap_dilate", W, H, passes, s.ptr(0), s.ptr(1))
    assert same(s.arrays[0], t_img) and same(s.arrays[1], t_own) and s.untouched_outside([True, True])
    assert not same(s.arrays[1], owner)
