"""The accept of the pair pass as wave masks with one update per ray (csrc/ptk_kernels.hip tri_accept_rect, csrc/ptk_flat_mt.h
mt_rect_accept_once), where tests/test_gpu_flat_rect_pairs.py does not reach: equal distances, waves with few lanes in the pass,
prefixes that change length under geometry updates.

Nothing a path computes may change: every comparison is np.array_equal on the float accumulator - against the CPU oracle, against
"flat_rect_pairs" 0 (the kernels without the pair loop) and against "plain_kernel" 0 (the generic FLAT kernel).

Frames of 64 x 48, 4 spp, depths 1, 3 and 8; every oracle image is computed once per module and shared."""
import numpy as np
import pytest

import flat_rect_scenes as R
import flat_zero_scenes as Z

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 64, 48, 4, 31
DEPTHS = (1, 3, 8)


def _twins(box, light_copy):
    """the box with a coincident twin of its light quad in front of it: 14 records, seven pairs, the twins first; the scene's lights
    are the twins' copy `light_copy` (0: records 0, 1; 1: records 2, 3), the other copy is the same emitter outside the light list"""
    lights = sorted(int(l) for l in box["lights"])
    assert len(lights) == 2 and lights[1] == lights[0] + 1
    rest = [k for k in range(len(box["verts"])) if k not in lights]
    b = Z.subset(box, lights + lights + rest)
    assert [int(l) for l in b["lights"]] == [0, 1] and len(b["verts"]) == 14
    b["lights"] = np.array([2 * light_copy, 2 * light_copy + 1], np.int32)
    return b


def _sparse_camera(cam):
    """the box seen from far behind the camera's place and off axis: it covers a few pixels about the frame's centre lines, so most
    8 x 8 pixel blocks that hold any live pixel hold only a few"""
    c = dict(cam)
    d = np.asarray(cam["dir"], np.float64); d = d / np.linalg.norm(d)
    up = np.asarray(cam["up"], np.float64)
    side = np.cross(d, up); side = side / np.linalg.norm(side)
    c["pos"] = (np.asarray(cam["pos"], np.float64) - 7.0 * d + 0.35 * side + 0.3 * up).astype(np.float32)
    return c


class _Refs:
    def __init__(self, OB):
        _, self.cam = Z.cornell()
        a, _ = Z.cornell()
        self.OB = OB; self.images = {}
        self.box = Z.subset(a, R.BOX6)
        self.sparse = _sparse_camera(self.cam)

    def image(self, name, arrays, D, cam=None):
        key = (name, D)
        if key not in self.images:
            c = cam or self.cam
            o = self.OB.Oracle(arrays)
            tot, _ = o.render(self.OB.make_camera(c["pos"], c["dir"], c["up"], c["focal"], c["fovy"], c["focal_dist"], c["aperture"]),
                              W, H, D, 0, SPP, SEED)
            o.close()
            tot.setflags(write=False)
            self.images[key] = tot
        return self.images[key]


@pytest.fixture(scope="module")
def refs(oracle_mod):
    return _Refs(oracle_mod)


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def _setup(ctx, arrays, cam, D=8):
    for name, v in (("flat_rect_pairs", 1), ("flat_zero_classes", 1), ("plain_kernel", 1), ("lambert_kernel", 1), ("persistent", -1)):
        ctx.set_option(name, v)
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(0, 1)


def _render(ctx):
    ctx.reset(); ctx.render(0, SPP, SEED)
    return ctx.read_accum()


def _three_ways(ctx, want, label, lambert=True):
    """pairs on, pairs off, the generic FLAT kernel: each the oracle's accumulator, bit for bit"""
    from pbrpathtracer_amd import ptk
    try:
        ctx.set_option("flat_rect_pairs", 1)
        on = _render(ctx)
        assert ctx.trace_variant() == ptk.TRACE_FLAT_PLAIN and ctx.trace_is_lambert() == lambert, label
        ctx.set_option("flat_rect_pairs", 0)
        off = _render(ctx)
        assert ctx.trace_variant() == ptk.TRACE_FLAT_PLAIN and ctx.trace_is_lambert() == lambert, label
        ctx.set_option("plain_kernel", 0)
        generic = _render(ctx)
        assert ctx.trace_variant() == ptk.TRACE_FLAT, label
    finally:
        ctx.set_option("plain_kernel", 1); ctx.set_option("flat_rect_pairs", 1)
    assert np.array_equal(on, want), (label, "against the oracle", int((on != want).sum()))
    assert np.array_equal(on, off), (label, "against flat_rect_pairs = 0", int((on != off).sum()))
    assert np.array_equal(on, generic), (label, "against plain_kernel = 0", int((on != generic).sum()))
    return on


@pytest.mark.parametrize("light_copy", [0, 1])
def test_equal_distances_leave_the_first_twin_as_the_closest_hit(ctx, refs, light_copy):
    """a coincident twin of the light quad: every ray that reaches it finds the same t twice, and the second pair's t < best must fail.
    A shadow ray towards a light triangle is lit when the reported hit is that triangle, so the two orders of the twins differ in
    the direct light - the oracle's image of each order is the yardstick, and the first order's is not black"""
    from pbrpathtracer_amd import ptk
    arrays = _twins(refs.box, light_copy)
    assert ptk.scene_is_plain(arrays) and ptk.scene_is_lambert(arrays)
    _setup(ctx, arrays, refs.cam)
    pairs = ctx.flat_rect_pairs()
    assert pairs == ptk.flat_rect_prefix(arrays["verts"]) and len(pairs) == 7 and pairs[0] == pairs[1], pairs
    for D in DEPTHS:
        ctx.set_frame(W, H, D)
        got = _three_ways(ctx, refs.image(f"twins{light_copy}", arrays, D), ("twins", light_copy, D))
        if light_copy == 0:
            # (the counts of the oracle's image, taken when this test was written: the comparison is not between black frames)
            assert int((got != 0).sum()) == (2178 if D == 1 else 2187), (D, int((got != 0).sum()))
    # ... and the orders do differ: with the listed light behind its twin every shadow ray reports the twin
    if light_copy == 1:
        assert not np.array_equal(refs.image("twins1", arrays, 8), refs.image("twins0", _twins(refs.box, 0), 8))


@pytest.mark.parametrize("level", ["lambert", "generic"])
def test_waves_with_few_lanes_in_the_pass(ctx, refs, level):
    """both levels of the kernel, one item per wave and a three-way tile split, through a camera that leaves most blocks of pixels
    a few live ones: the masks then carry a few bits, and a compare must return none for the lanes that do not run it"""
    arrays = refs.box if level == "lambert" else Z.mirror(refs.box)
    cam = refs.sparse
    _setup(ctx, arrays, cam)
    lit = False
    for D in DEPTHS:
        ctx.set_frame(W, H, D)
        want = refs.image(f"sparse/{level}", arrays, D, cam)
        live = (want != 0).any(axis=2)
        blocks = live.reshape(H // 8, 8, W // 8, 8).sum(axis=(1, 3))
        if D == 8:
            assert 0 < live.sum() < W * H // 8 and (blocks[blocks > 0] < 32).sum() * 2 > (blocks > 0).sum(), blocks
        lit |= bool(live.any())
        _three_ways(ctx, want, ("sparse", level, D), lambert=level == "lambert")
        ctx.set_option("persistent", 0)
        try:
            _three_ways(ctx, want, ("sparse", level, D, "one item per wave"), lambert=level == "lambert")
            if D == 8:
                total = np.zeros_like(want)
                for r in range(3):
                    ctx.set_tile(r, 3)
                    part = _render(ctx)
                    assert not np.any((part != 0) & (total != 0))
                    total += part
                assert np.array_equal(total, want), (level, "tiles")
        finally:
            ctx.set_tile(0, 1); ctx.set_option("persistent", -1)
    assert lit


def test_geometry_updates_that_shorten_and_restore_the_prefix(ctx, refs):
    """one ulp on the fifth quad's second record: six pairs become four and two single records; the old vertices back: six again.
    Rendered after each update, each time the oracle's frame for the geometry as it then is"""
    from pbrpathtracer_amd import ptk
    a = refs.box
    _setup(ctx, a, refs.cam)
    p0 = ctx.flat_rect_pairs()
    assert len(p0) == 6
    first = _three_ways(ctx, refs.image("box", a, 8), "six pairs")
    moved = dict(a); moved["verts"] = a["verts"].copy()
    v = moved["verts"][9].reshape(3, 3)                              # record 9 = (p0, p2, p3) of the fifth quad
    axis = [k for k in range(3) if v[1, k] != v[0, k]][0]
    # (the stored word is the float32 difference p2 - p0: step the coordinate until that difference moves, and it moves by one ulp)
    edge = np.float32(v[1, axis] - v[0, axis])
    for _ in range(4):
        v[1, axis] = np.nextafter(v[1, axis], np.float32(np.inf))
        if np.float32(v[1, axis] - v[0, axis]) != edge: break
    assert np.float32(v[1, axis] - v[0, axis]) == np.nextafter(edge, np.float32(np.inf))
    assert ptk.flat_rect_prefix(moved["verts"]) == p0[:4]
    ctx.update_geometry(9, moved["verts"][9:10])
    assert ctx.flat_rect_pairs() == p0[:4]
    for D in DEPTHS:
        ctx.set_frame(W, H, D)
        _three_ways(ctx, refs.image("box/four pairs", moved, D), ("four pairs", D))
    ctx.update_geometry(9, a["verts"][9:10])
    assert ctx.flat_rect_pairs() == p0
    for D in DEPTHS:
        ctx.set_frame(W, H, D)
        again = _three_ways(ctx, refs.image("box", a, D), ("six pairs again", D))
    assert np.array_equal(again, first)
