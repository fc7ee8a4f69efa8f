"""The cycle unit of the exact PLAIN trace kernels (csrc/ptk_kernels_cycle.hip, csrc/ptk_trace_cycle.h, csrc/ptk_unit_map.h;
include/ptk.h "flat_cycle", ptk_trace_unit): the pair unit's pass and shade block in a fixed deal / shade / pass cycle, the work
units dealt from scalar registers.

Nothing a path computes may change, and which lane traces which unit must not matter: every comparison is np.array_equal on the
float accumulator - against the CPU oracle, against "flat_cycle" 0 (the pair unit's kernel under the block vote) and against
"plain_kernel" 0 (the generic FLAT kernel).  ptk_trace_unit says which kernel a render ran.

Frames of 64 x 48 and 80 x 40, 8 spp (48 where the sample buffer is to be passed several times); every oracle image is computed
once per module and shared."""
import numpy as np
import pytest

import flat_rect_scenes as R
import flat_zero_scenes as Z

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 64, 48, 8, 47
DEPTHS = (0, 1, 2, 3, 8)


class _Refs:
    def __init__(self, OB):
        a, self.cam = Z.cornell()
        self.OB = OB; self.images = {}
        self.scenes = {
            "staged-box": Z.subset(a, R.BOX6),                       # six pairs: the whole list is the pair loop's
            "golden-box": a,                                         # four pairs, then four turns of the record loop
            "no-pair": Z.subset(a, [9] + R.BOX6[:10]),               # a single record in front: the record loop alone
            "one-triangle": Z.one_triangle(a),
        }
        # the light quad and the wall the camera looks at (the quad of the staged box most nearly square on to it)
        d = np.asarray(self.cam["dir"], np.float64)
        lights = [int(l) for l in a["lights"]]
        quads = [q for q in zip(R.BOX6[0::2], R.BOX6[1::2]) if q[0] not in lights]
        def facing(q):
            v = np.asarray(a["verts"][q[0]], np.float64).reshape(3, 3)
            n = np.cross(v[1] - v[0], v[2] - v[0])
            return abs(n @ d) / np.linalg.norm(n)
        self.scenes["light+wall"] = Z.subset(a, lights + list(max(quads, key=facing)))

    def image(self, name, arrays, D, cam=None, w=W, h=H, spp=SPP):
        key = (name, D, w, h, spp)
        if key not in self.images:
            c = cam or self.cam
            o = self.OB.Oracle(arrays)
            tot, _ = o.render(self.OB.make_camera(c["pos"], c["dir"], c["up"], c["focal"], c["fovy"], c["focal_dist"], c["aperture"]),
                              w, h, D, 0, spp, SEED)
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


DEFAULTS = (("flat_cycle", 1), ("flat_rect_pairs", 1), ("flat_zero_classes", 1), ("plain_kernel", 1), ("lambert_kernel", 1), ("persistent", -1),
            ("chunk", 0), ("contract", 0))


def _setup(ctx, arrays, cam, D=8, w=W, h=H):
    for name, v in DEFAULTS:
        ctx.set_option(name, v)
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(w, h, D); ctx.set_tile(0, 1)


def _render(ctx, spp=SPP):
    ctx.reset(); ctx.render(0, spp, SEED)
    return ctx.read_accum()


def _ways(ctx, want, label, lambert=True, spp=SPP):
    """the cycle unit, the pair unit, the generic FLAT kernel: each the oracle's accumulator, bit for bit"""
    from pbrpathtracer_amd import ptk
    try:
        ctx.set_option("flat_cycle", 1)
        on = _render(ctx, spp)
        assert (ctx.trace_variant(), ctx.trace_unit(), ctx.trace_is_lambert()) == (ptk.TRACE_FLAT_PLAIN, ptk.UNIT_CYCLE, lambert), label
        ctx.set_option("flat_cycle", 0)
        off = _render(ctx, spp)
        assert (ctx.trace_variant(), ctx.trace_unit(), ctx.trace_is_lambert()) == (ptk.TRACE_FLAT_PLAIN, ptk.UNIT_RECT, lambert), label
        ctx.set_option("plain_kernel", 0)
        generic = _render(ctx, spp)
        assert (ctx.trace_variant(), ctx.trace_unit()) == (ptk.TRACE_FLAT, ptk.UNIT_NONE), label
    finally:
        ctx.set_option("plain_kernel", 1); ctx.set_option("flat_cycle", 1)
    assert np.array_equal(on, want), (label, "against the oracle", int((on != want).sum()))
    assert np.array_equal(on, off), (label, "against flat_cycle = 0", int((on != off).sum()))
    assert np.array_equal(on, generic), (label, "against plain_kernel = 0", int((on != generic).sum()))
    return on


@pytest.mark.parametrize("level", ["lambert", "generic"])
@pytest.mark.parametrize("name", ["staged-box", "golden-box", "no-pair", "one-triangle"])
def test_every_depth_of_both_levels_is_the_oracles_frame(ctx, refs, name, level):
    """trace depths 0, 1, 2, 3 and 8; the LAMBERT level and, through a material with reflectiveness > 0 (iter != depth), the generic
    one; six pairs, four pairs and the record loop, the record loop alone, one triangle"""
    from pbrpathtracer_amd import ptk
    arrays = refs.scenes[name] if level == "lambert" else Z.mirror(refs.scenes[name])
    assert ptk.scene_is_plain(arrays) and ptk.scene_is_lambert(arrays) == (level == "lambert")
    _setup(ctx, arrays, refs.cam)
    assert len(ctx.flat_rect_pairs()) == {"staged-box": 6, "golden-box": 4, "no-pair": 0, "one-triangle": 0}[name]
    lit = False
    for D in DEPTHS:
        ctx.set_frame(W, H, D)
        got = _ways(ctx, refs.image(f"{name}/{level}", arrays, D), (name, level, D), lambert=level == "lambert")
        lit |= bool((got != 0).any())
    assert lit, name


def _roll(cam, deg, back, side, rise):
    """the camera moved back along its axis, off it by (side, rise), and rolled about it"""
    c = dict(cam)
    d = np.asarray(cam["dir"], np.float64); d = d / np.linalg.norm(d)
    up = np.asarray(cam["up"], np.float64); up = up - d * (up @ d); up = up / np.linalg.norm(up)
    right = np.cross(d, up)
    t = np.deg2rad(deg)
    c["up"] = (np.cos(t) * up + np.sin(t) * right).astype(np.float32)
    c["pos"] = (np.asarray(cam["pos"], np.float64) - back * d + side * right + rise * up).astype(np.float32)
    return c


def test_quadrants_with_one_live_pixel_and_with_sixty_three(ctx, refs):
    """the light and the wall the camera looks at, nothing else, seen rolled from behind the camera's place: the wall's edges cut
    8 x 8 quadrants at a slant.  Every point of the wall sees the light and the light is lit itself, so at depth 2 the frame's
    non-zero pixels are the live ones; the camera is the first of a fixed list whose frame has a quadrant with exactly one live
    pixel (n_live = 1: the deal's division is skipped) and one with 63"""
    arrays = refs.scenes["light+wall"]
    _setup(ctx, arrays, refs.cam, D=2)
    found = None
    for deg in (27.0, 41.0, 13.0):
        for back in (0.0, 1.5, 3.0):
            for side in np.arange(0.0, 0.36, 0.03):
                for rise in (0.0, 0.11, 0.23):
                    cam = _roll(refs.cam, deg, back, float(side), rise)
                    ctx.set_camera(**cam)
                    ctx.reset(); ctx.render(0, 1, SEED)
                    live = (ctx.read_accum() != 0).any(axis=2)
                    counts = live.reshape(H // 8, 8, W // 8, 8).sum(axis=(1, 3))
                    if (counts == 1).any() and (counts == 63).any():
                        found = cam; break
                if found: break
            if found: break
        if found: break
    assert found is not None, "no camera of the list leaves a quadrant with 1 and one with 63 live pixels"
    ctx.set_camera(**found)
    for D in (2, 3, 8):
        ctx.set_frame(W, H, D)
        want = refs.image("light+wall/rolled", arrays, D, cam=found)
        counts = (want != 0).any(axis=2).reshape(H // 8, 8, W // 8, 8).sum(axis=(1, 3))
        assert (counts == 1).any() and (counts == 63).any(), counts
        for persistent in (-1, 0):
            ctx.set_option("persistent", persistent)
            try:
                _ways(ctx, want, ("rolled", D, persistent))
            finally:
                ctx.set_option("persistent", -1)


@pytest.mark.parametrize("persistent", [0, 1])
@pytest.mark.parametrize("chunk", [4, 8])
def test_one_item_per_wave_persistent_waves_and_both_chunk_sizes(ctx, refs, persistent, chunk):
    arrays = refs.scenes["golden-box"]
    _setup(ctx, arrays, refs.cam, w=80, h=40)
    ctx.set_option("persistent", persistent); ctx.set_option("chunk", chunk)
    try:
        for D in (1, 8):
            ctx.set_frame(80, 40, D)
            _ways(ctx, refs.image("golden-box/80x40", arrays, D, w=80, h=40), ("golden-box", persistent, chunk, D))
    finally:
        ctx.set_option("persistent", -1); ctx.set_option("chunk", 0)


def test_a_three_way_tile_split(ctx, refs):
    arrays = refs.scenes["staged-box"]
    _setup(ctx, arrays, refs.cam)
    want = refs.image("staged-box/lambert", arrays, 8)
    from pbrpathtracer_amd import ptk
    total = np.zeros_like(want)
    try:
        for r in range(3):
            ctx.set_tile(r, 3)
            part = _render(ctx)
            assert ctx.trace_unit() == ptk.UNIT_CYCLE
            assert not np.any((part != 0) & (total != 0))
            total += part
    finally:
        ctx.set_tile(0, 1)
    assert np.array_equal(total, want)


def test_several_passes_of_the_sample_buffer_and_a_resumed_sample_range(ctx, refs):
    """48 spp of an 80 x 40 frame through a sample buffer of 1 MiB (65 536 samples: three passes), then 8 spp as 5 + 3"""
    from pbrpathtracer_amd import ptk
    arrays = refs.scenes["golden-box"]
    _setup(ctx, arrays, refs.cam, D=3, w=80, h=40)
    ctx.set_option("pass_bytes", 1 << 20)
    try:
        _ways(ctx, refs.image("golden-box/80x40", arrays, 3, w=80, h=40, spp=48), "three passes", spp=48)
    finally:
        ctx.set_option("pass_bytes", 16.0 * 1073741824.0)               # (the default)
    want = refs.image("golden-box/80x40", arrays, 3, w=80, h=40)
    ctx.reset(); ctx.render(0, 5, SEED); ctx.render(5, 3, SEED)
    assert ctx.trace_unit() == ptk.UNIT_CYCLE
    assert np.array_equal(ctx.read_accum(), want)


def test_geometry_updates_that_shrink_and_regrow_the_pair_prefix(ctx, refs):
    """one ulp on the fifth quad's second record: six pairs become four and two single records; the old vertices back: six again"""
    from pbrpathtracer_amd import ptk
    a = refs.scenes["staged-box"]
    _setup(ctx, a, refs.cam)
    p0 = ctx.flat_rect_pairs()
    assert len(p0) == 6
    first = _ways(ctx, refs.image("staged-box/lambert", a, 8), "six pairs")
    moved = dict(a); moved["verts"] = a["verts"].copy()
    v = moved["verts"][9].reshape(3, 3)
    axis = [k for k in range(3) if v[1, k] != v[0, k]][0]
    edge = np.float32(v[1, axis] - v[0, axis])
    for _ in range(4):
        v[1, axis] = np.nextafter(v[1, axis], np.float32(np.inf))
        if np.float32(v[1, axis] - v[0, axis]) != edge: break
    assert ptk.flat_rect_prefix(moved["verts"]) == p0[:4]
    ctx.update_geometry(9, moved["verts"][9:10])
    assert ctx.flat_rect_pairs() == p0[:4]
    _ways(ctx, refs.image("staged-box/four pairs", moved, 8), "four pairs")
    ctx.update_geometry(9, a["verts"][9:10])
    assert ctx.flat_rect_pairs() == p0
    assert np.array_equal(_ways(ctx, refs.image("staged-box/lambert", a, 8), "six pairs again"), first)


def test_the_unit_query_follows_every_option(ctx, refs):
    from pbrpathtracer_amd import ptk
    from test_gpu_random_scenes import random_scene
    a = refs.scenes["staged-box"]
    _setup(ctx, a, refs.cam, D=2)
    want = refs.image("staged-box/lambert", a, 2)
    cases = [({}, ptk.UNIT_CYCLE), ({"flat_cycle": 0}, ptk.UNIT_RECT), ({"flat_rect_pairs": 0}, ptk.UNIT_PLAIN),
             ({"flat_rect_pairs": 0, "flat_cycle": 0}, ptk.UNIT_PLAIN), ({"plain_kernel": 0}, ptk.UNIT_NONE), ({"lambert_kernel": 0}, ptk.UNIT_CYCLE)]
    for opts, unit in cases:
        try:
            for k, v in opts.items(): ctx.set_option(k, v)
            got = _render(ctx)
            assert ctx.trace_unit() == unit, (opts, ctx.trace_unit())
            assert ctx.trace_is_lambert() == (unit != ptk.UNIT_NONE and "lambert_kernel" not in opts), opts
            assert np.array_equal(got, want), opts
        finally:
            for name, v in DEFAULTS: ctx.set_option(name, v)
    # the contracted builds keep their PLAIN kernels in the common unit; the counters' kernels and the BVH walk have no unit either
    try:
        ctx.set_option("contract", 1)
        _render(ctx)
        assert (ctx.trace_variant(), ctx.trace_unit()) == (ptk.TRACE_FLAT_PLAIN, ptk.UNIT_NONE)
    finally:
        ctx.set_option("contract", 0)
    ctx.collect_stats(0, 1, SEED)
    assert (ctx.trace_variant(), ctx.trace_unit()) == (ptk.TRACE_FLAT, ptk.UNIT_NONE)
    _render(ctx)
    assert ctx.trace_unit() == ptk.UNIT_CYCLE
    arrays, cam = random_scene(14, 300, True)
    ctx.upload_scene(arrays); ctx.set_camera(**cam)
    _render(ctx, 1)
    assert (ctx.trace_variant(), ctx.trace_unit()) == (ptk.TRACE_BVH, ptk.UNIT_NONE)
