"""The LAMBERT level of the PLAIN trace kernel (trace_kernel<false, true, true, true>, csrc/ptk_kernels.hip; shade_interaction's
LAMBERT switch, csrc/ptk_device_fn.h) and the predicate that selects it (csrc/ptk_api.hip lambert_tables; include/ptk.h
"lambert_kernel", ptk_scene_is_lambert, ptk_trace_is_lambert).

In a plain scene without a material of reflectiveness > 0 the specular draw can never succeed, so the level keeps that draw's
advance of the stream and the diffuse route and drops the rest.  Nothing a path computes changes: every comparison here is
np.array_equal on the float accumulator and the RGB8 image, against the PLAIN kernel's generic level ("lambert_kernel" 0), the
generic FLAT kernel ("plain_kernel" 0) and the CPU oracle.  Results only; no test looks at instructions.

The 12-triangle Cornell golden at 64 x 48, 8 spp, as tests/test_gpu_flat_schedule.py renders it; every oracle image is computed
once per module and shared."""
import numpy as np
import pytest

from conftest import load_golden, scene_from_golden

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 64, 48, 8, 41
DEPTHS = (0, 1, 2, 3, 8)
DENORMAL = np.float32(1.401298464324817e-45)       # 2^-149: the smallest reflectiveness a draw (of exactly 0) can be below
# the box seen from the side: its silhouette leaves one 8 x 8 quadrant of the frame with a single pixel whose camera ray hits
SIDE_DIR = (0.27635565, 0.0, 0.96105544)


def _cornell():
    z = load_golden("tier_s_cornell.npz")
    a = {k: np.array(v) for k, v in scene_from_golden(z).items()}
    a["uvs"] = np.random.RandomState(5).rand(len(a["verts"]), 6).astype(np.float32)
    cam = z["cam"]; proj = z["proj"]
    cam = dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]),
               focal_dist=float(z["focal_dist"]), aperture=0.0)
    return a, cam


def _with_reflectiveness(a, which, value):
    b = dict(a); b["materials"] = a["materials"].copy()
    b["materials"]["reflectiveness"][which] = value
    return b


class _Refs:
    """oracle images of (scene variant, camera, depth, sample count), each rendered once"""
    def __init__(self, OB):
        self.OB = OB; self.oracles = {}; self.images = {}
        self.arrays, self.cam = _cornell()
        self.scenes = {"cornell": self.arrays,
                       "denormal": _with_reflectiveness(self.arrays, 1, DENORMAL),
                       "minus zero": _with_reflectiveness(self.arrays, 1, np.float32(-0.0)),
                       "mirror": _with_reflectiveness(self.arrays, 2, np.float32(0.7))}
        self.cams = {"front": self.cam, "side": dict(self.cam, dir=SIDE_DIR), "away": dict(self.cam, dir=(0.0, 0.0, -1.0))}

    def _oracle(self, scene):
        if scene not in self.oracles: self.oracles[scene] = self.OB.Oracle(self.scenes[scene])
        return self.oracles[scene]

    def _camera(self, cam):
        c = self.cams[cam]
        return self.OB.make_camera(c["pos"], c["dir"], c["up"], c["focal"], c["fovy"], c["focal_dist"], c["aperture"])

    def image(self, D, spp=SPP, scene="cornell", cam="front"):
        key = (scene, cam, D, spp)
        if key not in self.images:
            tot, rgb = self._oracle(scene).render(self._camera(cam), W, H, D, 0, spp, SEED)
            tot.setflags(write=False); rgb.setflags(write=False)
            self.images[key] = (tot, rgb)
        return self.images[key]

    def live_pixels(self, cam):
        """[H, W] bool: the pixels whose camera ray hits something (the pinhole's ray is the same for every sample)"""
        c = self._oracle("cornell").render_counted(self._camera(cam), W, H, 1, 0, 1, SEED)["counts"].reshape(W * H, -1)
        miss = (c[:, 1] == c[:, 0]) & (c[:, 2] == 0) & (c[:, 3] == 0) & (c[:, 4] == 0)
        return (~miss).reshape(H, W)

    def close(self):
        for o in self.oracles.values(): o.close()


@pytest.fixture(scope="module")
def refs(oracle_mod):
    r = _Refs(oracle_mod)
    yield r
    r.close()


def _ctx(arrays, cam, D):
    from pbrpathtracer_amd import ptk
    ctx = ptk.Context(0)
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(0, 1)
    return ctx


LEVELS = ("lambert", "plain", "flat")


def _select(ctx, level):
    ctx.set_option("plain_kernel", 0 if level == "flat" else 1)
    ctx.set_option("lambert_kernel", 1 if level == "lambert" else 0)


def _ran(ctx, level):
    from pbrpathtracer_amd import ptk
    want = {"lambert": (ptk.TRACE_FLAT_PLAIN, True), "plain": (ptk.TRACE_FLAT_PLAIN, False), "flat": (ptk.TRACE_FLAT, False)}[level]
    assert (ctx.trace_variant(), ctx.trace_is_lambert()) == want, (level, ctx.trace_variant(), ctx.trace_is_lambert())


def _render(ctx, spp=SPP):
    ctx.reset(); ctx.render(0, spp, SEED)
    return ctx.read_accum(), ctx.resolve_rgb8()


def _same(got, ref, label):
    assert np.array_equal(got[0], ref[0]), (label, "accumulator", int((got[0] != ref[0]).sum()))
    assert np.array_equal(got[1], ref[1]), (label, "rgb8", int((got[1] != ref[1]).sum()))


@pytest.mark.parametrize("persistent", [1, 0])
def test_four_renders_agree_at_every_depth(refs, persistent):
    """the queued and the one-item-per-wave distribution; the terminal rule meets the path start and the roulette at depths 0..3"""
    from pbrpathtracer_amd import ptk
    assert ptk.scene_is_lambert(refs.arrays)
    ctx = _ctx(refs.arrays, refs.cam, 8)
    try:
        ctx.set_option("persistent", persistent)
        lit = 0
        for D in DEPTHS:
            ctx.set_frame(W, H, D)
            want = refs.image(D)
            lit += int((want[0] != 0).any())
            for level in LEVELS:
                _select(ctx, level)
                got = _render(ctx)
                _ran(ctx, level)
                _same(got, want, (persistent, D, level))
        assert lit >= len(DEPTHS) - 1              # (depth 0 is black: every path ends at its first interaction)
    finally:
        ctx.close()


@pytest.mark.parametrize("D", DEPTHS)
def test_tile_split_passes_and_resumed_ranges(refs, D):
    want, want48 = refs.image(D), refs.image(D, 48)
    ctx = _ctx(refs.arrays, refs.cam, D)
    try:
        for level in LEVELS:
            _select(ctx, level)
            # a 3-way tile split: the shares do not overlap and add up to the frame
            total = np.zeros_like(want[0])
            for r in range(3):
                ctx.set_tile(r, 3); ctx.reset(); ctx.render(0, SPP, SEED)
                _ran(ctx, level)
                part = ctx.read_accum()
                assert not np.any((part != 0) & (total != 0))
                total += part
            ctx.set_tile(0, 1)
            assert np.array_equal(total, want[0]), (D, level, "tiles")
            # two passes of one render: the smallest budget (1 MiB) holds 21 samples of this frame's 12 tiles
            tiles = ((W + 15) // 16) * ((H + 15) // 16)
            assert 2 ** 20 // (tiles * 4 * 64 * 16) < 48
            ctx.set_option("pass_bytes", 2 ** 20)
            _same(_render(ctx, 48), want48, (D, level, "passes"))
            ctx.set_option("pass_bytes", 16 * 2 ** 30)
            # a resumed sample range
            ctx.reset()
            for first, n in ((0, 5), (5, 1), (6, 42)):
                ctx.render(first, n, SEED)
            _ran(ctx, level)
            _same((ctx.read_accum(), ctx.resolve_rgb8()), want48, (D, level, "resumed"))
    finally:
        ctx.close()


@pytest.mark.parametrize("persistent", [1, 0])
def test_a_quadrant_with_exactly_one_live_pixel(refs, persistent):
    """one live pixel: every unit of the item is the same pixel (the deal's n_live == 1 route)"""
    live = refs.live_pixels("side")
    per_quadrant = live.reshape(H // 8, 8, W // 8, 8).sum(axis=(1, 3))
    assert (per_quadrant == 1).any() and (per_quadrant == 64).any() and (per_quadrant == 0).any(), per_quadrant
    ctx = _ctx(refs.arrays, refs.cams["side"], 8)
    try:
        ctx.set_option("persistent", persistent)
        for D in DEPTHS:
            ctx.set_frame(W, H, D)
            want = refs.image(D, cam="side")
            for level in LEVELS:
                _select(ctx, level)
                got = _render(ctx)
                _ran(ctx, level)
                _same(got, want, (persistent, D, level))
    finally:
        ctx.close()


@pytest.mark.parametrize("contract", [1, 2])
def test_contracted_lambert_reproduces_contracted_plain(refs, contract):
    """the contracted builds are recompilations of the same text: reproducible, so their LAMBERT level reproduces their PLAIN kernel"""
    ctx = _ctx(refs.arrays, refs.cam, 8)
    try:
        ctx.set_option("contract", contract)
        for D in DEPTHS:
            ctx.set_frame(W, H, D)
            got = {}
            for level in LEVELS:
                _select(ctx, level)
                got[level] = _render(ctx)
                _ran(ctx, level)
            assert D == 0 or (got["lambert"][0] != 0).any()
            _same(got["lambert"], got["plain"], (contract, D, "plain"))
            _same(got["lambert"], got["flat"], (contract, D, "flat"))
    finally:
        ctx.close()


def test_draw_order_on_either_side_of_the_predicate(refs):
    """A material whose reflectiveness is the smallest denormal takes a specular bounce exactly when its draw is 0: not Lambert, and
    the PLAIN kernel follows the oracle through it.  With -0 in its place no draw is below it: Lambert, and the level follows the
    oracle with the draw reduced to its advance of the stream.  The two expectations differ only where a draw of exactly 0 occurs,
    and every later draw of such a path moves with it."""
    from pbrpathtracer_amd import ptk
    assert ptk.scene_is_plain(refs.scenes["denormal"]) and not ptk.scene_is_lambert(refs.scenes["denormal"])
    assert ptk.scene_is_lambert(refs.scenes["minus zero"])
    for scene, level in (("denormal", "plain"), ("minus zero", "lambert")):
        ctx = _ctx(refs.scenes[scene], refs.cam, 8)
        try:
            for D in (3, 8):
                ctx.set_frame(W, H, D)
                got = _render(ctx)                 # default options: the predicate alone picks the level
                _ran(ctx, level)
                _same(got, refs.image(D, scene=scene), (scene, D))
        finally:
            ctx.close()


def test_an_empty_frame_returns_a_zero_image(refs):
    """every camera ray misses: no item is live, each wave finds its queues empty and retires (the main loop's termination case)"""
    assert not refs.live_pixels("away").any()
    ctx = _ctx(refs.arrays, refs.cams["away"], 8)
    try:
        for persistent in (1, 0):
            ctx.set_option("persistent", persistent)
            for level in ("lambert", "plain"):
                _select(ctx, level)
                acc, rgb = _render(ctx)
                _ran(ctx, level)
                assert not acc.any() and not rgb.any(), (persistent, level)
        _same((acc, rgb), refs.image(8, cam="away"), "oracle")
    finally:
        ctx.close()


def test_predicate_follows_a_material_update_and_its_undo(refs):
    ctx = _ctx(refs.arrays, refs.cam, 8)
    try:
        for scene, level in (("cornell", "lambert"), ("mirror", "plain"), ("cornell", "lambert"), ("denormal", "plain"),
                             ("minus zero", "lambert"), ("cornell", "lambert")):
            ctx.update_materials(refs.scenes[scene]["materials"])
            got = _render(ctx)
            _ran(ctx, level)
            _same(got, refs.image(8, scene=scene), (scene, level))
        assert not np.array_equal(refs.image(8, scene="mirror")[0], refs.image(8)[0])      # an edit the image shows
        # a new scene through ptk_upload_scene is seen as well, and the option holds the level back
        ctx.upload_scene(refs.scenes["mirror"])
        _same(_render(ctx), refs.image(8, scene="mirror"), "upload mirror"); _ran(ctx, "plain")
        ctx.upload_scene(refs.arrays)
        _same(_render(ctx), refs.image(8), "upload cornell"); _ran(ctx, "lambert")
        ctx.set_option("lambert_kernel", 0)
        _same(_render(ctx), refs.image(8), "option off"); _ran(ctx, "plain")
    finally:
        ctx.close()
