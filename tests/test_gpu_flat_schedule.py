"""The FLAT trace kernels' scheduling (csrc/ptk_kernels.hip, trace_kernel's main loop): a bounce ray that hits while the path's
next interaction would be the terminal one finishes the path at the end of the triangle pass (PTK_WALK_DONE), and work units are
dealt only when the deal can change which block the wave runs next.  Neither touches what a path computes - only which lane
traces which unit, and when - so every comparison here is against the oracle bit for bit, float accumulator and RGB8.

The cases put the terminal route at every position relative to the path start and to the Russian roulette (trace depths 0, 1, 2,
3 and 8), through both instantiations (PLAIN and the generic FLAT kernel), through materials where `iter` and `depth` part ways
(mirror / glossy bounces do not count as iterations), through textures, a normal map, stochastic opacity and a thin lens (the
camera-ray block joins the vote), and through every way the work reaches a wave: queues, one item per wave, a 3-way tile split,
several passes of one render, resumed sample ranges."""
import numpy as np
import pytest

from conftest import load_golden, scene_from_golden

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 64, 48, 8, 41
DEPTHS = (0, 1, 2, 3, 8)


def _cornell():
    z = load_golden("tier_s_cornell.npz")
    a = {k: np.array(v) for k, v in scene_from_golden(z).items()}
    rs = np.random.RandomState(5)
    a["uvs"] = rs.rand(len(a["verts"]), 6).astype(np.float32)
    cam = z["cam"]; proj = z["proj"]
    cam = dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]),
               focal_dist=float(z["focal_dist"]), aperture=0.0)
    return a, cam


def _textured(a, slots):
    """one 16x16 texture per slot (0 diffuse, 1 normal map, 2 emission, 3 roughness, 4 metalness, 5 opacity), on every material"""
    from pbrpathtracer_amd import ptk
    b = dict(a)
    rs = np.random.RandomState(9)
    b["texels"] = rs.randint(0, 256, len(slots) * 16 * 16 * 4).astype(np.uint8)
    b["textures"] = np.array([(16, 16, i * 16 * 16 * 4) for i in range(len(slots))], dtype=ptk.TEXTURE_DTYPE)
    b["materials"] = a["materials"].copy()
    for i, s in enumerate(slots):
        b["materials"]["tex"][:, s] = i
    return b


def _mirrors(a):
    """a perfect mirror, a glossy and a rough metal among the diffuse walls: specular bounces take `iter` back (pathtracer.cpp:626)"""
    b = dict(a); m = a["materials"].copy()
    m["reflectiveness"][0] = 1.0; m["roughness"][0] = 0.0
    m["reflectiveness"][1] = 0.7; m["roughness"][1] = 0.4
    m["reflectiveness"][2] = 0.5; m["roughness"][2] = 1.0
    b["materials"] = m
    return b


def _scene(name):
    a, cam = _cornell()
    if name == "cornell": return a, cam
    if name == "mirrors": return _mirrors(a), cam
    if name == "textures": return _textured(a, (0, 1, 2, 3, 4)), cam
    if name == "opacity": return _textured(a, (0, 5)), cam
    if name == "lens": return _mirrors(a), dict(cam, aperture=0.05)
    raise KeyError(name)


class _Ref:
    def __init__(self, OB, arrays, cam):
        self.o = OB.Oracle(arrays)
        self.cam = OB.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])
        self.OB = OB

    def render(self, D, first, spp, seed=SEED, w=W, h=H):
        return self.o.render(self.cam, w, h, D, first, spp, seed)

    def close(self):
        self.o.close()


def _ctx(arrays, cam, D, w=W, h=H):
    from pbrpathtracer_amd import ptk
    ctx = ptk.Context(0)
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(w, h, D); ctx.set_tile(0, 1)
    return ctx


def _render(ctx, spp=SPP, seed=SEED):
    ctx.reset(); ctx.render(0, spp, seed)
    return ctx.read_accum(), ctx.resolve_rgb8()


def _same(got, ref, label):
    assert np.array_equal(got[0], ref[0]), (label, "accumulator", int((got[0] != ref[0]).sum()))
    assert np.array_equal(got[1], ref[1]), (label, "rgb8", int((got[1] != ref[1]).sum()))


@pytest.mark.parametrize("scene", ["cornell", "mirrors"])
def test_terminal_route_at_every_depth_plain_and_generic(oracle_mod, scene):
    from pbrpathtracer_amd import ptk
    arrays, cam = _scene(scene)
    assert ptk.scene_is_plain(arrays)
    ref = _Ref(oracle_mod, arrays, cam)
    ctx = _ctx(arrays, cam, 8)
    try:
        lit = 0
        for D in DEPTHS:
            ctx.set_frame(W, H, D)
            want = ref.render(D, 0, SPP)
            lit += int((want[0] != 0).any())
            for plain, variant in ((1, ptk.TRACE_FLAT_PLAIN), (0, ptk.TRACE_FLAT)):
                ctx.set_option("plain_kernel", plain)
                got = _render(ctx)
                assert ctx.trace_variant() == variant
                _same(got, want, (scene, D, plain))
        assert lit >= len(DEPTHS) - 1              # (depth 0 is black: every path ends at its first interaction)
    finally:
        ctx.close(); ref.close()


@pytest.mark.parametrize("scene", ["textures", "opacity", "lens"])
def test_generic_flat_scenes_at_every_depth(oracle_mod, scene):
    """textures incl. a normal map (sampled by the terminal interaction too, before it ends the path: the image must not notice
    that the pass now skips it), an opacity texture (uncached camera rays pass PTK_WALK_DONE with iter = 0), a thin lens over
    mirrors (three blocks in the vote)"""
    from pbrpathtracer_amd import ptk
    arrays, cam = _scene(scene)
    ref = _Ref(oracle_mod, arrays, cam)
    ctx = _ctx(arrays, cam, 8)
    try:
        for D in DEPTHS:
            ctx.set_frame(W, H, D)
            want = ref.render(D, 0, SPP)
            got = _render(ctx)
            assert ctx.trace_variant() == ptk.TRACE_FLAT
            _same(got, want, (scene, D))
            if scene != "textures":                 # ... and with the other camera-ray route where the scene has two
                option = "lens_cull" if scene == "lens" else "primary_cache"
                ctx.set_option(option, 0)
                _same(_render(ctx), want, (scene, D, option))
                ctx.set_option(option, 1)
    finally:
        ctx.close(); ref.close()


@pytest.mark.parametrize("scene,plain", [("cornell", 1), ("cornell", 0), ("lens", 0)])
def test_every_way_work_reaches_a_wave(oracle_mod, scene, plain):
    arrays, cam = _scene(scene)
    D = 3
    ref = _Ref(oracle_mod, arrays, cam)
    want = ref.render(D, 0, SPP)
    ctx = _ctx(arrays, cam, D)
    defaults = {"persistent": -1, "generations": 0, "max_batch": 1, "chunk": 0}
    try:
        ctx.set_option("plain_kernel", plain)
        # one item per wave (no queues), with whole and with ragged chunks; queues forced on a small launch, batched pops
        for opts in ({"persistent": 0}, {"persistent": 0, "chunk": 3}, {"persistent": 1}, {"persistent": 1, "max_batch": 7},
                     {"persistent": 1, "generations": 3, "chunk": 2}):
            for k, v in {**defaults, **opts}.items():
                ctx.set_option(k, v)
            _same(_render(ctx), want, (scene, plain, opts))
        for k, v in defaults.items():
            ctx.set_option(k, v)
        # a 3-way tile split: the shares do not overlap and add up to the frame
        total = np.zeros_like(want[0])
        for r in range(3):
            ctx.set_tile(r, 3); ctx.reset(); ctx.render(0, SPP, SEED)
            part = ctx.read_accum()
            assert not np.any((part != 0) & (total != 0))
            total += part
        ctx.set_tile(0, 1)
        assert np.array_equal(total, want[0]), (scene, plain, "tiles")
        # several passes of one render: the smallest budget (1 MiB) holds 21 samples of this frame's 12 tiles
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        assert 2 ** 20 // (tiles * 4 * 64 * 16) < 48
        want48 = ref.render(D, 0, 48)
        ctx.set_option("pass_bytes", 2 ** 20)
        _same(_render(ctx, 48), want48, (scene, plain, "passes"))
        ctx.set_option("pass_bytes", 16 * 2 ** 30)
        # resumed sample ranges
        ctx.reset()
        for first, n in ((0, 5), (5, 1), (6, 42)):
            ctx.render(first, n, SEED)
        _same((ctx.read_accum(), ctx.resolve_rgb8()), want48, (scene, plain, "resumed"))
    finally:
        ctx.close(); ref.close()


def test_a_frame_smaller_than_a_wave(oracle_mod):
    """5 x 3 pixels, 1 and 70 samples: most lanes never get a unit, the wave must still retire"""
    arrays, cam = _scene("cornell")
    ref = _Ref(oracle_mod, arrays, cam)
    ctx = _ctx(arrays, cam, 2, 5, 3)
    try:
        for spp in (1, 70):
            for plain in (1, 0):
                ctx.set_option("plain_kernel", plain)
                _same(_render(ctx, spp), ref.render(2, 0, spp, w=5, h=3), (spp, plain))
    finally:
        ctx.close(); ref.close()


@pytest.mark.parametrize("scene", ["cornell", "textures", "lens"])
@pytest.mark.parametrize("D", [1, 3])
def test_stats_counters_of_flat_scenes_equal_the_oracle(oracle_mod, scene, D):
    """The STATS FLAT kernels deal lazily too, but park a terminal hit for the shade block as before (shade_lanes counts executed
    interactions): every exact counter is the oracle's, terminal interactions and the normal-map fetch they make included."""
    arrays, cam = _scene(scene)
    ref = _Ref(oracle_mod, arrays, cam)
    r = ref.o.render_counted(ref.cam, W, H, D, 0, SPP, SEED)
    c = r["counts"].reshape(W * H, -1)
    ctx = _ctx(arrays, cam, D)
    try:
        _same(_render(ctx), ref.render(D, 0, SPP), (scene, D))
        st = ctx.collect_stats(0, SPP, SEED)
    finally:
        ctx.close(); ref.close()
    cached = cam["aperture"] == 0.0
    all_miss = (c[:, 1] == c[:, 0]) & (c[:, 2] == 0) & (c[:, 3] == 0) & (c[:, 4] == 0)
    if cached:
        paths, walked_camera = int(c[~all_miss, 0].sum()), 0
    else:
        culled = W * H * SPP - st["paths_started"]
        assert culled >= 0 and culled % SPP == 0 and culled // SPP <= int(all_miss.sum())
        paths = walked_camera = W * H * SPP - culled
    assert st["samples"] == W * H * SPP
    assert st["paths_started"] == paths
    assert st["rays"] == int(c[:, 2:4].sum()) + walked_camera
    assert st["shadow_rays"] == int(c[:, 3].sum())
    assert st["hits_shaded"] == int(c[:, 4].sum())
    assert st["tex_fetches"] == int(c[:, 5].sum()) + int(c[:, 6].sum())
    assert st["shade_lanes"] == st["hits_shaded"] and st["shade_lanes"] <= 64 * st["shade_wave_execs"]
    assert st["walk_lane_iters"] == st["rays"] - st["shadow_rays"] and st["walk_lane_iters"] <= 64 * st["walk_wave_iters"]
    assert st["gen_lanes"] == (0 if cached else st["paths_started"])
    assert st["tri_tests"] == st["rays"] * len(arrays["verts"])
