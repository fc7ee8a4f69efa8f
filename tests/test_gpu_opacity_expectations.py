"""Stochastic opacity on the HIP path against exact float64 expectations (tests/opacity_cases.py): layer-stack fractions
through the FLAT kernel and the BVH walk, pinhole and thin lens, bit-exact edges, shadow rays through layers, a light with
its own opacity texture, and the independence of the per-pixel random streams.  Every scene is also checked against the
CPU oracle bit for bit at a smaller spp; tests/test_opacity_expectations_cpu.py runs the same cases on the oracle."""
import numpy as np
import pytest

import opacity_cases as OC

pytestmark = pytest.mark.gpu

W = H = 64
SPP = 256
PER_SAMPLE = 32


_open = []
_shared = {}


@pytest.fixture(autouse=True)
def _close_tracers():
    """A failing assertion skips a test's own close() calls: every PathTracer it opened is closed here, so none outlives it."""
    yield
    while _open:
        _open.pop().close()


@pytest.fixture(scope="module", autouse=True)
def _one_context():
    """The whole module renders through ONE ptk context: each scene is uploaded into it when it is used."""
    yield
    c = _shared.pop("ctx", None)
    _shared.pop("bound", None)
    if c is not None:
        c.close()


class Gpu:
    """A scene on the module's ptk context; `options` are ptk_set_option pairs (flat 0: the BVH walk even for <= 16
    triangles), applied over the defaults whenever this scene is (re)bound."""
    DEFAULTS = dict(flat=1, contract=0)

    def __init__(self, built, **options):
        self.built = built
        self.options = {**self.DEFAULTS, **options}
        self.staged = OC.staged(built)
        self.cam = OC.camera(built)

    def _bind(self):
        from pbrpathtracer_amd import ptk
        if "ctx" not in _shared:
            _shared["ctx"] = ptk.Context(0)
        c = _shared["ctx"]
        if _shared.get("bound") is not self:
            for k, v in self.options.items():
                c.set_option(k, v)
            c.upload_scene(self.staged)
            cam = self.cam
            c.set_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])
            c.set_frame(self.built.width, self.built.height, self.built.depth)
            _shared["bound"] = self
        return c

    def __call__(self, b, first, spp, seed):
        assert b is self.built
        c = self._bind()
        c.reset()
        c.render(first, spp, seed)
        return c.read_accum()

    def close(self):
        if _shared.get("bound") is self:
            _shared["bound"] = None


def _matches_oracle(OB, g: Gpu, spp=4, seed=5):
    o, cam = OC.oracle(OB, g.built)
    b = g.built
    ref, _ = o.render(cam, b.width, b.height, b.depth, 0, spp, seed, want_rgb8=False)
    assert np.array_equal(g(b, 0, spp, seed), ref), "GPU accumulator differs from the oracle"


KERNELS = [dict(), dict(flat=0)]            # FLAT kernel (<= 16 triangles), BVH walk
KERNEL_IDS = ["flat", "bvh"]


@pytest.mark.parametrize("opts", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("stack", sorted(OC.STACKS))
def test_layer_stack_fractions(tmp_path, oracle_mod, stack, lens, opts):
    built, ps = OC.stack_scene(str(tmp_path), stack, W, H, lens=lens)
    g = Gpu(built, **opts)
    _matches_oracle(oracle_mod, g)
    zs = OC.check_stack(g, built, ps, SPP)
    print(stack, lens, opts, {k: round(float(v), 2) for k, v in zs.items()})
    g.close()


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
def test_layer_stack_behind_padding(tmp_path, oracle_mod, lens):
    """> 16 triangles (off-screen padding before the layers): the BVH kernels without any option."""
    built, ps = OC.stack_scene(str(tmp_path), "a", W, H, lens=lens, pad=16)
    g = Gpu(built)
    _matches_oracle(oracle_mod, g)
    OC.check_stack(g, built, ps, SPP)
    g.close()


@pytest.mark.parametrize("stack", sorted(OC.STACKS))
def test_layer_stack_fractions_contract2(tmp_path, stack):
    """contract 2 (fused multiply-adds, 1-ulp reciprocal / square root) changes the arithmetic, not the decisions: with 1x1
    textures no draw depends on uv arithmetic, so the same exact fractions hold."""
    for opts in KERNELS:
        built, ps = OC.stack_scene(str(tmp_path), stack, W, H)
        g = Gpu(built, contract=2, **opts)
        OC.check_stack(g, built, ps, SPP)
        g.close()


@pytest.mark.parametrize("opts", KERNELS, ids=KERNEL_IDS)
def test_exact_edges(tmp_path, oracle_mod, opts):
    d = str(tmp_path)
    plain = Gpu(OC.edge_scene(d, "none", None, W, H, with_layers=False), **opts)
    opaque = Gpu(OC.edge_scene(d, "opaque", None, W, H), **opts)
    want_plain, want_opaque = plain(plain.built, 0, 16, 3), opaque(opaque.built, 0, 16, 3)
    assert not np.array_equal(want_plain, want_opaque)
    _matches_oracle(oracle_mod, plain); _matches_oracle(oracle_mod, opaque)
    # texel 0 (and only red counts: green / blue / alpha full) is invisible; texel 255 (red full, the rest 0) is opaque
    for name, op, want in [("t0", 0, want_plain), ("t255", 255, want_opaque),
                           ("gb_ppm", (0, 255, 255), want_plain), ("r_ppm", (255, 0, 0), want_opaque),
                           ("gba_tga", (0, 255, 255, 255), want_plain), ("r_tga", (255, 0, 0, 0), want_opaque)]:
        g = Gpu(OC.edge_scene(d, name, op, W, H), **opts)
        assert np.array_equal(g(g.built, 0, 16, 3), want), name
        _matches_oracle(oracle_mod, g)
        g.close()
    plain.close(); opaque.close()


@pytest.mark.parametrize("opts", KERNELS, ids=KERNEL_IDS)
def test_uv_at_the_candidate(tmp_path, oracle_mod, opts):
    b = OC.uv_split_scene(str(tmp_path), W, H)
    o, cam = OC.oracle(oracle_mod, b)
    u = OC.uv_of_candidate(OC.staged(b), b.layer_tris[0], cam.pos[:], o.primary_dirs(cam, W, H).reshape(-1, 3)).reshape(H, W)
    g = Gpu(b, **opts)
    acc = g(b, 0, 16, 9)
    see, block = u < 0.5 - 1e-3, u > 0.5 + 1e-3
    assert see.sum() > 0.1 * W * H and block.sum() > 0.1 * W * H
    assert np.all(acc[see] == [0, 0, 16]) and np.all(acc[block] == [16, 0, 0])
    _matches_oracle(oracle_mod, g)
    g.close()


@pytest.mark.parametrize("opts", KERNELS, ids=KERNEL_IDS)
def test_shadow_rays_through_layers(tmp_path, oracle_mod, opts):
    texels = (77, 128, 1)
    p = OC.through_all([OC.p_accept(x) for x in texels])
    plain = Gpu(OC.shadow_scene(str(tmp_path), "plain", [], W, H), **opts)
    layered = Gpu(OC.shadow_scene(str(tmp_path), "layered", texels, W, H), **opts)
    _matches_oracle(oracle_mod, layered)
    for seed in OC.SEEDS:
        z = OC.check_shadow_pairs(OC.per_sample(plain, plain.built, PER_SAMPLE, seed),
                                  OC.per_sample(layered, layered.built, PER_SAMPLE, seed), p, f"seed {seed}")
        print(opts, seed, round(z, 2))
    plain.close(); layered.close()


@pytest.mark.parametrize("opts", KERNELS, ids=KERNEL_IDS)
def test_light_with_its_own_opacity(tmp_path, oracle_mod, opts):
    d = str(tmp_path)
    b0 = Gpu(OC.shadow_scene(d, "l0", [], W, H), **opts)
    b1 = Gpu(OC.shadow_scene(d, "l1", [], W, H, light_opacity=128), **opts)
    w0 = Gpu(OC.shadow_scene(d, "w0", [], W, H, wall_behind_light=True), **opts)
    w1 = Gpu(OC.shadow_scene(d, "w1", [], W, H, light_opacity=128, wall_behind_light=True), **opts)
    _matches_oracle(oracle_mod, b1); _matches_oracle(oracle_mod, w1)
    for seed in OC.SEEDS:
        # nothing behind the light: a rejected light lets the shadow ray go on, and finding nothing means lit
        assert np.array_equal(b0(b0.built, 0, 16, seed), b1(b1.built, 0, 16, seed))
        # a wall behind it: lit exactly when the light's one draw accepts (a second chance would give 1 - (1 - P)^2)
        OC.check_shadow_pairs(OC.per_sample(w0, w0.built, PER_SAMPLE, seed),
                              OC.per_sample(w1, w1.built, PER_SAMPLE, seed), OC.p_accept(128), f"seed {seed}")
    for g in (b0, b1, w0, w1):
        g.close()


@pytest.mark.parametrize("opts", KERNELS, ids=KERNEL_IDS)
def test_stream_independence(tmp_path, opts):
    """Count images of seeds s and s + 1, of s and s + 2^32 (through ptk_render and through PathTracer::SetSeed), and of the
    sample ranges [0, N) and [N, 2N) are uncorrelated."""
    from pbrpathtracer_amd.pathtracer import PathTracer
    built, _ = OC.stack_scene(str(tmp_path), "a", W, H)
    g = Gpu(built, **opts)
    pt = PathTracer(0)
    _open.append(pt)
    pt.LoadSceneFile(built.pts)
    pt.SetCameraAperture(0.0)
    for k, v in opts.items():
        pt.context().set_option(k, v)
    for s in OC.SEEDS:
        a = g(built, 0, SPP, s)
        pairs = [("seed + 1", g(built, 0, SPP, s + 1)), ("seed + 2^32", g(built, 0, SPP, s + 2 ** 32)),
                 ("next sample range", g(built, SPP, SPP, s))]
        accs = []
        for seed in (s, s + 2 ** 32):
            pt.ResetImage(); pt.SetSeed(seed); pt.RenderFrames(SPP)
            assert pt.LastError() == ""
            accs.append(pt.ReadAccumulation())
        assert np.array_equal(accs[0], a)
        pairs.append(("SetSeed(seed + 2^32)", accs[1]))
        for what, b in pairs:
            for c in range(3):
                OC.assert_uncorrelated(a[..., c], b[..., c], f"seed {s} vs {what}, channel {c}")
    pt.close(); g.close()


@pytest.mark.parametrize("opts", KERNELS, ids=KERNEL_IDS)
def test_shadow_and_bounce_draws_are_independent(tmp_path, oracle_mod, opts):
    """The shadow ray (ray number `ray`) and the bounce (`ray + 1`) of one sample cross the same layer; in the FLAT kernel
    they go through tri_test_pair together.  Their two draws must be independent: joint rate (1 - P) P."""
    d = str(tmp_path)
    p = OC.p_accept(128)
    plain = Gpu(OC.joint_scene(d, "plain", None, W, H, with_layer=False), **opts)
    opaque = Gpu(OC.joint_scene(d, "opaque", None, W, H), **opts)
    layered = Gpu(OC.joint_scene(d, "layered", 128, W, H), **opts)
    _matches_oracle(oracle_mod, layered)
    for seed in OC.SEEDS:
        A, B, C = (OC.per_sample(g, g.built, PER_SAMPLE, seed) for g in (plain, opaque, layered))
        print(opts, seed, {k: round(v, 2) for k, v in OC.check_joint(A, B, C, p, f"seed {seed}").items()})
    for g in (plain, opaque, layered):
        g.close()
