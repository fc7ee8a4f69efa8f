"""The contracted builds of the trace kernels (ptk_set_option "contract" 1: -ffp-contract=fast; 2: ... with the hardware's
v_rcp / v_sqrt / v_rsq) held SAMPLE BY SAMPLE to the exact kernels, and to reproducibility bit for bit.

tests/test_gpu_contract.py bounds the RMSE of the mean image, which averages a per-sample error away: a contracted-only bias of a
few 1e-4 on every diffuse bounce, or a wrong rare branch (total internal reflection, normal maps facing away, lens sampling),
would pass it.  Here every sample of every pixel is rendered on its own (reset; render(s, 1, seed); read_accum) with the exact
build and with both contracted builds, over a matrix of scenes: the tier S goldens (FLAT kernel, pinhole and lens cameras,
opacity textures), seeded random scenes of 9 / 16 triangles (FLAT), 300 (host-built BVH) and 6000 (device-built BVH), the
degenerate no-light scene, depths 1 / 2 / 12, a ragged frame, and three controls of one textured scene.  Per channel, with e the
exact sample and g the contracted one:

  * g is finite wherever e is;
  * g agrees with e when |g - e| <= 1e-4 max(|e|, |g|) + 1e-6; at most a fraction D_MAX of the samples may disagree (a path
    whose branch decision or hit flips on a last-bit difference takes another route: such samples are rare, not small);
  * over the agreeing samples the contracted build is unbiased: |sum(g - e)| <= BETA sum|e|.

The sum of the exact samples is, once per case, the oracle's accumulator bit for bit (the anchor).

Measured on gfx950 (the ENVELOPE lines this module prints, 16 cases x 2 levels, largest over the channels): 71-100 % of the
samples bit-identical; disagreeing 0 ... 7.5e-4 (glass at depth 12: 4.0e-4; random6000_device_tex: 7.5e-4; random300_host_tex
with its noise textures tamed: 7.4e-4), and 1.2e-3 ... 8.3e-3 in the scenes of noise textures used as normal maps
(NOISE_TEXTURES); bias 0 ... 2.1e-8 (opacity_lens, level 2).  D_MAX = 1e-3 (1.3x the largest), D_NOISE_TEXTURES = 1.2e-2
(1.45x), BETA = 8e-8 (3.8x).  A factor (1 + 2^-16) on the contracted builds' diffuse bounce weight gives a bias of
1.0e-5 ... 1.4e-5 here; with (1 + 2^-12) 11 of the first 13 cases fail, while tests/test_gpu_contract.py still passes.

The contracted builds are also deterministic: for a FLAT, a host-BVH and a device-BVH scene, the accumulator does not depend on
how work reaches the lanes, on passes, on launch splits, on tile shares or on the lens cull (for a camera where it does cull
pixels) - the promise INTEGRATION.md makes for a seed holds at every contract level."""
import numpy as np
import pytest

from conftest import load_golden, scene_from_golden
from test_gpu_edge_cases import _cam as golden_cam, no_lights_degenerate_scene
from test_gpu_random_scenes import random_scene

pytestmark = pytest.mark.gpu

D_MAX = 1e-3            # fraction of the samples (per channel) that may disagree; largest measured 7.5e-4
D_NOISE_TEXTURES = 1.2e-2  # ... in the scenes of noise textures used as normal maps (NOISE_TEXTURES below); largest measured 8.3e-3
BETA = 8e-8             # relative bias over the agreeing samples; largest measured 2.1e-8
REL, ABS = 1e-4, 1e-6
SEED = 9
DEFAULTS = {"persistent": -1, "generations": 0, "max_batch": 1, "chunk": 0, "tri_threshold": 6, "lens_cull": 1,
            "pass_bytes": float(16 << 30)}


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def _golden(name, aperture=None):
    z = load_golden(name)
    return scene_from_golden(z), golden_cam(z, aperture)


# name -> (scene factory, width, height, depth)
CASES = {
    "cornell_pinhole": (lambda: _golden("tier_s_cornell.npz", 0.0), 64, 48, 5),
    "glass": (lambda: _golden("tier_s_glass.npz"), 64, 48, 5),
    "opacity_lens": (lambda: _golden("tier_s_opacity.npz"), 64, 48, 5),
    "random9_flat": (lambda: random_scene(11, 9, False), 64, 48, 7),
    "random16_flat_tex": (lambda: random_scene(12, 16, True), 64, 48, 7),
    "random300_host": (lambda: random_scene(15, 300, False), 64, 48, 7),
    "random300_host_tex": (lambda: random_scene(14, 300, True), 64, 48, 7),
    "random6000_device_tex": (lambda: random_scene(16, 6000, True), 64, 48, 7),
    "no_lights_degenerate": (no_lights_degenerate_scene, 64, 48, 6),
    "glass_depth1": (lambda: _golden("tier_s_glass.npz"), 64, 48, 1),
    "glass_depth2": (lambda: _golden("tier_s_glass.npz"), 64, 48, 2),
    "glass_depth12": (lambda: _golden("tier_s_glass.npz"), 64, 48, 12),
    "opacity_ragged_37x23": (lambda: _golden("tier_s_opacity.npz"), 37, 23, 5),
    "random300_host_tex_uniform": (lambda: _tamed(*random_scene(14, 300, True), uniform=True, upright=False), 64, 48, 7),
    "random300_host_tex_upright": (lambda: _tamed(*random_scene(14, 300, True), uniform=False, upright=True), 64, 48, 7),
    "random300_host_tex_uniform_upright": (lambda: _tamed(*random_scene(14, 300, True), uniform=True, upright=True), 64, 48, 7),
}
# random_scene's textures are noise (every texel drawn on its own) stretched over up to four repeats per triangle, and any of
# them may serve as a normal map.  Two things then turn a last-bit difference into another path: a hit's texture coordinate
# crosses a texel edge now and then (another colour, normal or opacity from there on), and a normal-map texel whose third byte is
# below 128 lays the shading normal into the surface (nt.z <= 0 -> EPS), where the bounce and the EPS offset graze the triangle.
# The controls take them out of random300_host_tex one at a time, the same geometry, materials and lookups (measured, largest
# level): uniform textures 1.4e-3, upright normal maps 1.2e-3, both 7.4e-4 - the last held to D_MAX like every other case.
NOISE_TEXTURES = ("random16_flat_tex", "random300_host_tex", "random300_host_tex_uniform", "random300_host_tex_upright")
S = 32


def _tamed(arrays, cam, uniform, upright):
    """random_scene's textures with every texel of a texture set to its first one (uniform: no texel edge to cross) and / or
    with every texel's third byte raised to >= 200 (upright: a normal map tilts the shading normal by at most 55 degrees)"""
    a = dict(arrays); tx = a["texels"].copy().reshape(-1, 4)
    if uniform:
        for w, h, off in a["textures"][["width", "height", "offset"]].tolist():
            tx[off // 4: off // 4 + w * h] = tx[off // 4]
    if upright:
        tx[:, 2] = np.maximum(tx[:, 2], 200)
    a["texels"] = tx.reshape(-1)
    return a, cam


def _setup(ctx, arrays, cam, W, H, D):
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(0, 1)


def _per_sample(ctx, level, n, seed):
    ctx.set_option("contract", level)
    out = np.empty((n, ctx.height, ctx.width, 3), np.float32)
    for s in range(n):
        ctx.reset(); ctx.render(s, 1, seed); out[s] = ctx.read_accum()
    return out


def envelope(e, g):
    """per channel: (bit-identical fraction, disagreeing fraction, disagreements, largest relative error among the agreeing
    samples, relative bias over the agreeing samples); asserts g finite wherever e is"""
    rows = []
    for ch in range(3):
        e32, g32 = e[..., ch].reshape(-1), g[..., ch].reshape(-1)
        fin = np.isfinite(e32)
        assert np.isfinite(g32[fin]).all(), f"channel {ch}: the contracted build is not finite where the exact one is"
        e32, g32 = e32[fin], g32[fin]
        ed, gd = e32.astype(np.float64), g32.astype(np.float64)
        ad, mx = np.abs(gd - ed), np.maximum(np.abs(ed), np.abs(gd))
        agree = ad <= REL * mx + ABS
        n_dis = int((~agree).sum())
        rel = ad[agree] / np.where(mx[agree] > 0, mx[agree], 1.0)
        s_abs, s_dif = float(np.abs(ed[agree]).sum()), float((gd[agree] - ed[agree]).sum())
        bias = abs(s_dif) / s_abs if s_abs > 0 else (0.0 if s_dif == 0 else np.inf)
        rows.append((float(np.mean(e32 == g32)), n_dis / max(1, e32.size), n_dis, float(rel.max()) if rel.size else 0.0, bias))
    return rows


@pytest.mark.parametrize("case", list(CASES))
def test_contracted_samples_stay_in_the_envelope(ctx, oracle_mod, case):
    make, W, H, D = CASES[case]
    arrays, cam = make()
    _setup(ctx, arrays, cam, W, H, D)
    try:
        exact = _per_sample(ctx, 0, S, SEED)
        # anchor: the exact samples, summed in sample order as the accumulate kernel does, are the oracle's accumulator
        o = oracle_mod.Oracle(arrays)
        ocam = oracle_mod.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])
        ref, _ = o.render(ocam, W, H, D, 0, S, SEED, want_rgb8=False)
        o.close()
        acc = np.zeros((H, W, 3), np.float32)
        for s in range(S):
            acc += exact[s]
        assert np.array_equal(acc, ref), case
        assert acc.any() == (case != "no_lights_degenerate")
        per_level = {level: envelope(exact, _per_sample(ctx, level, S, SEED)) for level in (1, 2)}
        d_max = D_NOISE_TEXTURES if case in NOISE_TEXTURES else D_MAX
        for level, rows in per_level.items():
            bit = min(r[0] for r in rows); dis = max(r[1] for r in rows); n_dis = sum(r[2] for r in rows)
            rel = max(r[3] for r in rows); bias = max(r[4] for r in rows)
            print(f"ENVELOPE {case:34s} contract={level}: bit-identical {bit:.4f}, disagreeing {dis:.2e} (bound {d_max:.1e}), "
                  f"{n_dis} of {3 * exact[..., 0].size}, max rel error (agreeing) {rel:.2e}, bias {bias:.2e} (bound {BETA:.1e})")
        for level, rows in per_level.items():
            for ch, r in enumerate(rows):
                assert r[1] <= d_max, (case, level, ch, r)
                assert r[4] <= BETA, (case, level, ch, r)
    finally:
        ctx.set_option("contract", 0)


# ---- reproducibility -------------------------------------------------------------------------------------------------------
MODES = ({"persistent": 1}, {"persistent": 0}, {"persistent": 1, "max_batch": 7}, {"persistent": 1, "generations": 3, "chunk": 2},
         {"persistent": 1, "chunk": 24}, {"persistent": 0, "chunk": 3}, {"persistent": 1, "tri_threshold": 0},
         {"persistent": 1, "tri_threshold": 64})                 # test_work_distribution_modes_agree's option sets
REPRO = {
    "flat": lambda: _golden("tier_s_cornell.npz", 0.0),
    "host_bvh": lambda: random_scene(14, 300, True),
    "device_bvh": lambda: random_scene(16, 6000, True),
}


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("case", list(REPRO))
def test_contracted_renders_are_reproducible(ctx, case, level):
    arrays, cam = REPRO[case]()
    W, H, D, N = 64, 48, 5, 8
    _setup(ctx, arrays, cam, W, H, D)
    ctx.set_option("contract", level)

    def render(first=0, spp=N, reset=True):
        if reset:
            ctx.reset()
        ctx.render(first, spp, SEED)
        return ctx.read_accum()

    try:
        base = render()
        assert base.any() and np.isfinite(base).all()
        assert np.array_equal(render(), base), "the same render twice"
        for opts in MODES:
            for k, v in {**DEFAULTS, **opts}.items():
                ctx.set_option(k, v)
            assert np.array_equal(render(), base), opts
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)
        # several passes through a small sample buffer (1 MiB holds 20 samples of this frame at chunk 5)
        many = render(0, 40)
        ctx.set_option("pass_bytes", 1 << 20); ctx.set_option("chunk", 5)
        assert np.array_equal(render(0, 40), many), "pass_bytes 1 MiB, chunk 5"
        ctx.set_option("pass_bytes", DEFAULTS["pass_bytes"]); ctx.set_option("chunk", 0)
        # one launch of N samples = N launches of one sample
        ctx.reset()
        for s in range(N):
            ctx.render(s, 1, SEED)
        assert np.array_equal(ctx.read_accum(), base), "N launches of one sample"
        # tile shares under persistent waves: disjoint, summing to the whole frame
        ctx.set_option("persistent", 1); ctx.set_option("generations", 2)
        total = np.zeros_like(base)
        for r in range(3):
            ctx.set_tile(r, 3)
            part = render()
            assert not np.any((part != 0) & (total != 0))
            total += part
        assert np.array_equal(total, base), "tile shares"
        ctx.set_tile(0, 1); ctx.set_option("persistent", -1); ctx.set_option("generations", 0)
        # the lens cull on a thin-lens camera that sees the scene's box in the middle of the frame only (three extents back,
        # 60 degrees): the cull must leave pixels untraced, and the image must not notice
        v = arrays["verts"].reshape(-1, 3).astype(np.float64)
        centre = (v.min(axis=0) + v.max(axis=0)) / 2
        reach = 3.0 * float(np.abs(v - centre).max())
        d = np.asarray(cam["dir"], np.float64)
        ctx.set_camera(**{**cam, "pos": (centre - d * reach).astype(np.float32), "fovy": 60.0, "focal_dist": reach, "aperture": 0.08})
        culled = render()
        traced = ctx.collect_stats(0, N, SEED)["rays"]
        ctx.set_option("lens_cull", 0)
        assert np.array_equal(render(), culled) and culled.any(), "lens_cull 0 / 1"
        assert ctx.collect_stats(0, N, SEED)["rays"] > traced, "the cull removed no pixel: the check would be vacuous"
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)
        ctx.set_tile(0, 1)
        ctx.set_option("contract", 0)
