"""The golden scenes of the registry (tests/trace_arms.py golden_scenes: every fixture the oracle is pinned to the reference on), and
the arms of Trace that no golden, random or plain-frame scene takes (tests/trace_edge_cases.py; the census of
tests/test_trace_arms_cpu.py shows that these scenes take them): Russian roulette's cap, both clamps of tex2d in all six slots,
the band of |n.x| between the two sampler thresholds, texels of exactly 0 and 1, exact ties - each scene under every trace kernel
it admits, asserted through ptk_trace_variant, every accumulator word == the CPU oracle's.  The texture edges also through the
feature planes (against answers written down in the helper), and through ptk_intersect_rays / ptk_occluded_rays (against
tests/hit_rule.py); the bright walls also through ptk_trace_rays and a lightmap bake, whose kernel runs the same shade."""
import numpy as np
import pytest

import bake_cases as BC
import feature_truth as FT
import hit_rule as HR
import ray_cases as RC
import trace_arms as TA
import trace_edge_cases as TE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def edge_scenes():
    return {s[0]: s for s in TA.edge_scenes()}


def _ocam(OB, cam):
    return OB.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _defaults(ctx):
    ctx.set_option("flat", 1); ctx.set_option("plain_kernel", 1); ctx.set_option("device_build", 1)


def _set_variant(ctx, arrays, variant, device_build):
    """the options that send `arrays` down `variant`; the caller asserts ptk_trace_variant after the render"""
    small = len(arrays["verts"]) <= 16
    ctx.set_option("flat", 0 if (variant == "BVH" and small) else 1)
    ctx.set_option("plain_kernel", 1 if variant == "PLAIN" else 0)
    ctx.set_option("device_build", device_build)


def _variant_id(name):
    from pbrpathtracer_amd import ptk
    return {"PLAIN": ptk.TRACE_FLAT_PLAIN, "FLAT": ptk.TRACE_FLAT, "BVH": ptk.TRACE_BVH}[name]


def _check_scene(ctx, OB, scene):
    """the scene under every kernel it admits (a tree built on the host and on the device) == the oracle; returns the renders done"""
    name, arrays, cam, W, H, D, spp, seed, variants = scene
    o = OB.Oracle(arrays)
    ref, ref8 = o.render(_ocam(OB, cam), W, H, D, 0, spp, seed)
    o.close()
    done = 0
    try:
        for variant in variants:
            for device_build in ((0, 1) if variant == "BVH" else (1,)):
                _set_variant(ctx, arrays, variant, device_build)
                ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(0, 1); ctx.reset()
                ctx.render(0, spp, seed)
                got, got8 = ctx.read_accum(), ctx.resolve_rgb8()
                assert ctx.trace_variant() == _variant_id(variant), (name, variant, device_build, ctx.trace_variant())
                bad = int((got.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())
                assert bad == 0, (name, variant, device_build, f"{bad} pixels differ")
                assert np.array_equal(got8, ref8), (name, variant, device_build)
                done += 1
    finally:
        _defaults(ctx)
    return done


def _group(edge_scenes, prefix):
    return [s for n, s in edge_scenes.items() if n.startswith(prefix)]


# ---- the golden scenes: every scene on which a tape pins the oracle to the reference -----------------------------------------------
@pytest.fixture(scope="module")
def golden_scenes():
    return {s[0]: s + (TA.variants_admitted(s[1], s[2]),) for s in TA.golden_scenes()}


@pytest.mark.parametrize("name", [s[0] for s in TA.golden_scenes()])
def test_golden_scene_renders(ctx, oracle_mod, golden_scenes, name):
    """the lens and the pinhole entry of every tier_s_* / tier_f_* fixture (tests/trace_arms.py golden_scenes), as registered: 64 x 48,
    the fixture's depth, 8 samples - under every kernel the scene admits"""
    scene = golden_scenes[name]
    assert scene[3:5] + scene[6:8] == TA.GOLDEN_FRAME
    assert _check_scene(ctx, oracle_mod, scene) == {"PLAIN": 4, "FLAT": 3, "BVH": 2}[scene[8][0]]


# ---- renders ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "textured", "padded", "glass"])
def test_rr_cap_renders(ctx, oracle_mod, edge_scenes, kind):
    group = _group(edge_scenes, f"rr_cap_{kind}_")
    assert len(group) == 3
    n = sum(_check_scene(ctx, oracle_mod, s) for s in group)
    assert n == 3 * {"plain": 4, "textured": 3, "padded": 2, "glass": 3}[kind]


@pytest.mark.parametrize("slot", TE.SLOTS)
def test_tex_edges_renders(ctx, oracle_mod, edge_scenes, slot):
    group = [s for n, s in edge_scenes.items() if n.startswith("tex_edges_") and f"_{slot}_" in n]
    assert len(group) == 3 * len(TE.TEX_SIZES)
    for s in group:
        _check_scene(ctx, oracle_mod, s)


@pytest.mark.parametrize("prefix,count", [("tex_missing", 2), ("sampler_band_", len(TE.BAND_MATERIALS) + 2), ("exact_texture_values_", 3),
                                          ("render_ties_", 3), ("no_lights", 1), ("lost_light", 1)])
def test_other_edge_scene_renders(ctx, oracle_mod, edge_scenes, prefix, count):
    group = _group(edge_scenes, prefix)
    assert len(group) == count
    for s in group:
        _check_scene(ctx, oracle_mod, s)


def test_a_tie_shows_the_smaller_index(ctx, oracle_mod):
    """what the tie rule means in a picture: of two coincident emitters the one with the smaller index is seen - red in the even pairs,
    green in the odd ones - and the twin, which has the larger index, never is"""
    from pbrpathtracer_amd import ptk
    arrays, cam = TE.render_ties(6, others=3, rotate=False)        # exact copies: every hit of a pair is a tie
    try:
        for variant in ("PLAIN", "FLAT", "BVH"):
            _set_variant(ctx, arrays, variant, 1)
            ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(TE.W, TE.H, 3); ctx.set_tile(0, 1); ctx.reset()
            ctx.render(0, 1, 3)                                  # depth 3: no Russian roulette at the first hit
            acc = ctx.read_accum()
            assert ctx.trace_variant() == _variant_id(variant)
            ctx.render_features(1 << ptk.FEAT_TRIANGLE)
            tri = ctx.read_feature(ptk.FEAT_TRIANGLE)
            seen = set(np.unique(tri[tri >= 0]).tolist())
            assert set(range(6)) <= seen and not (seen & set(range(9, 15))), (variant, seen)
            for k in range(6):
                px = acc[tri == k]
                assert len(px) and ((px[:, 0] > px[:, 1]) == (k % 2 == 0)).all(), (variant, k)
    finally:
        _defaults(ctx)


# ---- the bright walls through the ray query and the bake ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "textured", "padded", "glass"])
def test_rr_cap_through_trace_rays_and_a_bake(ctx, oracle_mod, kind):
    arrays, cam = TE.rr_cap(kind)
    o = oracle_mod.Oracle(arrays)
    try:
        ctx.upload_scene(arrays)
        ro, rd = RC.rays_in_box(arrays, 160, 5)
        for D in (1, 2, 3):
            got = ctx.trace_rays(ro, rd, D, 0, 3, 41, key_base=7)
            want = RC.truth(o, ro, rd, D, 41, 0, 3, key_base=7)
            assert want.any() and _same(got, want), (kind, D, int((got != want).any(axis=1).sum()))
        from pbrpathtracer_amd.lightmap import grid_atlas
        n = len(arrays["verts"])
        uvs = np.zeros((n, 6), np.float32); uvs[:12] = grid_atlas(12, 24, 16, 1)
        off = BC.offset_of(arrays)
        got, owner = ctx.bake_lightmap(24, 16, off, 2, 0, 3, 43, uvs=uvs)
        want, want_owner = BC.truth_bake(o, arrays, uvs, 24, 16, off, 2, 43, 0, 3)
        assert np.array_equal(owner, want_owner) and (owner >= 0).sum() > 100
        assert want.any() and _same(got, want), kind
    finally:
        o.close()


# ---- texture edges: the feature planes against written-down answers ----------------------------------------------------------------
def _known_planes(ctx, oracle_mod, slot, size, feature, channels, scale=1.0):
    """render the feature planes of tex_edges(slot, size, "uv") and compare `feature` on every panel pixel with the texel the table of
    trace_edge_cases.SPECIALS names; everything else with the oracle (feature_truth)"""
    from pbrpathtracer_amd import ptk
    w, h = size
    arrays, cam, names = TE.tex_edges(slot, size, "uv")
    img = TE.edge_texture(w, h, slot).astype(np.float32) / np.float32(255)
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(TE.W, TE.H, 2); ctx.set_tile(0, 1); ctx.reset()
    ctx.render_features(ptk.FEAT_ALL, 0, TE.SEED)
    tri = ctx.read_feature(ptk.FEAT_TRIANGLE)
    plane = ctx.read_feature(feature)
    want = FT.truth(oracle_mod, arrays, cam, TE.W, TE.H, TE.SEED, 0)
    for f, nm in enumerate(ptk.FEAT_NAMES):
        assert FT.planes_equal(ctx.read_feature(f), want[nm]), (TE.SLOTS[slot], size, nm)
    if not channels:
        return 0
    plain_col, plain_row = int(0.3 * w), int(0.3 * h)
    checked = 0
    for k, (axis, name) in enumerate(names):
        px = plane[tri == k][:, :len(channels)] if plane.ndim == 3 else plane[tri == k][:, None]
        assert len(px) >= 4, (k, axis, name)
        n = w if axis == "u" else h
        cols = [TE.special_texel(name, n)] if name in TE.STABLE or n == 1 else sorted({0, n - 1, TE.special_texel(name, n)})
        if name == "0.5" and n % 2 == 0:
            cols = [n // 2 - 1, n // 2]
        texels = [img[plain_row, c] if axis == "u" else img[c, plain_col] for c in cols]
        ok = np.zeros(len(px), bool)
        for t in texels:
            ok |= (px == (t[list(channels)] * np.float32(scale))[None, :]).all(axis=1)
        assert ok.all(), (TE.SLOTS[slot], size, axis, name, cols, px[~ok][:2])
        checked += len(px)
    return checked


@pytest.mark.parametrize("size", TE.TEX_SIZES)
def test_tex_edges_feature_planes_hold_the_known_texels(ctx, oracle_mod, size):
    from pbrpathtracer_amd import ptk
    assert _known_planes(ctx, oracle_mod, 0, size, ptk.FEAT_ALBEDO, (0, 1, 2)) >= 300
    assert _known_planes(ctx, oracle_mod, 2, size, ptk.FEAT_EMISSION, (0, 1, 2)) >= 300
    assert _known_planes(ctx, oracle_mod, 3, size, ptk.FEAT_GLOSS, (0,)) >= 300          # gloss = (roughness, reflectiveness)
    _known_planes(ctx, oracle_mod, 1, size, ptk.FEAT_NORMAL, ())                        # the normal slot: all planes == the oracle


# ---- texture edges: the opacity fetch of the ray queries -----------------------------------------------------------------------------
@pytest.mark.parametrize("size", TE.TEX_SIZES)
def test_tex_edges_opacity_through_the_hit_queries(ctx, oracle_mod, size):
    """rays at the panels of the opacity-mapped scene: edge texels hold 0 and 255, so a wrong texel turns a hit into a miss"""
    rng = np.random.default_rng(3)
    for axis, pad in (("u", 0), ("uv", 0)):                      # 16 triangles: the FLAT-sized scene; 33: a tree
        arrays, cam, names = TE.tex_edges(5, size, axis, pad=pad)
        np_ = len(names)
        v = arrays["verts"][:np_].reshape(np_, 3, 3).astype(np.float64)
        b = rng.dirichlet((1.0, 1.0, 1.0), (np_, 6))
        target = np.einsum("krj,kjc->krc", b, v).reshape(-1, 3)
        ro = np.tile(np.asarray(cam["pos"], np.float32), (len(target), 1))
        rd = (target - ro).astype(np.float32)
        ctx.upload_scene(arrays)
        o = oracle_mod.Oracle(arrays)
        kept = 0
        for sample in (0, 1):
            keys = HR.ray_keys(11, 5, len(ro), sample)
            want = HR.mirror(oracle_mod, arrays, ro, rd, keys, oracle=o)
            got = ctx.intersect_rays(ro, rd, sample=sample, seed=11, key_base=5)
            for g, w_, what in zip(got, want, ("tri", "t", "bary", "material")):
                assert np.array_equal(g, w_), (size, axis, sample, what, int((g != w_).sum()))
            occ = ctx.occluded_rays(ro, rd, sample=sample, seed=11, key_base=5)
            assert np.array_equal(occ, HR.occluded(want[1])), (size, axis, sample)
            kept += int(((want[0] >= 0) & (want[0] < np_)).sum())
        o.close()
        assert kept > 0 and (kept < 2 * len(ro) or size == (1, 1))    # some panels stop their rays, some let them through (one texel: all stop)
