"""Stochastic opacity on the CPU oracle (and, when oracle/_ref was built, on the real reference) against exact float64
expectations that depend on neither: layer-stack fractions, exact edges, shadow rays through layers, a light with its own
opacity texture, and the independence of the per-pixel random streams.  The scenes and the expectations live in
tests/opacity_cases.py; tests/test_gpu_opacity_expectations.py runs the same cases on the HIP path."""
import numpy as np
import pytest

import opacity_cases as OC
from oracle import ref_binding as RB

W = H = 48
SPP = 96


def _renderer(OB, built):
    o, cam = OC.oracle(OB, built)

    def render(b, first, spp, seed):
        assert b is built
        return o.render(cam, b.width, b.height, b.depth, first, spp, seed, want_rgb8=False)[0]
    return render


def _render(OB, built, first, spp, seed):
    return _renderer(OB, built)(built, first, spp, seed)


@pytest.mark.parametrize("stack", sorted(OC.STACKS))
@pytest.mark.parametrize("lens", [False, True])
def test_layer_stack_fractions(tmp_path, oracle_mod, stack, lens):
    built, ps = OC.stack_scene(str(tmp_path), stack, W, H, lens=lens)
    zs = OC.check_stack(_renderer(oracle_mod, built), built, ps, SPP)
    print(stack, lens, {k: round(v, 2) for k, v in zs.items()})


def test_exact_edges(tmp_path, oracle_mod):
    d = str(tmp_path)
    plain = OC.edge_scene(d, "none", None, W, H, with_layers=False)
    opaque = OC.edge_scene(d, "opaque", None, W, H)
    ref_plain = _render(oracle_mod, plain, 0, 8, 3)
    ref_opaque = _render(oracle_mod, opaque, 0, 8, 3)
    assert not np.array_equal(ref_plain, ref_opaque)
    # texel 0 (and only red counts: green / blue / alpha full) is invisible; texel 255 (red full, the rest 0) is opaque
    for name, op, want in [("t0", 0, ref_plain), ("t255", 255, ref_opaque),
                           ("gb_ppm", (0, 255, 255), ref_plain), ("r_ppm", (255, 0, 0), ref_opaque),
                           ("gba_tga", (0, 255, 255, 255), ref_plain), ("r_tga", (255, 0, 0, 0), ref_opaque)]:
        b = OC.edge_scene(d, name, op, W, H)
        assert np.array_equal(_render(oracle_mod, b, 0, 8, 3), want), name


def test_uv_at_the_candidate(tmp_path, oracle_mod):
    b = OC.uv_split_scene(str(tmp_path), W, H)
    o, cam = OC.oracle(oracle_mod, b)
    u = OC.uv_of_candidate(OC.staged(b), b.layer_tris[0], cam.pos[:], o.primary_dirs(cam, W, H).reshape(-1, 3)).reshape(H, W)
    acc, _ = o.render(cam, W, H, b.depth, 0, 16, 9, want_rgb8=False)
    see, block = u < 0.5 - 1e-3, u > 0.5 + 1e-3
    assert see.sum() > 0.1 * W * H and block.sum() > 0.1 * W * H
    assert np.all(acc[see] == [0, 0, 16]) and np.all(acc[block] == [16, 0, 0])


@pytest.mark.parametrize("pad", [0, 16])
def test_shadow_rays_through_layers(tmp_path, oracle_mod, pad):
    texels = (77, 128, 1)
    p = OC.through_all([OC.p_accept(x) for x in texels])
    plain = OC.shadow_scene(str(tmp_path), "plain", [], W, H, pad=pad)
    layered = OC.shadow_scene(str(tmp_path), "layered", texels, W, H, pad=pad)
    for seed in OC.SEEDS:
        z = OC.check_shadow_pairs(OC.per_sample(_renderer(oracle_mod, plain), plain, 24, seed),
                                  OC.per_sample(_renderer(oracle_mod, layered), layered, 24, seed), p, f"seed {seed}")
        print(seed, round(z, 2))


def test_light_with_its_own_opacity(tmp_path, oracle_mod):
    d = str(tmp_path)
    b0 = OC.shadow_scene(d, "l0", [], W, H)
    b1 = OC.shadow_scene(d, "l1", [], W, H, light_opacity=128)
    w0 = OC.shadow_scene(d, "w0", [], W, H, wall_behind_light=True)
    w1 = OC.shadow_scene(d, "w1", [], W, H, light_opacity=128, wall_behind_light=True)
    for seed in OC.SEEDS:
        # nothing behind the light: a rejected light lets the shadow ray go on, and finding nothing means lit
        assert np.array_equal(_render(oracle_mod, b0, 0, 16, seed), _render(oracle_mod, b1, 0, 16, seed))
        # a wall behind it: lit exactly when the light's one draw accepts (a second chance would give 1 - (1 - P)^2)
        OC.check_shadow_pairs(OC.per_sample(_renderer(oracle_mod, w0), w0, 24, seed),
                              OC.per_sample(_renderer(oracle_mod, w1), w1, 24, seed), OC.p_accept(128), f"seed {seed}")


def test_stream_independence(tmp_path, oracle_mod):
    """Count images of seeds s and s + 1, of s and s + 2^32, and of the sample ranges [0, N) and [N, 2N) are uncorrelated."""
    built, ps = OC.stack_scene(str(tmp_path), "a", W, H)
    render = _renderer(oracle_mod, built)
    for s in OC.SEEDS:
        a = render(built, 0, SPP, s)
        for what, b in [("seed + 1", render(built, 0, SPP, s + 1)), ("seed + 2^32", render(built, 0, SPP, s + 2 ** 32)),
                        ("next sample range", render(built, SPP, SPP, s))]:
            for c in range(3):
                OC.assert_uncorrelated(a[..., c], b[..., c], f"seed {s} vs {what}, channel {c}")


@pytest.mark.parametrize("pad", [0, 16])
def test_shadow_and_bounce_draws_are_independent(tmp_path, oracle_mod, pad):
    d = str(tmp_path)
    p = OC.p_accept(128)
    plain = OC.joint_scene(d, "plain", None, W, H, with_layer=False, pad=pad)
    opaque = OC.joint_scene(d, "opaque", None, W, H, pad=pad)
    layered = OC.joint_scene(d, "layered", 128, W, H, pad=pad)
    for seed in OC.SEEDS:
        A, B, C = (OC.per_sample(_renderer(oracle_mod, b), b, 24, seed) for b in (plain, opaque, layered))
        print(seed, {k: round(v, 2) for k, v in OC.check_joint(A, B, C, p, f"seed {seed}").items()})


# ---- the real reference (oracle/_ref, built by `make -f oracle/Makefile.ref`): ties the exact formulas to it ------------------


def _ref_render(ref, built, first, spp, seed):
    assert first == 0
    ref.load_scene(built.scene, exact_pinhole=True)
    ref.lib.ref_seed(seed)
    ref.render(spp, threads=1)
    return ref.total(built.width, built.height)


def _ref_lit(ref, built, spp, seed):
    """Per (pixel, sample): whether the sample's radiance is non-zero (one RenderFrame at a time, single thread)."""
    ref.load_scene(built.scene, exact_pinhole=True)
    ref.lib.ref_seed(seed)
    prev = np.zeros((built.height, built.width, 3), np.float32)      # (the first frame clears the accumulator, :745-751)
    out = []
    for _ in range(spp):
        ref.render(1, threads=1)
        t = ref.total(built.width, built.height)
        out.append(np.any(t != prev, axis=-1))
        prev = t
    return np.stack(out)


@pytest.mark.skipif(not RB.available(), reason="the real reference is not built: run `make -f oracle/Makefile.ref` "
                                               "(needs the reference sources)")
def test_reference_meets_the_exact_expectations(tmp_path):
    """Cases 1, 3 and 4 on the reference itself.  Its Rand() draws for every intersected triangle in traversal order, from the
    same stream as everything else, so samples cannot be paired with an opacity-free render: the "unchanged or 0" checks
    become two-sample rate checks."""
    ref = RB.Ref()
    d = str(tmp_path)
    zs = {}
    for stack in sorted(OC.STACKS):
        for lens in (False, True):
            built, ps = OC.stack_scene(d, stack, 32, 32, lens=lens, pow2=True)
            z = OC.check_stack(lambda b, f, n, s: _ref_render(ref, b, f, n, s), built, ps, 64)
            zs[f"stack {stack} lens {int(lens)}"] = max(z.values(), key=abs)
    texels = (77, 128, 1)
    plain = OC.shadow_scene(d, "plain", [], 32, 32, pow2=True)
    layered = OC.shadow_scene(d, "layered", texels, 32, 32, pow2=True)
    b0 = OC.shadow_scene(d, "l0", [], 32, 32, pow2=True)
    b1 = OC.shadow_scene(d, "l1", [], 32, 32, light_opacity=128, pow2=True)
    w0 = OC.shadow_scene(d, "w0", [], 32, 32, wall_behind_light=True, pow2=True)
    w1 = OC.shadow_scene(d, "w1", [], 32, 32, light_opacity=128, wall_behind_light=True, pow2=True)
    for seed in OC.SEEDS:
        a, b = _ref_lit(ref, plain, 32, seed), _ref_lit(ref, layered, 32 , seed + 1)
        zs[f"shadow {seed}"] = OC.assert_ratio(b.sum(), b.size, a.sum(), a.size,
                                               OC.through_all([OC.p_accept(x) for x in texels]), f"reference shadow, seed {seed}")
        a, b = _ref_lit(ref, b0, 32, seed), _ref_lit(ref, b1, 32, seed + 1)
        zs[f"light alone {seed}"] = OC.assert_ratio(b.sum(), b.size, a.sum(), a.size, 1.0, f"reference light alone, seed {seed}")
        a, b = _ref_lit(ref, w0, 32, seed), _ref_lit(ref, w1, 32, seed + 1)
        zs[f"light + wall {seed}"] = OC.assert_ratio(b.sum(), b.size, a.sum(), a.size, OC.p_accept(128),
                                                     f"reference light before a wall, seed {seed}")
    print({k: round(float(v), 2) for k, v in zs.items()})


@pytest.mark.skipif(not RB.available(), reason="the real reference is not built: run `make -f oracle/Makefile.ref` "
                                               "(needs the reference sources)")
def test_reference_draws_twice_for_a_lone_triangle(tmp_path):
    """The reference's tree builder makes BOTH children of a one-triangle subtree that triangle (mesh.cpp:182-186), and Hit visits
    both, so such a triangle gets two opacity draws per ray and is accepted with 1 - (1 - P)^2.  Which triangles end up alone
    depends on its random tree (none when the triangle count is a power of two); the port draws once per candidate (DESIGN.md
    §2, difference 4).  Pinned on a one-layer scene, where the lone triangle is the layer whatever the tree."""
    ref = RB.Ref()
    built, _ = OC.build(str(tmp_path), "lone", [], [OC.Layer(0.0, 77, OC.RED)], 32, 32, 2), None
    p = OC.p_accept(77)
    for seed in OC.SEEDS:
        acc = _ref_render(ref, built, 0, 64, seed)
        n = 32 * 32 * 64
        OC.assert_binom(acc[..., 0].sum(), n, 1.0 - (1.0 - p) ** 2, f"reference, one layer, seed {seed}")
        assert abs(OC.binom_z(acc[..., 0].sum(), n, p)) > 50
