"""The census of Trace's arms over the scenes the GPU parity tests render (tests/trace_arms.py): for each trace kernel, every arm
the kernel can reach is reached at least FLOOR times - otherwise "bit for bit against the oracle" says nothing about that arm.  And
the edge scenes' own preconditions: the known-answer table of tex2d against orc_tex2d, the band classes, the ties.  No device."""
import numpy as np
import pytest

import trace_arms as TA
import trace_edge_cases as TE


@pytest.fixture(scope="module")
def counted(oracle_mod):
    return TA.census(oracle_mod)


def test_census_image_is_the_render_and_no_thread_count_shows(oracle_mod):
    a, cam = TE.exact_texture_values("both", pad=4)
    ocam = oracle_mod.make_camera(**cam)
    o = oracle_mod.Oracle(a)
    ref, _ = o.render(ocam, TE.W, TE.H, 4, 0, 3, 9)
    for brute in (False, True):
        tot = np.zeros_like(ref)
        c = o.render_census(ocam, TE.W, TE.H, 4, 0, 3, 9, brute=brute, total=tot)
        assert np.array_equal(tot.view(np.uint32), ref.view(np.uint32))
        assert c == o.render_census(ocam, TE.W, TE.H, 4, 0, 3, 9, brute=brute, threads=1)
        assert all(isinstance(k, str) and k for k in c) and len(set(c)) == len(c)
    o.close()


def test_every_reachable_arm_is_reached_under_every_kernel(counted):
    total, rows = counted
    print("\n" + TA.format_table(total))
    names = list(total["BVH"])
    short = []
    for v in TA.VARIANTS:
        un = TA.unreachable(v, names)
        assert set(un) <= set(names), set(un) - set(names)
        for n in names:
            if n in un:
                assert total[v][n] == 0, f"{v} {n}: listed as unreachable ({un[n]}) and reached {total[v][n]} times"
            elif total[v][n] < TA.FLOOR:
                short.append((v, n, total[v][n]))
    assert not short, short


def test_only_argued_arms_are_listed_unreachable():
    names = ["tex2d.diffuse.plain_fetch", "shade.glass.tir", "shade.opaque.diffuse", "test_triangle.tie_accepted_smaller_index"]
    assert set(TA.unreachable("BVH", names)) == set(TA.NOWHERE)
    assert set(TA.unreachable("FLAT", names)) == set(TA.NOWHERE) | set(TA.IN_INDEX_ORDER)
    for v in TA.VARIANTS:
        assert all(len(why) > 20 for why in TA.unreachable(v, names).values())
    assert "shade.opaque.diffuse" not in TA.unreachable("PLAIN", names) and "shade.glass.tir" in TA.unreachable("PLAIN", names)


def test_every_scene_runs_on_the_kernel_the_registry_says():
    for name, arrays, cam, *_, variants in TA.registry():
        assert variants[0] == TA.variant_of(arrays, cam), name
        assert (len(arrays["verts"]) > 16) == (variants == ("BVH",)), name
    kinds = {name: variants for name, *_, variants in TA.edge_scenes()}
    assert kinds["rr_cap_plain_D1"][0] == "PLAIN" and kinds["rr_cap_textured_D1"][0] == "FLAT" and kinds["rr_cap_padded_D1"] == ("BVH",)
    assert kinds["render_ties_flat"][0] == "PLAIN" and kinds["render_ties_tree"] == ("BVH",)
    assert kinds["sampler_band_opaque_lobe"][0] == "PLAIN" and kinds["sampler_band_glass_lobe"][0] == "FLAT"
    assert kinds["sampler_band_all"] == ("BVH",) and kinds["tex_edges_uv_diffuse_3x2"] == ("BVH",)


# ---- the registry is the tests ----------------------------------------------------------------------------------------------------------
def _params(module, function):
    """the parameter list of a parametrized test, read from its marks"""
    import importlib
    fn = getattr(importlib.import_module(module), function)
    out = []
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize":
            out += list(m.args[1])
    return out


def test_the_registrys_golden_entries_are_the_golden_scenes():
    import glob
    import os
    gold = TA.golden_scenes()
    reg = [s for s in TA.registry() if s[0].startswith(("tier_s_", "tier_f_"))]
    assert [s[0] for s in reg] == [s[0] for s in gold]
    for r, g in zip(reg, gold):
        assert r[3:8] == g[3:8] and r[3:5] + r[6:8] == TA.GOLDEN_FRAME, r[0]
        assert all(np.array_equal(r[2][k], g[2][k]) for k in g[2]) and set(r[2]) == set(g[2]), r[0]
        assert all(np.array_equal(r[1][k], g[1][k], equal_nan=k in ("uvs", "tbn", "normals")) for k in g[1]), r[0]
        assert r[8] == TA.variants_admitted(g[1], g[2]), r[0]
    # every fixture that holds a camera is there, with and without its lens
    with_cam = [os.path.basename(p)[:-4] for p in sorted(glob.glob(os.path.join(TA.GOLDEN, "tier_[sf]_*.npz"))) if "cam" in TA.load_golden(os.path.basename(p)).files]
    assert sorted(s[0] for s in gold) == sorted(n + tail for n in with_cam for tail in ("_lens", "_pinhole")) and len(with_cam) >= 11
    assert all(s[2]["aperture"] == 0.0 for s in gold if s[0].endswith("_pinhole")) and all(s[2]["aperture"] > 0.0 for s in gold if s[0].endswith("_lens"))
    # a plain scene runs on the PLAIN kernel only without a lens
    kinds = {r[0]: r[8] for r in reg}
    assert kinds["tier_f_cornell_pinhole"] == ("PLAIN", "FLAT", "BVH") and kinds["tier_f_cornell_lens"] == ("FLAT", "BVH")
    # ... and tests/test_gpu_trace_arms.py renders exactly that list
    assert _params("test_gpu_trace_arms", "test_golden_scene_renders") == [s[0] for s in gold]


def test_no_registry_entry_is_without_a_rendering_test():
    import test_gpu_plain_frames as PF
    edge = {s[0] for s in TE.scenes()}
    seen = set()
    for name, *_ in TA.registry():
        prefix = max((p for p in TA.RENDERED_BY if p and name.startswith(p)), key=len, default="")
        assert prefix or name in edge, f"{name}: no test is named for it"
        module, function = TA.RENDERED_BY[prefix]
        params = _params(module, function)
        if prefix in ("tier_s_", "tier_f_"):
            ok = name in params
        elif prefix in ("random_", "grazing_"):
            ok = int(name[len(prefix):]) in [p[0] for p in params]
        elif prefix == "plain_frames_":
            ok = name[len(prefix):] in params or name[len(prefix):] in PF.moved_scenes()       # (the moved ones: test_table_follows_a_geometry_update)
        elif prefix == "rr_cap_":
            ok = name.split("_")[2] in params
        elif prefix == "tex_edges_":
            ok = name.split("_")[3] in params
        elif prefix == "":
            ok = any(name.startswith(p) for p, _ in params)
        else:
            ok = params == []                                                               # one scene, one unparametrized test
        assert ok, (name, module, function)
        seen.add(prefix)
    assert seen == set(TA.RENDERED_BY)


# ---- tex2d: the known answers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", TE.TEX_SIZES)
def test_tex2d_known_answers_are_orc_tex2d(oracle_mod, size):
    """the table of trace_edge_cases.SPECIALS, written down from the rule, against the oracle's tex2d on each axis"""
    w, h = size
    a, _, _ = TE.tex_edges(0, size, "u")
    img = TE.edge_texture(w, h, 0)
    assert len(np.unique(img[..., 0])) == w * h, "every texel distinct"
    o = oracle_mod.Oracle(a)
    for name, c, _ in TE.SPECIALS:
        col, row = TE.special_texel(name, w), TE.special_texel(name, h)
        plain_col, plain_row = int(0.3 * w), int(0.3 * h)
        got_u = o.tex2d(0, c, TE.PLAIN_COORD); got_v = o.tex2d(0, TE.PLAIN_COORD, c)
        assert np.array_equal(got_u, img[plain_row, col].astype(np.float32) / np.float32(255)), (name, "u", size)
        assert np.array_equal(got_v, img[row, plain_col].astype(np.float32) / np.float32(255)), (name, "v", size)
    o.close()


def test_the_upper_clamp_is_taken_by_a_slightly_negative_coordinate_and_the_lower_by_nan(oracle_mod):
    a, cam, names = TE.tex_edges(0, (3, 2), "uv")
    o = oracle_mod.Oracle(a)
    c = o.render_census(oracle_mod.make_camera(**cam), TE.W, TE.H, 4, 0, TE.SPP, TE.SEED)
    o.close()
    for arm in ("upper_clamp_x", "upper_clamp_y", "lower_clamp_x", "lower_clamp_y", "plain_fetch"):
        assert c["tex2d.diffuse." + arm] >= TA.FLOOR, (arm, c["tex2d.diffuse." + arm])


# ---- the sampler's band --------------------------------------------------------------------------------------------------------
def test_band_values_fall_in_their_classes():
    assert [TE.band_class(x) for x in TE.BAND_NX] == ["below", "band", "band", "band", "pole", "pole", "pole"]
    a, _ = TE.sampler_band("all")
    nx = np.abs(a["tbn"][:14 * len(TE.BAND_MATERIALS), 0])
    assert set(nx.tolist()) == set(float(x) for x in TE.BAND_NX)
    # the shading-normal panels: geometric normal at the pole, stored tangents of half length on the mapped one
    tail = a["tbn"][14 * len(TE.BAND_MATERIALS):14 * len(TE.BAND_MATERIALS) + 14]
    assert (tail[:, 0] == 1.0).all()


def test_shading_normal_alone_reaches_the_band(oracle_mod):
    """the panels of sampler_band("shading") have the pole as geometric normal: whatever the census finds in the band got there
    through smoothing or the normal map"""
    a, cam = TE.sampler_band("shading")
    o = oracle_mod.Oracle(a)
    c = o.render_census(oracle_mod.make_camera(**cam), TE.W, TE.H, 4, 0, TE.SPP, TE.SEED, brute=True)
    o.close()
    for site in ("opaque_rough_one", "opaque_lobe", "opaque_diffuse", "glass_refract_normal", "glass_rough_one", "glass_lobe",
                 "glass_diffuse"):
        assert c[f"sample_about.{site}.in_the_band"] >= TA.FLOOR, (site, c[f"sample_about.{site}.in_the_band"])
    assert c["shade.smoothing_on"] >= TA.FLOOR and c["shade.normal_map_on"] >= TA.FLOOR


# ---- Russian roulette's cap ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "textured", "padded", "glass"])
def test_rr_cap_scenes_kill_paths_between_the_cap_and_the_maximum(oracle_mod, kind):
    """the draw that tells cap from no cap, 0.95 < r <= max(diffuse), happens - and the image stays finite with a diffuse of 4"""
    n = 0
    for D in (1, 2, 3):
        a, cam = TE.rr_cap(kind)
        o = oracle_mod.Oracle(a)
        tot = np.zeros((TE.H, TE.W, 3), np.float32)
        c = o.render_census(oracle_mod.make_camera(**cam), TE.W, TE.H, D, 0, 4, TE.SEED, total=tot)
        o.close()
        assert np.isfinite(tot).all() and tot.any()
        assert c["shade.rr_cap_active"] >= TA.FLOOR
        n += c["shade.rr_killed_between_cap_and_max"]
    assert n >= TA.FLOOR, n


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
def test_render_ties_take_both_arms_in_the_tree_and_one_in_index_order(oracle_mod):
    for name, build, brute in (("flat", lambda: TE.render_ties(6, others=3), True), ("tree", lambda: TE.render_ties(12, pad=6, others=6), False)):
        a, cam = build()
        o = oracle_mod.Oracle(a)
        c = o.render_census(oracle_mod.make_camera(**cam), TE.W, TE.H, 4, 0, TE.SPP, TE.SEED, brute=brute)
        o.close()
        assert c["test_triangle.tie_rejected_larger_index"] >= TA.FLOOR, (name, c)
        if brute:
            assert c["test_triangle.tie_accepted_smaller_index"] == 0
        else:
            assert c["test_triangle.tie_accepted_smaller_index"] >= TA.FLOOR, (name, c["test_triangle.tie_accepted_smaller_index"])
