"""The scene table of tests/scene_swap_cases.py is what it claims: every scene on its stated side of every boundary at which
ptk_upload_scene switches representation, and the ordered pairs of tests/test_gpu_scene_swap.py cross every boundary in both
directions - so that a later edit cannot quietly take a boundary out of the matrix.  And the stale-history case is a real one: by
the rule (tests/temporal_rule.py), one scene's temporal history over the other's planes does change pixels."""
import numpy as np
import pytest

import feature_truth as FT
import scene_swap_cases as SC
import temporal_rule as TR


def desc(arrays):
    from pbrpathtracer_amd import ptk
    a = ptk.normalise_arrays(arrays)
    return a, ptk.scene_desc(a)


@pytest.mark.parametrize("name", SC.NAMES)
def test_scene_is_on_its_stated_sides(name):
    from pbrpathtracer_amd import ptk
    claim, b = SC.CLAIMS[name], SC.boundaries(name)
    arrays, cam = SC.scene(name)
    a, d = desc(arrays)
    L = ptk.load()
    assert claim["tris"][0] <= b["tris"] <= claim["tris"][1], (name, b["tris"])
    assert (b["tris"] <= 16) == (claim["tris"][1] <= 16) and (b["tris"] >= 4096) == (claim["tris"][0] >= 4096)
    assert bool(L.ptk_scene_is_plain(ptk.C.byref(d))) == claim["plain"] == b["plain"], name
    assert bool(L.ptk_scene_is_lambert(ptk.C.byref(d))) == claim["lambert"] == b["lambert"], name
    assert b["opacity"] == claim["opacity"] and b["lights"] == claim["lights"] and (b["textures"] > 0) == claim["textures"], (name, b)
    # what the upload checks before it takes a scene, so that no pair is refused
    n = b["tris"]
    assert np.isfinite(a["verts"]).all() and (a["material"] >= 0).all() and (a["material"] < b["materials"]).all()
    assert (a["lights"] >= 0).all() and (a["lights"] < max(n, 1)).all() and (a["materials"]["tex"] < b["textures"]).all()
    assert b["materials"] >= 1 and cam["aperture"] >= 0.0


def test_the_particular_claims():
    from pbrpathtracer_amd import ptk
    b = {name: SC.boundaries(name) for name in SC.NAMES}
    assert b["empty"]["tris"] == 0 and b["empty"]["materials"] == 1
    assert b["bvh_small"]["num_lights"] == 2
    assert 64 < b["bvh_nolights"]["tris"] < 160 and b["bvh_nolights"]["num_lights"] == 0
    assert b["bvh_device"]["tris"] == 4096                      # torus(nu, nv) has 2 nu nv triangles: no closed grid mesh is nearer the threshold
    for name in SC.NAMES:
        if name != "bvh_textured":
            assert b[name]["materials"] < b["bvh_textured"]["materials"] and b[name]["textures"] < b["bvh_textured"]["textures"], name
    assert b["bvh_textured"]["textures"] >= 3
    # the device-built mesh is closed: every directed edge has its opposite
    v = np.round(SC.scene("bvh_device")[0]["verts"].reshape(-1, 3, 3).astype(np.float64), 5)
    edges = {}
    for t in v:
        for k in range(3):
            key = (tuple(t[k]), tuple(t[(k + 1) % 3]))
            edges[key] = edges.get(key, 0) + 1
    assert all(c == 1 and edges.get((q, p), 0) == 1 for (p, q), c in edges.items())
    # flat_plain: a pair prefix and a class table that are not trivial
    plain = SC.scene("flat_plain")[0]
    assert len(ptk.flat_rect_prefix(plain["verts"])) == 6
    classes = {ptk.flat_zero_class(*t) for t in plain["verts"].reshape(-1, 3, 3)}
    assert len(classes) >= 3 and classes != {0}
    # flat_generic: smoothing, a reflective material, a texture; flat_opacity: the map is on one material
    gen = SC.scene("flat_generic")[0]
    assert gen["smoothing"].any() and (gen["materials"]["reflectiveness"] > 0).any() and (gen["materials"]["tex"][:, :5] >= 0).any()
    assert (SC.scene("flat_opacity")[0]["materials"]["tex"][:, 5] >= 0).sum() == 1


def test_the_pairs_are_the_agreed_ones_and_cross_every_boundary_both_ways():
    want = [("flat_plain", "bvh_small"), ("flat_plain", "flat_generic"), ("flat_generic", "flat_opacity"), ("flat_opacity", "bvh_device"),
            ("bvh_small", "bvh_device"), ("bvh_textured", "bvh_small"), ("bvh_small", "bvh_nolights"), ("empty", "bvh_textured"),
            ("empty", "flat_plain")]
    assert set(SC.PAIRS) == {p for a, b in want for p in ((a, b), (b, a))} and len(SC.PAIRS) == 18 == len(set(SC.PAIRS))
    b = {name: SC.boundaries(name) for name in SC.NAMES}
    crossed = set()
    for x, y in SC.PAIRS:
        for key in ("empty", "flat", "device", "plain", "lambert", "opacity", "lights"):
            if b[x][key] != b[y][key]:
                crossed.add((key, b[x][key], b[y][key]))
        for key in ("tris", "materials", "textures", "num_lights"):
            if b[x][key] != b[y][key]:
                crossed.add((key, "more" if b[y][key] > b[x][key] else "fewer"))
        if b[x]["flat"] and b[y]["flat"] and b[x]["plain"] != b[y]["plain"]:
            crossed.add(("plain among flat lists", b[x]["plain"], b[y]["plain"]))
        if not b[x]["empty"] and not b[y]["empty"] and not b[x]["flat"] and not b[y]["flat"] and b[x]["device"] != b[y]["device"]:
            crossed.add(("builder among trees", b[x]["device"], b[y]["device"]))
    for key in ("empty", "flat", "device", "plain", "lambert", "opacity", "lights", "plain among flat lists", "builder among trees"):
        assert (key, True, False) in crossed and (key, False, True) in crossed, key
    for key in ("tris", "materials", "textures", "num_lights"):
        assert (key, "more") in crossed and (key, "fewer") in crossed, key


def test_queries_hit_and_miss():
    for name in SC.NAMES:
        q = SC.queries(name)
        n = SC.N_QUERIES
        assert all(len(q[k]) == n for k in q) and n % 64 != 0 and n // 64 == 3
        assert np.isinf(q["tmax"]).sum() > n // 2 and np.isfinite(q["tmax"]).sum() > n // 8
        assert np.isinf(q["max_dist"]).sum() > n // 3 and np.isfinite(q["max_dist"]).sum() > n // 3
    # a third misses whatever the scene: brute force over the box scene and the torus
    import closest_rule as CR
    import crossings_rule as XR
    for name in ("bvh_small", "bvh_nolights"):
        a, q = SC.scene(name)[0], SC.queries(name)
        miss = np.arange(SC.N_QUERIES) % 3 == 2
        front, back = XR.crossing_masks(a["verts"], q["ro"], q["rd"], q["tmax"])
        crosses = (front | back).any(axis=1)
        assert not crosses[miss].any() and crosses[~miss].mean() > 0.25, name
        tri = CR.mirror(a, q["pts"], q["max_dist"])[0]
        assert (tri[miss] < 0).all() and (tri[~miss] >= 0).mean() > 0.25, name


@pytest.mark.parametrize("old,new", [("flat_plain", "flat_generic"), ("flat_generic", "flat_plain")])
def test_a_surviving_history_would_change_the_temporal_frame(oracle_mod, old, new):
    """The two boxes share walls and material indices: by the rule every tap of the old scene's history is accepted over the new
    scene's planes.  So a context that kept its history across the upload gives another frame than a fresh one."""
    from pbrpathtracer_amd import ptk
    frames = {}
    for name in (old, new):
        arrays, cam = SC.scene(name)
        o = oracle_mod.Oracle(arrays)
        ocam = oracle_mod.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])
        total, _ = o.render(ocam, SC.W, SC.H, SC.DEPTH, 0, SC.SPP, SC.SEED)
        o.close()
        planes = FT.truth(oracle_mod, arrays, cam, SC.W, SC.H, 0, 0)
        color, count = TR.frame_inputs(total, np.full((SC.H, SC.W), SC.SPP))
        frames[name] = (color, count, planes["material"], planes["position"], planes["normal"])
    cam = SC.scene(new)[1]
    assert all(np.array_equal(SC.scene(old)[1][k], cam[k]) for k in cam)
    prm = ptk.temporal_defaults(SC.extent(SC.scene(new)[0])).as_dict()
    out, out_n, found = TR.reproject(TR.view_of(cam, SC.W, SC.H), frames[new], frames[old], prm, want_found=True)
    fresh, fresh_n = TR.no_history(frames[new])
    differ = (out.view(np.uint32) != fresh.view(np.uint32)).any(axis=2)
    print(f"{old} -> {new}: history found at {int(found.sum())} of {SC.W * SC.H} pixels, colour differs at {int(differ.sum())}, "
          f"count at {int((out_n != fresh_n).sum())}")
    assert found.sum() > SC.W * SC.H // 4 and differ.sum() > SC.W * SC.H // 8 and (out_n != fresh_n).sum() > SC.W * SC.H // 4
