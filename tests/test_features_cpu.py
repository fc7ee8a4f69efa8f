"""Host-only half of the first-hit feature planes (include/ptk.h ptk_render_features): the plane table, the truth helper the GPU
tests compare against (tests/feature_truth.py) pinned to a second route through the oracle, and the CLI flag."""
import numpy as np
import pytest

import feature_truth as FT
from conftest import load_golden, scene_from_golden


def test_feature_info_gives_the_table():
    from pbrpathtracer_amd import ptk
    assert len(ptk.FEAT_NAMES) == 10 == len(FT.NAMES) and tuple(ptk.FEAT_NAMES) == FT.NAMES
    assert ptk.FEAT_ALL == 0x3ff
    for k in range(10):
        assert ptk.feature_info(k) == (FT.CHANNELS[k], FT.IS_INT[k]), k
        a = ptk.feature_array(k, 5, 3)
        assert a.shape == ((3, 5) if FT.CHANNELS[k] == 1 else (3, 5, FT.CHANNELS[k]))
        assert a.dtype == (np.int32 if FT.IS_INT[k] else np.float32)
    assert (ptk.FEAT_DEPTH, ptk.FEAT_TRIANGLE, ptk.FEAT_MATERIAL, ptk.FEAT_BARY, ptk.FEAT_POSITION, ptk.FEAT_NORMAL_GEOM,
            ptk.FEAT_NORMAL, ptk.FEAT_ALBEDO, ptk.FEAT_EMISSION, ptk.FEAT_GLOSS) == tuple(range(10))
    for bad in (-1, 10, 1000):
        with pytest.raises(ptk.PtkError):
            ptk.feature_info(bad)
    # NULL outputs are allowed
    assert ptk.load().ptk_feature_info(3, None, None) == ptk.PTK_OK


def _golden_case():
    z = load_golden("tier_s_cornell.npz")
    cam = z["cam"]; proj = z["proj"]
    return scene_from_golden(z), dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]),
                                      focal_dist=float(z["focal_dist"]), aperture=float(z["aperture"]))


def _random_case():
    from test_gpu_random_scenes import random_scene
    return random_scene(15, 300, False)


@pytest.mark.parametrize("case,W,H", [("golden", 48, 40), ("random", 53, 37)])
def test_truth_hits_agree_with_brute_force(oracle_mod, case, W, H):
    """The helper's hit planes come from the oracle's camera-ray records; Oracle.hit(brute=True) on the same rays is a second
    route to the same closest hit (no opacity maps in these scenes, so no draw is involved)."""
    arrays, cam = _golden_case() if case == "golden" else _random_case()
    assert (np.asarray(arrays["materials"])["tex"][:, 5] < 0).all()
    seed, sample = 5, 2
    rec = FT.camera_records(oracle_mod, arrays, cam, W, H, seed, sample)
    tr = FT.truth(oracle_mod, arrays, cam, W, H, seed, sample)
    o = oracle_mod.Oracle(arrays)
    verts = oracle_mod.normalise_arrays(arrays)["verts"]
    hits = 0
    for i in range(W * H):
        y, x = divmod(i, W)
        h, tri, tuv = o.hit(rec["ro"][i], rec["rd"][i], brute=True)
        b = H - 1 - y
        assert tr["triangle"][b, x] == (tri if h else -1)
        if h:
            hits += 1
            assert tr["depth"][b, x] == tuv[0] and tuple(tr["bary"][b, x]) == (tuv[1], tuv[2])
            assert tr["material"][b, x] == arrays["material"][tri]
            assert np.array_equal(tr["normal_geom"][b, x], np.asarray(arrays["tbn"], np.float32).reshape(-1, 9)[tri, 0:3])
            assert np.array_equal(tr["position"][b, x], rec["ro"][i] + rec["rd"][i] * tuv[0])
            # the shading normal never faces away from the viewer
            n = tr["normal"][b, x]
            assert not (np.float32(np.float32(n[0] * rec["rd"][i][0] + n[1] * rec["rd"][i][1]) + n[2] * rec["rd"][i][2]) > 0)
        else:
            assert np.isposinf(tr["depth"][b, x]) and tr["material"][b, x] == -1
            for nm in ("bary", "position", "normal_geom", "normal", "albedo", "emission", "gloss"):
                assert not tr[nm][b, x].any()
    o.close()
    assert 0 < hits, "no pixel hits anything: a poor test"
    assert tr["owned"].all()
    if case == "golden":
        assert hits < W * H, "the golden Cornell frame is expected to show some sky"
    # the lens setting is not part of the definition
    lens = dict(cam, aperture=0.06)
    tr2 = FT.truth(oracle_mod, arrays, lens, W, H, seed, sample)
    for nm in FT.NAMES:
        assert FT.planes_equal(tr[nm], tr2[nm]), nm


def test_truth_under_a_tile_split_partitions_the_frame(oracle_mod):
    arrays, cam = _golden_case()
    W, H = 53, 37
    full = FT.truth(oracle_mod, arrays, cam, W, H, 1, 0)
    seen = np.zeros((H, W), int)
    for r in range(3):
        part = FT.truth(oracle_mod, arrays, cam, W, H, 1, 0, rank=r, world=3)
        seen += part["owned"]
        for nm in FT.NAMES:
            assert FT.planes_equal(part[nm][part["owned"]], full[nm][part["owned"]]), nm
        assert (part["triangle"][~part["owned"]] == -1).all() and np.isposinf(part["depth"][~part["owned"]]).all()
    assert (seen == 1).all()


def test_render_cli_accepts_features_flag():
    from pbrpathtracer_amd import render
    a = render.build_parser().parse_args(["scene.pts", "--features", "planes.npz"])
    assert a.features == "planes.npz"
    assert render.build_parser().parse_args(["scene.pts"]).features is None
