"""Surface attribute queries (include/ptk.h ptk_surface_attributes) without a GPU: the numpy restatement tests/surface_attr_rule.py
reproduces the feature planes' truth (tests/feature_truth.py, itself held to the GPU planes by tests/test_gpu_features.py) when it
is fed that truth's own triangle, bary and camera-ray directions; its miss rule; the shape and type tables; and the symbols."""
import os
import re

import numpy as np
import pytest

import feature_truth as FT
import surface_attr_rule as AR
from conftest import load_golden, scene_from_golden
from pbrpathtracer_amd.ptk import ATTR_ALL, ATTR_NAMES          # (without the feature this module does not import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SHARED = ("material", "normal_geom", "normal", "albedo", "emission", "gloss")


def _golden(name):
    z = load_golden(f"tier_{name}.npz")
    cam = z["cam"]; proj = z["proj"]
    return scene_from_golden(z), dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]),
                                      focal_dist=float(z["focal_dist"]), aperture=0.0)


def _random(seed, n):
    from test_gpu_random_scenes import random_scene
    arrays, cam = random_scene(seed, n, True)
    return arrays, dict(cam, aperture=0.0)


CASES = {"golden_s_cornell": (lambda: _golden("s_cornell"), 48, 40), "golden_s_opacity": (lambda: _golden("s_opacity"), 48, 40),
         "random_14_300": (lambda: _random(14, 300), 48, 32)}


@pytest.mark.parametrize("kind", sorted(CASES))
def test_restatement_reproduces_the_feature_truth(oracle_mod, kind):
    make, W, H = CASES[kind]
    arrays, cam = make()
    seed, sample = 9, 3
    want = FT.truth(oracle_mod, arrays, cam, W, H, seed, sample)
    rec = FT.camera_records(oracle_mod, arrays, cam, W, H, seed, sample)
    tri = want["triangle"][::-1].reshape(-1)                         # planes are bottom-up, records top-down
    bary = want["bary"][::-1].reshape(-1, 2)
    assert np.array_equal(tri, rec["tri"])
    got, arms = AR.restate(oracle_mod, arrays, tri, bary[:, 0], bary[:, 1], rec["rd"])
    assert (tri >= 0).any() and np.array_equal(arms["hit"], tri >= 0)
    for nm in SHARED:
        c = got[nm].shape[1] if got[nm].ndim > 1 else 1
        plane = np.ascontiguousarray(got[nm].reshape((H, W, c) if c > 1 else (H, W))[::-1])
        assert FT.planes_equal(plane, want[nm]), (kind, nm)
    b = want["branches"]
    assert (int(arms["smooth_only"].sum()), int(arms["map_only"].sum()), int(arms["both"].sum()), int(arms["flip"].sum())) == \
           (b["smooth"], b["normal_map"], b["both"], b["flip"])


def test_miss_rule_and_values_as_given(oracle_mod):
    arrays, _ = _random(14, 300)
    n_tris = len(arrays["verts"])
    tri = np.array([-1, n_tris, 2 ** 31 - 1, -2 ** 31, 0, n_tris - 1], np.int32)
    u = np.full(len(tri), 0.25, F32); v = np.full(len(tri), 0.5, F32)
    d = np.tile(np.array([[0.0, 0.0, 1.0]], F32), (len(tri), 1))
    got, arms = AR.restate(oracle_mod, arrays, tri, u, v, d)
    assert arms["hit"].tolist() == [False, False, False, False, True, True]
    for nm in AR.NAMES:
        miss = got[nm][:4]
        assert (miss == (-1 if nm == "material" else 0)).all(), nm
    a = oracle_mod.normalise_arrays(arrays)
    assert got["material"][4] == a["material"][0] and got["material"][5] == a["material"][n_tris - 1]
    # no clamp: a corner is that vertex (u = 1: the second), outside extrapolates, a NaN propagates into what depends on it
    tri = np.zeros(4, np.int32)
    got, _ = AR.restate(oracle_mod, arrays, tri, np.array([0, 1, 0, np.nan], F32), np.array([0, 0, 1, 0.5], F32))
    vt = a["verts"][0]
    assert np.array_equal(got["position"][0], vt[0:3]) and np.array_equal(got["position"][1], vt[3:6]) and np.array_equal(got["position"][2], vt[6:9])
    assert np.isnan(got["position"][3]).all() and np.isnan(got["uv"][3]).all()
    assert got["material"][3] == a["material"][0] and np.array_equal(got["normal_geom"][3], a["tbn"][0, 0:3])


def test_attribute_tables_and_arrays():
    from pbrpathtracer_amd import ptk
    assert ATTR_NAMES == AR.NAMES and ATTR_ALL == (1 << 9) - 1 == (1 << len(AR.NAMES)) - 1
    assert (ptk.ATTR_MATERIAL, ptk.ATTR_UV, ptk.ATTR_POSITION, ptk.ATTR_NORMAL_GEOM, ptk.ATTR_NORMAL, ptk.ATTR_ALBEDO, ptk.ATTR_EMISSION,
            ptk.ATTR_GLOSS, ptk.ATTR_OPACITY) == tuple(range(9))
    for k, (c, i) in enumerate(zip(AR.CHANNELS, AR.IS_INT)):
        assert ptk.attribute_info(k) == (c, i), k
        arr = ptk.attribute_array(k, 7)
        assert arr.shape == ((7,) if c == 1 else (7, c)) and arr.dtype == (np.int32 if i else np.float32)
        assert ptk.attribute_array(k, 0).shape[0] == 0
    for bad in (-1, 9):
        with pytest.raises(ptk.PtkError):
            ptk.attribute_info(bad)
    text = open(os.path.join(ROOT, "include", "ptk.h")).read()
    for k, nm in enumerate(AR.NAMES):
        assert re.search(rf"#define PTK_ATTR_{nm.upper()} {k}\b", text), nm
    assert re.search(r"#define PTK_ATTR_COUNT 9\b", text)


def test_symbols_are_exported_and_declared():
    from pbrpathtracer_amd import ptk, pathtracer
    L = ptk.load()
    text = open(os.path.join(ROOT, "include", "ptk.h")).read() + open(os.path.join(ROOT, "include", "ptk_host.h")).read()
    declared = set(re.findall(r"\b(p(?:tk|th)_[a-z0-9_]+)\s*\(", text))
    for name in ("ptk_surface_attributes", "ptk_surface_attributes_device", "ptk_attribute_info", "ptk_last_attributes_ms",
                 "pth_surface_attributes"):
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in ptk.SYMBOLS + pathtracer.HOST_SYMBOLS, name
    assert "typedef struct ptk_surface_attrs" in text
    assert "SurfaceAttributes" in open(os.path.join(ROOT, "include", "pathtracer.h")).read()
    assert callable(ptk.Context.surface_attributes) and callable(pathtracer.PathTracer.surface_attributes)
    assert [f[0] for f in ptk.SurfaceAttrs._fields_] == list(AR.NAMES)
