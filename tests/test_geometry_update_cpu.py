"""Geometry updates, the part that needs no GPU: PathTracer::SetObjectTransform stages an object again bit for bit as
LoadObject(file, model) would have staged it, and the C-ABI entry points exist and refuse what can be refused without a device."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT, load_golden

KEYS = ("verts", "normals", "tbn", "uvs", "smoothing", "material", "lights")


def _matrices():
    """[column][row] matrices as LoadObject takes them: TRS, negative scale, shear, a plain translation."""
    from pbrpathtracer_amd import pathtracer as P
    trs = P.trs_matrix((0.3, -1.25, 2.0), (20.0, -35.0, 110.0), (1.5, 0.75, 2.25))
    neg = P.trs_matrix((-2.0, 0.5, 0.0), (0.0, 45.0, 0.0), (-1.0, 1.0, 0.5))
    shear = np.eye(4, dtype=np.float32)
    shear[1][0] = 0.6; shear[2][1] = -0.35; shear[0][2] = 0.2; shear[3][:3] = (0.1, 0.2, -0.3)
    move = np.eye(4, dtype=np.float32); move[3][:3] = (4.0, 0.0, -1.0)
    return {"trs": trs, "negative_scale": neg, "shear": shear, "translation": move}


def _obj_files(tmp_path):
    """the committed OBJ fixtures: the staged scene of tier_k_scene and every flavour of tier_k_obj_variants that has triangles"""
    files = []
    z = load_golden("tier_k_scene.npz")
    p = tmp_path / "scene.obj"
    p.write_bytes(z["obj_file"].tobytes())
    files.append((str(p), [np.asarray(m) for m in z["materials_in"]]))
    v = load_golden("tier_k_obj_variants.npz")
    for name in [str(n) for n in v["names"]]:
        if len(v["tris_" + name]) == 0:
            continue
        q = tmp_path / (name + ".obj")
        q.write_bytes(v["obj_" + name].tobytes())
        files.append((str(q), []))
    assert len(files) >= 10
    return files


def _same(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape, (what, k)
        # bit for bit, NaNs (degenerate tangent frames) included
        assert np.array_equal(a[k].view(np.uint8) if a[k].size else a[k], b[k].view(np.uint8) if b[k].size else b[k]), (what, k)


def test_set_object_transform_stages_like_load_object(tmp_path):
    from pbrpathtracer_amd.pathtracer import PathTracer
    for f, mats in _obj_files(tmp_path):
        for name, M in _matrices().items():
            a = PathTracer(); b = PathTracer()
            a.LoadObject(f, np.eye(4, dtype=np.float32))
            b.LoadObject(f, M)
            for t in (a, b):
                for j, m in enumerate(mats):
                    t.SetMaterial(0, j, m)
            before = a.StagedScene()
            a.SetObjectTransform(0, M)
            a.SetObjectTransform(3, M)                      # a bad id is ignored
            a.SetObjectTransform(-1, M)
            assert a.LastError() == ""
            _same(a.StagedScene(), b.StagedScene(), (f, name))
            if name == "trs":
                assert not np.array_equal(before["verts"], a.StagedScene()["verts"]), f
            a.SetObjectTransform(0, np.eye(4, dtype=np.float32))     # and back: the identity load again
            _same(a.StagedScene(), before, (f, name, "back"))
            a.close(); b.close()


def test_set_object_transform_on_the_second_of_two_objects(tmp_path):
    from pbrpathtracer_amd.pathtracer import PathTracer
    files = _obj_files(tmp_path)
    (f0, mats0), (f1, _) = files[0], files[1]
    M0 = _matrices()["translation"]
    for name, M in _matrices().items():
        a = PathTracer(); b = PathTracer()
        a.LoadObject(f0, M0); a.LoadObject(f1, np.eye(4, dtype=np.float32))
        b.LoadObject(f0, M0); b.LoadObject(f1, M)
        for t in (a, b):
            for j, m in enumerate(mats0):
                t.SetMaterial(0, j, m)
        n0 = PathTracer(); n0.LoadObject(f0, M0); first = n0.GetTriangleCount(); n0.close()
        before = a.StagedScene()
        a.SetObjectTransform(1, M)
        after = a.StagedScene()
        _same(after, b.StagedScene(), name)
        for k in ("verts", "normals", "tbn"):                # the first object is untouched
            assert np.array_equal(after[k][:first].view(np.uint32), before[k][:first].view(np.uint32)), (name, k)
        assert a.GetTriangleCount() == b.GetTriangleCount()
        a.close(); b.close()


def test_update_geometry_entry_points_refuse_without_a_context():
    from pbrpathtracer_amd import ptk
    L = ptk.load()
    for n in ("ptk_update_geometry", "ptk_update_geometry_device", "ptk_geometry_info", "pth_set_object_transform"):
        assert hasattr(L, n), n
    v = np.zeros((1, 9), np.float32)
    assert L.ptk_update_geometry(None, 0, 1, v.ctypes.data, None, None) == -1            # PTK_ERR_BAD_ARG
    assert L.ptk_update_geometry_device(None, 0, 1, v.ctypes.data, None, None) == -1
    assert L.ptk_update_geometry(None, 0, 0, None, None, None) == -1
    u = C.c_uint32(7)
    assert L.ptk_geometry_info(None, C.byref(u), None, None, None) == -1 and u.value == 7



def test_refit_rule_reproduces_the_host_builders_nodes(tmp_path):
    """tests/cpp/test_refit_rule.cpp: the rule refit_kernel applies - leaf boxes from the vertices padded as the builder pads,
    interior boxes from the children's unions, the builders' quantiser - restated in host code, gives the host builder's node
    array bit for bit on soups of 5 to 40 000 triangles, and a valid tree of the same links after the vertices have moved."""
    exe = str(tmp_path / "test_refit_rule")
    csrc = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "test_refit_rule.cpp"),
                           os.path.join(csrc, "bvh_build.cpp"), "-o", exe, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
