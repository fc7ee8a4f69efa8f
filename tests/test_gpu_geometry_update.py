"""Geometry updates after ptk_upload_scene (include/ptk.h ptk_update_geometry): records repacked in place, the
BVH refitted on the GPU with its links kept.  Closest hits do not depend on the tree, so after any motion the context must
render, probe and pick bit for bit what a second context does that uploaded the moved arrays from scratch, and what the CPU
oracle renders from them.  Every comparison is np.array_equal."""
import time

import numpy as np
import pytest

from bvh_check import check_bvh
from conftest import load_golden, scene_from_golden
from test_gpu_random_scenes import random_scene

pytestmark = pytest.mark.gpu

W, H, D, SPP = 56, 40, 5, 4
LINKS = [6, 7, 8, 9]


@pytest.fixture(scope="module")
def ctxs():
    from pbrpathtracer_amd import ptk
    a, b = ptk.Context(0), ptk.Context(0)
    yield a, b
    a.close(); b.close()


def _ocam(OB, cam):
    return OB.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])


def _oracle(OB, arrays, cam, first=0, spp=SPP, seed=5, w=W, h=H, d=D):
    o = OB.Oracle(arrays)
    out = o.render(_ocam(OB, cam), w, h, d, first, spp, seed)
    o.close()
    return out


def _setup(c, arrays, cam, w=W, h=H, d=D):
    c.upload_scene(arrays); c.set_camera(**cam); c.set_frame(w, h, d); c.set_tile(0, 1); c.reset()


def _render(c, spp=SPP, seed=5):
    c.reset(); c.render(0, spp, seed)
    return c.read_accum(), c.resolve_rgb8()


def _rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def _motion(arrays, kind, seed=3):
    """(first, verts, normals, tbn) of an update and the whole moved scene; normals / tbn None = vertices only"""
    rng = np.random.default_rng(seed)
    n = len(arrays["verts"])
    v = arrays["verts"].reshape(n, 3, 3).astype(np.float64)
    a, b = (n // 3, max(n // 3 + 1, (2 * n) // 3)) if n > 2 else (0, n)
    nn = tb = None
    if kind == "rigid":
        R = _rot_y(25.0)
        nv = v[a:b] @ R.T + np.array([0.3, 0.15, -0.2])
        nn = (arrays["normals"][a:b].reshape(-1, 3, 3).astype(np.float64) @ R.T).astype(np.float32).reshape(-1, 9)
        tb = (arrays["tbn"][a:b].reshape(-1, 3, 3).astype(np.float64) @ R.T).astype(np.float32).reshape(-1, 9)
    elif kind == "scale":
        a, b = 0, n
        nv = v * np.array([1.3, 0.8, 1.1])
    elif kind == "jitter":
        a, b = 0, n
        nv = v + rng.normal(0, 0.03, v.shape)
    elif kind == "collapse":
        nv = np.broadcast_to(v[a:b].mean(axis=(0, 1)), v[a:b].shape)
    elif kind == "far":
        size = float(np.abs(v).max())
        nv = v[a:b] + np.array([1e4 * size, 0, 0])
    else:
        raise ValueError(kind)
    nv = np.ascontiguousarray(nv, np.float32).reshape(-1, 9)
    moved = dict(arrays)
    moved["verts"] = arrays["verts"].copy(); moved["verts"][a:b] = nv
    if nn is not None:
        moved["normals"] = arrays["normals"].copy(); moved["normals"][a:b] = nn
        moved["tbn"] = arrays["tbn"].copy(); moved["tbn"][a:b] = tb
    return a, nv, nn, tb, moved


def _c4_arrays(tmp):
    from pbrpathtracer_amd import scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer, camera_from_scene
    pts, scene, _ = S.build_config("C4", str(tmp), width=W, height=H, depth=D)
    pt = PathTracer(0); pt.LoadSceneFile(pts)
    arrays = pt.StagedScene(); pt.close()
    cam = camera_from_scene(scene); cam["aperture"] = 0.0
    return arrays, cam


FLAT_CAM = dict(pos=np.array([0.0, 0.0, -3.4], np.float32), dir=np.array([0, 0, 1], np.float32), up=np.array([0, 1, 0], np.float32),
                focal=0.05, fovy=55.0, focal_dist=3.0, aperture=0.0)


class _Scenes:
    """flat: the FLAT Cornell golden (12 triangles); host / device: random scenes with textures, smoothing, normal and opacity
    maps, built by the host (300 triangles) and the device builder (6000); c4: the ~70 k-triangle blob at a small resolution"""

    def __init__(self, tmp_path):
        self.tmp = tmp_path

    def __getitem__(self, name):
        if name == "flat":
            return scene_from_golden(load_golden("tier_f_cornell.npz")), dict(FLAT_CAM), 1
        if name == "host":
            return random_scene(14, 300, True) + (1,)
        if name == "device":
            return random_scene(16, 6000, True) + (1,)
        return _c4_arrays(self.tmp) + (1,)


def _scenes(tmp_path):
    return _Scenes(tmp_path)


def _check_against_fresh(a, b, OB, moved, cam, what, oracle=True):
    """context a (updated) vs context b (fresh upload of the moved arrays) vs the oracle: image, hits, features, pick, tree"""
    _setup(b, moved, cam)
    acc_b, rgb_b = _render(b)
    acc_a, rgb_a = _render(a)
    assert np.array_equal(acc_a, acc_b) and np.array_equal(rgb_a, rgb_b), what
    if oracle:
        ref, ref8 = _oracle(OB, moved, cam)
        assert np.isfinite(ref).all() and (ref != 0).any(), what
        assert np.array_equal(acc_a, ref) and np.array_equal(rgb_a, ref8), what
    rng = np.random.default_rng(1)
    ext = float(np.abs(moved["verts"][np.isfinite(moved["verts"]).all(axis=1)]).max())
    ro = (rng.uniform(-1.2, 1.2, (2000, 3)) * min(ext, 8.0)).astype(np.float32)
    rd = rng.normal(0, 1, (2000, 3)).astype(np.float32); rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    ta, ua = a.probe_hits(ro, rd); tb_, ub = b.probe_hits(ro, rd)
    assert np.array_equal(ta, tb_) and np.array_equal(ua, ub), what
    from pbrpathtracer_amd import ptk
    a.render_features(ptk.FEAT_ALL, 0, 5); b.render_features(ptk.FEAT_ALL, 0, 5)
    for f in range(len(ptk.FEAT_NAMES)):
        assert np.array_equal(a.read_feature(f).view(np.uint32), b.read_feature(f).view(np.uint32)), (what, ptk.FEAT_NAMES[f])
    for x, y in ((W // 2, H // 2), (3, 5), (W - 2, H - 3)):
        assert a.pick(x, y, 5) == b.pick(x, y, 5), what
    nodes, order = a.download_bvh()
    fin = np.where(np.isfinite(moved["verts"]), moved["verts"], 0)
    info = check_bvh(nodes, order, fin)
    assert info["stack_need"] == a.bvh_layout()[2], what
    return nodes, order


@pytest.mark.parametrize("name", ["flat", "host", "device", "c4"])
def test_identity_update_changes_no_bit(ctxs, name, tmp_path):
    a, _ = ctxs
    arrays, cam, _ = _scenes(tmp_path)[name]
    _setup(a, arrays, cam)
    assert a.upload_timing()["built_on_device"] == (name in ("device", "c4"))
    assert a.geometry_info()["updates"] == 0 and not a.geometry_info()["refitted"]
    nodes0, order0 = a.download_bvh()
    acc0, rgb0 = _render(a)
    n = len(arrays["verts"])
    a.update_geometry(0, arrays["verts"], arrays["normals"], arrays["tbn"])
    a.update_geometry(n // 4, arrays["verts"][n // 4: n // 2 + 1])
    nodes1, order1 = a.download_bvh()
    assert np.array_equal(order0, order1)
    assert np.array_equal(nodes0.view(np.uint32), nodes1.view(np.uint32))
    acc1, rgb1 = _render(a)
    assert np.array_equal(acc0, acc1) and np.array_equal(rgb0, rgb1)
    gi = a.geometry_info()
    assert gi["updates"] == 2 and gi["refitted"] and gi["sah_built"] > 0 and gi["sah_now"] == gi["sah_built"]


@pytest.mark.parametrize("name", ["flat", "host", "device", "c4"])
@pytest.mark.parametrize("kind", ["rigid", "scale", "jitter", "collapse", "far"])
def test_moved_scene_equals_fresh_upload_and_oracle(ctxs, oracle_mod, name, kind, tmp_path):
    a, b = ctxs
    arrays, cam, _ = _scenes(tmp_path)[name]
    _setup(a, arrays, cam)
    nodes0, _ = a.download_bvh()
    stack0 = a.bvh_layout()[2]
    acc0, rgb0 = _render(a)
    first, nv, nn, tb, moved = _motion(arrays, kind)
    a.update_geometry(first, nv, nn, tb)
    nodes1, _ = _check_against_fresh(a, b, oracle_mod, moved, cam, (name, kind))
    assert np.array_equal(nodes0[:, LINKS].view(np.uint32), nodes1[:, LINKS].view(np.uint32))
    assert a.bvh_layout()[2] == stack0
    assert a.geometry_info()["sah_now"] > 0
    if kind == "far":
        # ... and back again: the uploaded scene, the uploaded image
        k = len(nv)
        a.update_geometry(first, arrays["verts"][first:first + k])
        acc1, rgb1 = _render(a)
        assert np.array_equal(acc0, acc1) and np.array_equal(rgb0, rgb1)
        check_bvh(*a.download_bvh(), arrays["verts"])


@pytest.mark.parametrize("kind", ["rigid", "scale", "far"])
@pytest.mark.parametrize("name", ["host", "device"])
def test_moved_scene_under_other_render_settings(ctxs, oracle_mod, name, kind, tmp_path):
    """primary cache on / off, thin lens (lens cull on), a 3-way tile split, the contracted builds against a fresh context"""
    a, b = ctxs
    arrays, cam, _ = _scenes(tmp_path)[name]
    first, nv, nn, tb, moved = _motion(arrays, kind)         # (scale, far: the extent, scene_bound and the lens cull's box change too)
    ref = {}
    for ap in (0.0, 0.08):
        cam2 = dict(cam); cam2["aperture"] = ap
        ref[ap] = _oracle(oracle_mod, moved, cam2)
    try:
        for ap in (0.0, 0.08):
            cam2 = dict(cam); cam2["aperture"] = ap
            for cache in (1, 0):
                a.set_option("primary_cache", cache)
                _setup(a, arrays, cam2)
                _render(a)                                   # fills the caches the update has to invalidate
                a.update_geometry(first, nv, nn, tb)
                acc, rgb = _render(a)
                assert np.array_equal(acc, ref[ap][0]) and np.array_equal(rgb, ref[ap][1]), (ap, cache)
            a.set_option("primary_cache", 1)
            # 3-way tile split: the three shares of the updated context add up to the oracle's image
            total = np.zeros_like(ref[ap][0])
            for r in range(3):
                a.set_tile(r, 3); a.reset(); a.render(0, SPP, 5)
                total += a.read_accum()
            a.set_tile(0, 1)
            assert np.array_equal(total, ref[ap][0]), ap
        for contract in (1, 2):
            cam2 = dict(cam); cam2["aperture"] = 0.0
            a.set_option("contract", contract); b.set_option("contract", contract)
            _setup(a, arrays, cam2); _render(a); a.update_geometry(first, nv, nn, tb)
            _setup(b, moved, cam2)
            assert np.array_equal(_render(a)[0], _render(b)[0]), contract
    finally:
        for c in (a, b):
            c.set_option("contract", 0); c.set_option("primary_cache", 1); c.set_tile(0, 1)


@pytest.mark.parametrize("caller_stream", [False, True])
def test_updates_are_ordered_between_queued_renders(oracle_mod, caller_stream, tmp_path):
    """render, update A, render, update B, render - queued without a host wait of the caller's, each render into its own bound
    accumulator: every accumulator holds the oracle's samples of the geometry of its moment"""
    import torch
    from pbrpathtracer_amd import ptk
    w, h = 128, 96                                           # 48 tiles: 1 MiB of pass_bytes makes every render several passes
    arrays, cam, _ = _scenes(tmp_path)["device"]
    fa, va, na, ta, moved_a = _motion(arrays, "rigid")
    fb, vb, _, _, moved_b = _motion(moved_a, "jitter")
    refs = [_oracle(oracle_mod, s, cam, first=8 * k, spp=8, w=w, h=h)[0] for k, s in enumerate((arrays, moved_a, moved_b))]
    stream = torch.cuda.Stream() if caller_stream else None
    a = ptk.Context(0)
    try:
        a.set_option("overlap", 1); a.set_option("pass_bytes", 1 << 20)
        if stream is not None:
            a.set_stream(stream.cuda_stream)
        _setup(a, arrays, cam, w, h)
        # (the one-off topology download and the staging buffer's allocation happen here, not between the renders)
        a.update_geometry(0, arrays["verts"], arrays["normals"], arrays["tbn"])
        acc = [torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        a.bind_accum(acc[0].data_ptr()); a.render(0, 8, 5)
        assert a.last_render_ms()[1] >= 6                    # two passes at least
        a.update_geometry(fa, va, na, ta)
        a.bind_accum(acc[1].data_ptr()); a.render(8, 8, 5)
        a.update_geometry(fb, vb)
        a.bind_accum(acc[2].data_ptr()); a.render(16, 8, 5)
        a.synchronize()
        for k in range(3):
            assert np.array_equal(acc[k].cpu().numpy(), refs[k]), k
    finally:
        a.synchronize()
        a.close()


@pytest.mark.parametrize("name", ["flat", "host", "device"])
def test_device_arrays_give_what_host_arrays_give(ctxs, name, tmp_path):
    """records (through renders) and nodes: within ONE context - so that two device builds' node numbering stays out of it - the
    tree after an update from host arrays, then after the same update from torch tensors on the GPU; and against a second
    context that only ever saw the device path"""
    import torch
    a, b = ctxs
    arrays, cam, _ = _scenes(tmp_path)[name]
    first, nv, nn, tb, moved = _motion(arrays, "rigid")
    _, jv, _, _, moved2 = _motion(moved, "jitter")
    dv, dn, dt, dj = (torch.from_numpy(x).cuda() for x in (nv, nn, tb, jv))
    torch.cuda.synchronize()
    _setup(a, arrays, cam); _setup(b, arrays, cam)
    back = arrays["verts"], arrays["normals"], arrays["tbn"]

    a.update_geometry(first, nv, nn, tb)
    nodes_h, order_h = a.download_bvh(); acc_h = _render(a); sah_h = a.geometry_info()["sah_now"]
    a.update_geometry(0, *back)                              # away again, so that the device update has something to change
    assert not np.array_equal(a.download_bvh()[0].view(np.uint32), nodes_h.view(np.uint32))
    a.update_geometry(first, dv, dn, dt)
    nodes_d, order_d = a.download_bvh(); acc_d = _render(a)
    assert np.array_equal(nodes_h.view(np.uint32), nodes_d.view(np.uint32)) and np.array_equal(order_h, order_d)
    assert np.array_equal(acc_h[0], acc_d[0]) and np.array_equal(acc_h[1], acc_d[1])
    assert a.geometry_info()["sah_now"] == sah_h
    b.update_geometry(first, dv, dn, dt)
    assert np.array_equal(_render(b)[0], acc_h[0])

    # vertices only, by address
    a.update_geometry(0, jv)
    nodes_h, _ = a.download_bvh(); acc_h = _render(a); sah_h = a.geometry_info()["sah_now"]
    a.update_geometry(0, moved["verts"])
    a.update_geometry(0, dj.data_ptr(), num_tris=len(jv))
    assert np.array_equal(nodes_h.view(np.uint32), a.download_bvh()[0].view(np.uint32))
    assert np.array_equal(_render(a)[0], acc_h[0]) and a.geometry_info()["sah_now"] == sah_h
    b.update_geometry(0, dj.data_ptr(), num_tris=len(jv))
    assert np.array_equal(_render(b)[0], acc_h[0])
    with pytest.raises(AssertionError):
        a.update_geometry(first, dv, dn[:-1], dt)            # the binding refuses arrays of different lengths


def test_refusals_leave_the_scene_unmoved(ctxs, tmp_path):
    from pbrpathtracer_amd import ptk
    import torch
    a, _ = ctxs
    c = ptk.Context(0)
    with pytest.raises(ptk.PtkError, match=r"\(-1\)"):
        c.update_geometry(0, np.zeros((1, 9), np.float32))   # before any upload
    c.close()
    for name in ("flat", "device"):
        arrays, cam, _ = _scenes(tmp_path)[name]
        n = len(arrays["verts"])
        _setup(a, arrays, cam)
        gi = a.geometry_info()
        assert gi["updates"] == 0 and not gi["refitted"]
        acc0, rgb0 = _render(a)
        nodes0, order0 = a.download_bvh()
        for bad in (np.nan, np.inf, -np.inf, 2.0 ** 61, -(2.0 ** 61)):
            v = arrays["verts"][1:4].copy(); v[1, 4] = bad
            with pytest.raises(ptk.PtkError, match=r"\(-4\)"):
                a.update_geometry(1, v)
            d = torch.from_numpy(v).cuda(); torch.cuda.synchronize()
            with pytest.raises(ptk.PtkError, match=r"\(-4\)"):
                a.update_geometry(1, d)
        for args in ((n - 1, arrays["verts"][:2]), (-1, arrays["verts"][:1]), (n, arrays["verts"][:1])):
            with pytest.raises(ptk.PtkError, match=r"\(-1\)"):
                a.update_geometry(*args)
        with pytest.raises(ptk.PtkError, match=r"\(-1\)"):
            a.update_geometry(0, arrays["verts"][:2], normals=arrays["normals"][:2])
        a.update_geometry(0, np.zeros((0, 9), np.float32))   # nothing to do is fine
        assert a.geometry_info()["updates"] == 0
        acc1, rgb1 = _render(a)
        assert np.array_equal(acc0, acc1) and np.array_equal(rgb0, rgb1)
        nodes1, order1 = a.download_bvh()
        assert np.array_equal(nodes0.view(np.uint32), nodes1.view(np.uint32)) and np.array_equal(order0, order1)
        a.update_geometry(0, arrays["verts"][:1])
        assert a.geometry_info()["updates"] == 1
        a.upload_scene(arrays)
        gi = a.geometry_info()
        assert gi["updates"] == 0 and not gi["refitted"]


def test_lights_and_materials_together(ctxs, oracle_mod, tmp_path):
    a, _ = ctxs
    arrays, cam, _ = _scenes(tmp_path)["host"]
    arrays = dict(arrays)
    lights = arrays["lights"]
    assert len(lights) >= 2
    _setup(a, arrays, cam)
    # the emissive triangles move
    lo, hi = int(lights.min()), int(lights.max()) + 1
    v1 = arrays["verts"][lo:hi] + np.tile(np.array([0.25, 0.1, 0.0], np.float32), 3)
    s1 = dict(arrays); s1["verts"] = arrays["verts"].copy(); s1["verts"][lo:hi] = v1
    a.update_geometry(lo, v1)
    r = _oracle(oracle_mod, s1, cam)
    acc, rgb = _render(a)
    assert np.array_equal(acc, r[0]) and np.array_equal(rgb, r[1])
    # ... change colour
    mats = arrays["materials"].copy()
    mats[0]["emissive"] = (0.2, 1.0, 0.3); mats[0]["emissive_intensity"] = 5.0
    s2 = dict(s1); s2["materials"] = mats
    a.update_materials(mats)
    r = _oracle(oracle_mod, s2, cam)
    acc, rgb = _render(a)
    assert np.array_equal(acc, r[0]) and np.array_equal(rgb, r[1])
    # ... and move again
    v3 = v1 + np.tile(np.array([-0.4, 0.0, 0.15], np.float32), 3)
    s3 = dict(s2); s3["verts"] = s1["verts"].copy(); s3["verts"][lo:hi] = v3
    a.update_geometry(lo, v3)
    r = _oracle(oracle_mod, s3, cam)                      # (the oracle takes the light list as given: the upload's order)
    acc, rgb = _render(a)
    assert np.array_equal(acc, r[0]) and np.array_equal(rgb, r[1])
    a.update_materials(mats)                              # a later material edit keeps the moved light vertices
    assert np.array_equal(_render(a)[0], r[0])


def test_host_class_moves_an_object(tmp_path):
    from pbrpathtracer_amd import scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    groups, mats = S.cornell_groups()
    box = str(tmp_path / "box.obj"); S.write_obj(box, groups)
    ball = str(tmp_path / "ball.obj"); S.write_obj(ball, [S.uv_sphere("ball", (0.0, 0.0, 0.0), 0.35, nu=24, nv=12)])
    M0 = np.eye(4, dtype=np.float32); M0[3][:3] = (-0.4, -0.5, 0.0)
    M1 = np.eye(4, dtype=np.float32); M1[0][0] = 1.4; M1[3][:3] = (0.35, 0.1, 0.2)
    k = 3

    def tracer(M):
        pt = PathTracer(0)
        pt.LoadObject(box); pt.LoadObject(ball, M)
        for j, m in enumerate(mats):
            pt.SetMaterial(0, j, m)
        pt.SetCamera((0.0, 0.0, -3.4), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)); pt.SetProjection(0.05, 55.0)
        pt.BuildBVH(); pt.SetResolution((W, H)); pt.SetTraceDepth(D); pt.SetSeed(9); pt.ResetImage()
        return pt

    a = tracer(M0)
    for _ in range(k):
        a.RenderFrame()
    a.SetObjectTransform(1, M1)
    a.ResetImage()
    for _ in range(k):
        a.RenderFrame()
    assert a.LastError() == ""
    b = tracer(M1)
    for _ in range(k):
        b.RenderFrame()
    assert a.GetSamples() == k
    assert np.array_equal(a.ReadAccumulation(), b.ReadAccumulation())
    assert a.context().geometry_info()["updates"] == 1
    sa, sb = a.StagedScene(), b.StagedScene()
    assert np.array_equal(sa["verts"], sb["verts"])
    # a pixel the moved ball covers: the projection of its centre
    hits = [(x, y) for y in range(H) for x in range(W) if b.Pick(x, y)[0] == 1]
    assert hits
    for x, y in hits[:: max(1, len(hits) // 8)]:
        assert a.Pick(x, y) == b.Pick(x, y) and a.Pick(x, y)[0] == 1
    # a refused update reaches LastError() and leaves the picture as it was
    bad = M1.copy(); bad[3][0] = np.inf
    a.SetObjectTransform(1, bad)
    a.ResetImage()
    for _ in range(k):
        a.RenderFrame()
    assert "2^61" in a.LastError()
    assert np.array_equal(a.ReadAccumulation(), b.ReadAccumulation())
    assert np.array_equal(a.StagedScene()["verts"], sb["verts"])       # the refused matrix is gone from the staging too
    a.SetDiffuseTextureForElement(1, 0, str(tmp_path / "no_such_texture.png")); b.SetDiffuseTextureForElement(1, 0, str(tmp_path / "no_such_texture.png"))
    for t in (a, b):                                        # a texture edit uploads the staged scene again: still the accepted one
        t.ResetImage()
        for _ in range(k):
            t.RenderFrame()
    assert np.array_equal(a.ReadAccumulation(), b.ReadAccumulation()) and np.isfinite(a.ReadAccumulation()).all()
    a.close(); b.close()


def test_plain_scene_stays_on_the_plain_kernel(ctxs, oracle_mod):
    from pbrpathtracer_amd import ptk
    a, _ = ctxs
    arrays = scene_from_golden(load_golden("tier_f_cornell.npz"))
    assert ptk.scene_is_plain(arrays)
    cam = dict(FLAT_CAM)
    _setup(a, arrays, cam)
    _render(a)
    assert a.trace_variant() == ptk.TRACE_FLAT_PLAIN
    first, nv, nn, tb, moved = _motion(arrays, "rigid")
    a.update_geometry(first, nv, nn, tb)
    acc, rgb = _render(a)
    assert a.trace_variant() == ptk.TRACE_FLAT_PLAIN
    ref = _oracle(oracle_mod, moved, cam)
    assert np.array_equal(acc, ref[0]) and np.array_equal(rgb, ref[1])


def test_update_is_faster_than_a_new_upload_at_1m_triangles(tmp_path):
    """C5, whole scene, host arrays, to synchronize: the median of five updates against the median of five uploads of the same
    arrays in the same process.  The re-upload is what a caller had before; nothing but 'faster' is asserted."""
    from pbrpathtracer_amd import scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    pts, scene, _ = S.build_config("C5", str(tmp_path))
    pt = PathTracer(0); pt.LoadSceneFile(pts)
    arrays = pt.StagedScene()
    c = pt.context()
    assert len(arrays["verts"]) >= 1_000_000
    v = (arrays["verts"] * np.float32(1.01)).astype(np.float32)
    c.update_geometry(0, v, arrays["normals"], arrays["tbn"]); c.synchronize()      # (tables of the first update)
    t_up, t_load = [], []
    for _ in range(5):
        t0 = time.perf_counter(); c.update_geometry(0, v, arrays["normals"], arrays["tbn"]); c.synchronize(); t_up.append(time.perf_counter() - t0)
    print("last update on the device:", c.geometry_timing())
    moved = dict(arrays); moved["verts"] = v
    for _ in range(5):
        t0 = time.perf_counter(); c.upload_scene(moved); c.synchronize(); t_load.append(time.perf_counter() - t0)
    up, load = float(np.median(t_up)), float(np.median(t_load))
    print(f"C5 ({len(v)} triangles): update_geometry {up * 1e3:.2f} ms, upload_scene {load * 1e3:.2f} ms")
    pt.close()
    assert up < load
