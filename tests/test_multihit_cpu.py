"""Ordered multi-hit ray queries (include/ptk.h ptk_multihit_rays) without a GPU: the entry points exist, the numpy
restatement of the rule (tests/multihit_rule.py) is the sorted list of crossings it claims to be - held to a float64 brute force on
closed meshes -, has the three consequences the header states, and the worked uses of rays.py do what they say on lists written
by hand."""
import os
import re

import numpy as np
import pytest

import closest_rule as CR
import crossings_rule as XR
import hit_rule as HR
import multihit_rule as MR
import ray_cases as RC

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_PTK = ("ptk_multihit_rays", "ptk_multihit_rays_device", "ptk_last_multihit_ms")
NEW_PTH = ("pth_multihit_rays",)


@pytest.fixture(autouse=True, scope="module")
def built_library():
    """every test here is about the feature the library must have"""
    from pbrpathtracer_amd import ptk
    L = ptk.load()
    for name in NEW_PTK + NEW_PTH:
        assert hasattr(L, name), name


def test_symbols_are_exported_and_declared():
    from pbrpathtracer_amd import ptk, pathtracer, rays
    L = ptk.load()
    head = open(os.path.join(ROOT, "include", "ptk.h")).read()
    text = head + open(os.path.join(ROOT, "include", "ptk_host.h")).read()
    declared = set(re.findall(r"\b(p(?:tk|th)_[a-z0-9_]+)\s*\(", text))
    for name in NEW_PTK + NEW_PTH:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in ptk.SYMBOLS + pathtracer.HOST_SYMBOLS, name
    assert int(re.search(r"#define PTK_MULTIHIT_MAX (\d+)", head).group(1)) == 16 == ptk.MULTIHIT_MAX == MR.MAX_HITS
    for cls, names in ((ptk.Context, ("multihit_rays", "last_multihit_ms")), (pathtracer.PathTracer, ("multihit_rays", "MultiHitRays"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("inside_length", "thickness", "layers_between"):
        assert callable(getattr(rays, name)), name


# ---- the mirror against float64 ----------------------------------------------------------------------------------------------------
def _brute64(verts, ro, rd):
    """(cross [n, m] bool, t, side, safe [n] bool) in float64: Moeller-Trumbore with the rule's tests; safe = the ray's float64
    crossings are at least 1e-4 apart in t and every triangle is crossed or missed clearly: u, v, 1 - u - v and t - 1e-5 all above
    1e-4 with |a| > 1e-3, or one of them below -1e-4 (below -1e-2 where |a| <= 1e-3: there f magnifies the rounding of the dots)"""
    tr = np.asarray(verts, np.float64).reshape(-1, 3, 3)
    v0, e1, e2 = tr[None, :, 0], (tr[:, 1] - tr[:, 0])[None], (tr[:, 2] - tr[:, 0])[None]
    o = np.asarray(ro, np.float64)[:, None]; d = np.asarray(rd, np.float64)[:, None]
    h = np.cross(d, e2)
    a = (e1 * h).sum(-1)
    with np.errstate(all="ignore"):
        f = 1.0 / a
        s = o - v0
        u = f * (s * h).sum(-1)
        q = np.cross(s, e1)
        v = f * (d * q).sum(-1)
        t = f * (e2 * q).sum(-1)
    cross = (np.abs(a) >= 1e-5) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-5)
    with np.errstate(invalid="ignore"):
        least = np.minimum(np.minimum(u, v), np.minimum(1 - u - v, t - 1e-5))
        clear = np.where(np.abs(a) > 1e-3, np.abs(least) > 1e-4, least < -1e-2)
    ts = np.sort(np.where(cross, t, np.inf), axis=1)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(ts[:, 1:]), ts[:, 1:] - ts[:, :-1], np.inf).min(axis=1)
    return cross, t, np.where(a > 0, 1, -1), clear.all(axis=1) & (gap >= 1e-4)


@pytest.mark.parametrize("name", XR.MESHES)
def test_mirror_equals_float64_brute_force(name):
    verts = XR.mesh(name)
    ro, rd = RC.rays_in_box(dict(verts=verts), 1000, 5)
    cross, t64, side64, safe = _brute64(verts, ro, rd)
    ncross = cross.sum(axis=1)
    print(f"{name}: {int(safe.sum())} of {len(ro)} rays are well apart, most crossings on one ray {int(ncross.max())}")
    assert safe.mean() > 0.5 and ncross.max() <= MR.MAX_HITS and (ncross[safe] >= 2).mean() > 0.1
    count, tri, t, bary, side = MR.multihit(dict(verts=verts), ro, rd, MR.MAX_HITS)
    assert (count.dtype, tri.dtype, t.dtype, bary.dtype, side.dtype) == (np.int32, np.int32, F32, F32, np.int8)
    assert tri.shape == t.shape == side.shape == (len(ro), 16) and bary.shape == (len(ro), 16, 2)
    pad = max(0, 16 - cross.shape[1])                                       # (a mesh of fewer than 16 triangles: columns that never cross)
    cross, t64, side64 = (np.pad(x, ((0, 0), (0, pad))) for x in (cross, t64, side64))
    order = np.argsort(np.where(cross, t64, np.inf), axis=1, kind="stable")[:, :16]
    rows = np.arange(len(ro))[:, None]
    kept = cross[rows, order]
    want_tri = np.where(kept, order, -1)
    assert np.array_equal(count[safe], ncross[safe])
    assert np.array_equal(tri[safe], want_tri[safe])
    assert np.array_equal(side[safe], np.where(kept, side64[rows, order], 0)[safe])
    want_t = np.where(kept, t64[rows, order], np.inf)
    m = safe[:, None] & kept
    assert (np.abs(t[m] - want_t[m]) <= 1e-5 * np.abs(want_t[m])).all()
    assert np.isposinf(t[~kept & safe[:, None]]).all() and (bary[~kept & safe[:, None]] == 0).all()


# ---- the three consequences, within the mirror ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("torus", "soup"))
def test_prefix_and_count(name):
    verts = XR.mesh(name) if name != "soup" else MR.soup(1500, 0.5, 7)
    arrays = dict(verts=verts)
    ro, rd = RC.rays_in_box(arrays, 300, 11)
    tm = np.random.default_rng(3).uniform(0.0, 2.0, len(ro)).astype(F32)
    for tmax in (None, tm):
        full = MR.multihit(arrays, ro, rd, 16, tmax)
        front, back = XR.crossings(arrays, ro, rd, tmax)
        for k in (1, 2, 3, 5, 8, 16):
            got = MR.multihit(arrays, ro, rd, k, tmax)
            for g, w, nm in zip(got, MR.cut(full, k), MR.NAMES):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (k, nm)
            assert np.array_equal(got[0], np.minimum(k, front + back))
            kept = np.arange(k)[None, :] < got[0][:, None]
            assert (got[1][kept] >= 0).all() and (got[1][~kept] == -1).all() and np.isposinf(got[2][~kept]).all()
            assert (np.abs(got[4][kept]) == 1).all() and (got[4][~kept] == 0).all() and (got[3][~kept] == 0).all()
            with np.errstate(invalid="ignore"):                             # (inf - inf behind a list's end: not looked at)
                assert (np.diff(got[2], axis=1) >= 0)[kept[:, 1:]].all()
        if name == "soup":
            assert (front + back > 3).mean() > 0.2


def test_one_hit_is_the_closest_hit(oracle_mod):
    arrays = CR.scene_of(XR.mesh("cube"))
    ro, rd = RC.rays_in_box(arrays, 600, 5)
    tri, t, bary, _ = HR.mirror(oracle_mod, arrays, ro, rd, HR.PROBE_KEY)
    count, mtri, mt, mbary, side = MR.multihit(arrays, ro, rd, 1)
    assert (tri >= 0).mean() > 0.5
    assert np.array_equal(mtri[:, 0], tri) and np.array_equal(mt[:, 0], t) and np.array_equal(mbary[:, 0], bary)
    assert np.array_equal(count, (tri >= 0).astype(np.int32)) and np.array_equal(side[:, 0] != 0, tri >= 0)


def test_refuses_a_list_length_outside_1_to_16():
    for k in (0, 17, -1):
        with pytest.raises(ValueError):
            MR.multihit(dict(verts=XR.mesh("cube")), np.zeros((1, 3), F32), np.ones((1, 3), F32), k)


# ---- rays.inside_length on lists written by hand --------------------------------------------------------------------------------------
def test_inside_length():
    from pbrpathtracer_amd import rays
    inf = np.inf
    count = np.array([2, 4, 4, 0, 1, 2], np.int32)
    t = np.array([[1.0, 3.0, inf, inf],             # a cube entered and left
                  [1.0, 1.0, 2.5, 2.5],             # through a shared edge both neighbours accept, in and out
                  [1.0, 2.0, 4.0, 7.0],             # a list cut at K = 4 while inside the second solid
                  [inf, inf, inf, inf],             # nothing
                  [2.0, inf, inf, inf],             # entered and never left (an open mesh, or the origin was inside)
                  [1.0, 3.0, inf, inf]], F32)       # the same cube wound the other way
    side = np.array([[1, -1, 0, 0], [1, 1, -1, -1], [1, -1, 1, -1], [0, 0, 0, 0], [1, 0, 0, 0], [-1, 1, 0, 0]], np.int8)
    length, complete = rays.inside_length(count, t, side, 4)
    assert length.dtype == F32 and complete.dtype == bool
    assert length.tolist() == [2.0, 1.5, 4.0, 0.0, 0.0, 2.0]
    assert complete.tolist() == [True, False, False, True, True, True]
    e = rays.inside_length(np.zeros(0, np.int32), np.zeros((0, 4), F32), np.zeros((0, 4), np.int8), 4)
    assert e[0].shape == (0,) and e[1].shape == (0,)
    one = rays.inside_length(np.array([1], np.int32), np.array([[2.0]], F32), np.array([[1]], np.int8), 1)
    assert one[0].tolist() == [0.0] and one[1].tolist() == [False]


# ---- the slabs: exact ties ------------------------------------------------------------------------------------------------------------
def test_slabs_along_z():
    verts = MR.slabs(24)
    assert verts.shape == (60, 9) and verts.dtype == F32
    rng = np.random.default_rng(2)
    n = 64
    xy = rng.uniform(-0.9, 0.9, (n, 2))
    ro = np.c_[xy, np.where(np.arange(n) % 2, 1.5, -0.5)].astype(F32)
    rd = np.c_[np.zeros((n, 2)), np.where(np.arange(n) % 2, -1.0, 1.0)].astype(F32)
    front, back = XR.crossings(dict(verts=verts), ro, rd)
    assert (front + back == 30).all()
    count, tri, t, bary, side = MR.multihit(dict(verts=verts), ro, rd, 16)
    assert (count == 16).all() and (np.diff(t, axis=1) >= 0).all()
    tie = np.diff(t, axis=1) == 0
    assert (tie.sum(axis=1) >= 3).all()
    assert (np.diff(tri, axis=1)[tie] == 2).all()                           # a square's copy follows it: the smaller index first
    first = verts.reshape(-1, 3, 3)[tri[:, 0], 0, 2]
    assert np.array_equal(first == 0, np.arange(n) % 2 == 0)                 # from below the first square is z = 0
    eight = MR.multihit(dict(verts=verts), ro, rd, 8)
    assert (np.diff(eight[2], axis=1) == 0).any(axis=1).all()
