"""Crossing counts, point containment and the signed distance (include/ptk.h ptk_crossings_rays, ptk_contains_points,
ptk_signed_distance) without a GPU: the entry points exist, the numpy restatement of the rule
(tests/crossings_rule.py) really is the containment it claims to be - held to the float64 solid-angle winding number on closed
meshes, every point -, agrees with the occlusion rule the product already has, and behaves at its edges as the header says."""
import os
import re

import numpy as np
import pytest

import crossings_rule as XR
import hit_rule as HR
import ray_cases as RC

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_PTK = ("ptk_crossings_rays", "ptk_crossings_rays_device", "ptk_contains_points", "ptk_contains_points_device",
           "ptk_inside_default_dirs", "ptk_signed_distance", "ptk_signed_distance_device", "ptk_last_crossings_ms")
NEW_PTH = ("pth_crossings_rays", "pth_contains_points", "pth_signed_distance")
OPAQUE_CASES = ("s_cornell", "s_glass")


@pytest.fixture(autouse=True, scope="module")
def built_library():
    """every test here is about the feature the library must have"""
    from pbrpathtracer_amd import ptk
    L = ptk.load()
    for name in NEW_PTK + NEW_PTH:
        assert hasattr(L, name), name


def default_dirs():
    from pbrpathtracer_amd import ptk
    return ptk.inside_default_dirs()


def test_symbols_are_exported_and_declared():
    from pbrpathtracer_amd import ptk, pathtracer
    L = ptk.load()
    text = open(os.path.join(ROOT, "include", "ptk.h")).read() + open(os.path.join(ROOT, "include", "ptk_host.h")).read()
    declared = set(re.findall(r"\b(p(?:tk|th)_[a-z0-9_]+)\s*\(", text))
    for name in NEW_PTK + NEW_PTH:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in ptk.SYMBOLS + pathtracer.HOST_SYMBOLS, name
    for cls, names in ((ptk.Context, ("crossings_rays", "contains_points", "signed_distance", "last_crossings_ms")),
                       (pathtracer.PathTracer, ("crossings_rays", "contains_points", "signed_distance"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)


def test_default_directions():
    """the built-in set is the float32 normalisation of the header's three vectors and has the properties the header states"""
    d = default_dirs()
    assert d.dtype == F32 and d.shape == (3, 3)
    src = np.array([(0.5377, 0.7283, 0.4251), (-0.3119, 0.4673, -0.8273), (0.6931, -0.6173, 0.3719)])
    assert np.array_equal(d, (src / np.linalg.norm(src, axis=1, keepdims=True)).astype(F32))
    text = open(os.path.join(ROOT, "include", "ptk.h")).read()
    lits = re.search(r"#define PTK_INSIDE_DEFAULT_DIRS \{([^}]*)\}", text).group(1)
    assert np.array_equal(np.array([F32(x.strip().rstrip("f")) for x in lits.split(",")], F32).reshape(3, 3), d)
    d64 = d.astype(np.float64)
    assert (np.abs(np.linalg.norm(d64, axis=1) - 1.0) < 1e-6).all()
    assert (np.abs(d64) > 0.3).all()                                        # no zero component: not along an axis or in an axis plane
    for i in range(3):
        for j in range(i + 1, 3):
            assert abs(d64[i] @ d64[j]) < 0.9                               # no two parallel
    a = np.sort(np.abs(d64), axis=1)
    # not along a face diagonal (two equal components, one zero) or a body diagonal (three equal): the components differ clearly
    assert (a[:, 1] - a[:, 0] > 0.05).all() and (a[:, 2] - a[:, 1] > 0.05).all()


@pytest.mark.parametrize("name", XR.MESHES)
def test_rule_is_containment(name):
    """WINDING and PARITY with the built-in directions equal the float64 winding number, |w| > 0.5, for EVERY point: 4096 uniform in
    the bounds enlarged by 20 % and a 9 x 9 x 9 lattice over the bounds padded by 0.25, rounded to float32"""
    verts = XR.mesh(name)
    assert len(verts) == {"cube": 12, "cube flipped": 12, "icosphere": 320, "torus": 256}[name]
    pts = XR.mesh_points(verts)
    assert pts.dtype == F32 and pts.shape == (4096 + 729, 3)
    w = XR.winding_number64(verts, pts)
    margin = float(np.abs(np.abs(w) - 0.5).min())
    want = np.abs(w) > 0.5
    assert 0.1 < want.mean() < 0.9
    arrays = dict(verts=verts)
    dirs = default_dirs()
    for mode in (XR.WINDING, XR.PARITY):
        inside, winding = XR.contains(arrays, pts, dirs, mode)
        wrong = int((inside.astype(bool) != want).sum())
        single = [int(((winding[:, j] != 0) != want).sum()) for j in range(3)]
        print(f"{name} mode {mode}: {wrong} wrong of {len(pts)}, per direction (winding != 0) {single}, least | |w| - 0.5 | {margin:.3g}")
        assert inside.dtype == np.uint8 and winding.dtype == np.int32 and winding.shape == (len(pts), 3)
        assert wrong == 0, (name, mode, np.nonzero(inside.astype(bool) != want)[0][:5].tolist())
    assert margin > 1e-3                                                    # the reference itself is nowhere near undecided
    # the winding number's sign is the mesh's orientation: back - front = +1 inside a mesh wound outward, -1 wound inward
    inside, winding = XR.contains(arrays, pts, dirs, XR.WINDING)
    sign = -1 if name == "cube flipped" else 1
    assert (winding[want] == sign).all() and (winding[~want] == 0).all()


@pytest.mark.parametrize("case", OPAQUE_CASES)
def test_consistent_with_the_occlusion_rule(oracle_mod, case):
    """on a scene without opacity maps, some triangle crosses before tmax exactly when the oracle's closest hit lies before tmax"""
    import walker_limit_cases as WC
    arrays, _ = RC.scene(case)
    a = oracle_mod.normalise_arrays(arrays)
    assert (a["materials"]["tex"][:, HR.OPACITY_SLOT] < 0).all(), "an opaque scene"
    ro, rd = RC.rays_in_box(arrays, 400, 5)
    tri, t, _, _ = HR.mirror(oracle_mod, arrays, ro, rd, HR.PROBE_KEY)
    assert 0.5 < (tri >= 0).mean()
    for label, tmax in WC.occlusion_bounds(t):
        front, back = XR.crossings(arrays, ro, rd, tmax)
        assert front.dtype == back.dtype == np.int32
        assert np.array_equal((front + back > 0).astype(np.uint8), HR.occluded(t, tmax)), (case, label)
    front, back = XR.crossings(arrays, ro, rd)
    assert (front + back).max() >= 2                                        # rays do pass through several surfaces


def test_edges_of_the_rule():
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], F32)                       # counter-clockwise seen from +z
    arrays = dict(verts=tri)
    o = np.array([[0.25, 0.25, 1.0]], F32); down = np.array([[0, 0, -1.0]], F32); up = -down
    assert [int(x[0]) for x in XR.crossings(arrays, o, down)] == [1, 0]      # from the counter-clockwise side: front
    assert [int(x[0]) for x in XR.crossings(arrays, o * F32(-1) + F32(0.5) * np.array([[1, 1, 0]], F32), up)] == [0, 1]
    assert [int(x[0]) for x in XR.crossings(arrays, o, up)] == [0, 0]        # behind the origin
    # tmax: the crossing lies at t = 1 exactly; strict
    for tmax, want in ((np.nan, 0), (0.0, 0), (-0.0, 0), (-1.0, 0), (-np.inf, 0), (np.inf, 1), (1.0, 0), (np.nextafter(F32(1), F32(2)), 1), (0.5, 0), (2.0, 1)):
        front, back = XR.crossings(arrays, o, down, np.array([tmax], F32))
        assert (int(front[0]), int(back[0])) == (want, 0), tmax
    # t > 1e-5: a ray that starts on the triangle does not cross it
    assert XR.crossings(arrays, np.array([[0.25, 0.25, 0.0]], F32), down)[0][0] == 0
    # directions are used as given: t is in units of |dir|
    assert XR.crossings(arrays, o, down * F32(4), np.array([0.25], F32))[0][0] == 0
    assert XR.crossings(arrays, o, down * F32(4), np.array([0.26], F32))[0][0] == 1
    # a ray in the triangle's plane, and degenerate triangles (two equal vertices, three equal, collinear): |a| < 1e-5 or a NaN
    inplane_o = np.array([[-1.0, 0.25, 0.0]], F32); inplane_d = np.array([[1.0, 0, 0]], F32)
    assert [int(x[0]) for x in XR.crossings(arrays, inplane_o, inplane_d)] == [0, 0]
    deg = np.array([[0, 0, 0, 0, 0, 0, 0, 1, 0], [0.2, 0.2, 0, 0.2, 0.2, 0, 0.2, 0.2, 0], [0, 0, 0, 0.5, 0.5, 0, 1, 1, 0]], F32)
    both = dict(verts=np.concatenate([deg, tri]))
    assert [int(x[0]) for x in XR.crossings(dict(verts=deg), o, down)] == [0, 0]
    assert [int(x[0]) for x in XR.crossings(both, o, down)] == [1, 0]
    # coincident triangles each count
    assert [int(x[0]) for x in XR.crossings(dict(verts=np.concatenate([tri, tri, tri])), o, down)] == [3, 0]
    # no triangles, no rays
    assert [x.tolist() for x in XR.crossings(dict(verts=np.zeros((0, 9), F32)), o, down)] == [[0], [0]]
    assert [x.shape for x in XR.crossings(arrays, np.zeros((0, 3), F32), np.zeros((0, 3), F32))] == [(0,), (0,)]


def test_votes_majority_and_the_sign_flip():
    front = np.array([0, 1, 1, 2, 0], np.int32); back = np.array([0, 0, 1, 1, 3], np.int32)
    assert XR.votes(front, back, XR.WINDING).tolist() == [False, True, False, True, True]
    assert XR.votes(front, back, XR.PARITY).tolist() == [False, True, False, True, True]
    assert XR.votes(np.array([2]), np.array([0]), XR.WINDING).tolist() == [True] and XR.votes(np.array([2]), np.array([0]), XR.PARITY).tolist() == [False]
    for D in (0, 2, 4, 30, 32, 33, -1):
        with pytest.raises(ValueError):
            XR.check_dirs(D, XR.WINDING)
    for D in (1, 3, 31):
        XR.check_dirs(D, XR.PARITY)
    with pytest.raises(ValueError):
        XR.check_dirs(3, 2)
    # a majority of an odd D: one direction of three that grazes does not decide
    cube = dict(verts=XR.mesh("cube"))
    p = np.array([[0.1, 0.2, 0.3], [3.0, 0.2, 0.3]], F32)
    d5 = np.concatenate([default_dirs(), -default_dirs()[:2]])
    inside, winding = XR.contains(cube, p, d5)
    assert inside.tolist() == [1, 0] and winding.shape == (2, 5) and (winding[0] == 1).all() and (winding[1] == 0).all()
    dist = np.array([1.5, 0.0, np.inf, 2.0], F32)
    got = XR.flip_sign(dist, np.array([1, 1, 1, 0], np.uint8))
    assert got.dtype == F32 and got.tolist() == [-1.5, -0.0, -np.inf, 2.0] and np.signbit(got).tolist() == [True, True, True, False]
    assert np.array_equal(np.abs(got), dist)


def test_refusals_that_need_no_gpu():
    from pbrpathtracer_amd import ptk
    L = ptk.load()
    BAD = -1
    assert L.ptk_inside_default_dirs(None) == BAD
    assert L.ptk_last_crossings_ms(None, None) == BAD
    out = np.full(4, 77, np.int32)
    o = np.zeros((4, 3), F32)
    assert L.ptk_crossings_rays(None, 4, o.ctypes.data, o.ctypes.data, None, out.ctypes.data, None) == BAD
    assert L.ptk_crossings_rays_device(None, 4, o.ctypes.data, o.ctypes.data, None, out.ctypes.data, None) == BAD
    assert L.ptk_contains_points(None, 4, o.ctypes.data, 3, None, 0, None, out.ctypes.data) == BAD
    assert L.ptk_signed_distance(None, 4, o.ctypes.data, None, 3, None, 0, out.ctypes.data, None, None, None) == BAD
    assert (out == 77).all()
    assert ptk.inside_mode("winding") == ptk.INSIDE_WINDING == XR.WINDING and ptk.inside_mode("parity") == ptk.INSIDE_PARITY == XR.PARITY
    assert ptk.inside_mode(1) == 1
    for bad in ("odd", 2, -1):
        with pytest.raises(ptk.PtkError):
            ptk.inside_mode(bad)


def test_worked_uses_arithmetic():
    from pbrpathtracer_amd import probes, rays

    class Fake:
        """closest_points and contains_points fed by hand: probe 0 too near, 1 too near and inside, 2 a miss, 3 a miss and inside"""
        def closest_points(self, points, max_dist=None):
            return (np.array([4, 2, -1, -1], np.int32), np.array([0.25, 0.25, np.inf, np.inf], F32),
                    np.array([[1, 1, 0], [2, 2, 2], [0, 0, 0], [0, 0, 0]], F32), np.zeros((4, 2), F32))

        def contains_points(self, points, dirs=None, mode=0, want_winding=False):
            assert dirs is None and not want_winding and len(points) == 4
            return np.array([0, 1, 0, 1], np.uint8)

        def crossings_rays(self, origins, dirs, tmax=None):
            assert np.array_equal(origins, a) and np.array_equal(dirs, b - a) and (tmax == 1).all()
            return np.array([0, 2], np.int32), np.array([1, 2], np.int32)

    pos = np.array([[1, 1, 0.25], [2, 2, 2.25], [9, 9, 9], [5, 5, 5]], F32)
    plain = probes.relocate(Fake(), pos, 0.5)
    assert len(plain) == 2 and plain[1].tolist() == [True, True, False, False]            # the default: today's return value
    new, moved, keep = probes.relocate(Fake(), pos, 0.5, drop_inside=True)
    assert keep.dtype == bool and keep.tolist() == [True, False, True, False]
    assert moved.tolist() == [True, False, False, False]
    assert np.array_equal(new[0], plain[0][0]) and np.array_equal(new[1:], pos[1:])
    assert probes.inside(Fake(), pos).tolist() == [False, True, False, True]
    a = np.array([[0, 0, 0], [1, 1, 1]], F32); b = np.array([[1, 0, 0], [3, 1, 1]], F32)
    layers = rays.count_layers(Fake(), a, b)
    assert layers.dtype == np.int32 and layers.tolist() == [1, 4]
