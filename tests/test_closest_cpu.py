"""Closest-point queries (include/ptk.h ptk_closest_points) without a GPU: the entry points exist, the numpy mirror
of the rule (tests/closest_rule.py) really finds closest points - held to an independent float64 computation within the slack
DESIGN derives -, the point sets of tests/test_gpu_closest.py reach every arm of the rule, ties and both sides of a radius, and
probes.relocate's arithmetic."""
import os
import re

import numpy as np
import pytest

import closest_rule as CR
import ray_cases as RC

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_CASES = ("random16", "random300", "random6000")


def points_of(case):
    arrays, _ = RC.scene(case)
    return arrays, RC.rays_in_box(arrays, 400, 5)[0]


_full = {}


def full(case):
    """mirror_full of a case's 400 points; computed once, not to be modified"""
    if case not in _full:
        arrays, pts = points_of(case)
        _full[case] = CR.mirror_full(arrays, pts)
    return _full[case]


def test_symbols_are_exported_and_declared():
    from pbrpathtracer_amd import ptk, pathtracer
    L = ptk.load()
    text = open(os.path.join(ROOT, "include", "ptk.h")).read() + open(os.path.join(ROOT, "include", "ptk_host.h")).read()
    declared = set(re.findall(r"\b(p(?:tk|th)_[a-z0-9_]+)\s*\(", text))
    for name in ("ptk_closest_points", "ptk_closest_points_device", "ptk_last_closest_ms", "pth_closest_points"):
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in ptk.SYMBOLS + pathtracer.HOST_SYMBOLS, name


@pytest.mark.parametrize("case", ("s_cornell",) + RANDOM_CASES)
def test_mirror_finds_closest_points(case):
    """dist within E + REL x dist of the float64 minimum over every triangle (E, REL: the prune's slack), and the winner
    one of the float64 minimisers within that bound; q lies that near its triangle and bary reproduces it"""
    arrays, pts = points_of(case)
    m = full(case)
    verts = np.asarray(arrays["verts"], F32).reshape(-1, 9)
    d64 = CR.distances64(verts, pts)
    want = d64.min(axis=1)
    bound = CR.slack(verts, pts) + CR.REL_SLACK * want
    assert (m["tri"] >= 0).all() and np.isfinite(m["dist"]).all()
    err = np.abs(m["dist"].astype(np.float64) - want)
    print(f"{case}: largest |dist - float64 minimum| / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float((err / bound).max())
    own = d64[np.arange(len(pts)), m["tri"]]
    assert (own <= want + bound).all()
    # the returned point: at the returned distance from p, on its triangle within E, and the barycentrics give it back
    q = m["point"].astype(np.float64)
    assert (np.abs(np.linalg.norm(pts.astype(np.float64) - q, axis=1) - m["dist"]) <= bound).all()
    t = verts.reshape(-1, 3, 3)[m["tri"]].astype(np.float64)
    v, w = m["bary"][:, 0].astype(np.float64), m["bary"][:, 1].astype(np.float64)
    assert (v >= 0).all() and (w >= 0).all() and (v + w <= 1 + 2.0 ** -24).all()
    rebuilt = t[:, 0] + (t[:, 1] - t[:, 0]) * v[:, None] + (t[:, 2] - t[:, 0]) * w[:, None]
    assert (np.linalg.norm(rebuilt - q, axis=1) <= CR.slack(verts, pts)).all()


@pytest.mark.parametrize("case", RANDOM_CASES)
def test_every_region_wins(case):
    m = full(case)
    counts = {r: int((m["region"] == r).sum()) for r in (0, 1, 2, 3, 4, 5, 7)}
    print(case, counts)
    assert min(counts.values()) >= 8, counts
    assert sum(counts.values()) == 400


def test_cornell_has_tied_minima():
    m = full("s_cornell")
    tied = int((m["ties"] >= 2).sum())
    print("s_cornell: queries with a tied minimum", tied)
    assert tied >= 10


def test_grid_mesh_ties_go_to_the_smallest_index():
    verts, pts = CR.grid_mesh()
    assert verts.shape == (4608, 9) and len(pts) >= 200
    m = CR.mirror_full(CR.scene_of(verts), pts)
    assert (m["ties"] >= 2).mean() >= 0.25, float((m["ties"] >= 2).mean())
    assert (m["dist"] == F32(CR.GRID_HEIGHT)).all()                       # exact arithmetic: straight down
    # the smallest index among the float64 minimisers (exact here)
    d64 = CR.distances64(verts, pts)
    first = np.argmax(d64 == d64.min(axis=1, keepdims=True), axis=1)
    assert np.array_equal(m["tri"], first.astype(np.int32))
    assert ((d64 == d64.min(axis=1, keepdims=True)).sum(axis=1) == m["ties"]).all()


@pytest.mark.parametrize("case", ("random16", "random300"))
def test_radius_set_splits_the_points(case):
    arrays, pts = points_of(case)
    m = full(case)
    md = radius_set(m["dist"], len(pts))
    r = CR.mirror_full(arrays, pts, md)
    share = float((r["tri"] >= 0).mean())
    assert 0.15 <= share <= 0.85, share
    hit = r["tri"] >= 0
    assert (m["dist"][hit] <= md[hit]).all() and (m["dist"][~hit] >= md[~hit]).all()     # (strict in d2k < max_dist^2; the roots may round together)
    for k in ("tri", "dist", "point", "bary"):
        assert np.array_equal(r[k][hit], m[k][hit])
    for bad in (np.nan, 0.0, -0.0, -1.0, -np.inf):
        assert (CR.mirror(arrays, pts[:20], np.full(20, bad, F32))[0] == -1).all(), bad
    assert np.array_equal(CR.mirror(arrays, pts[:20], np.full(20, np.inf, F32))[0], m["tri"][:20])


def radius_set(dist, n, seed=11):
    """max_dist uniform in [0, 2 x the median distance]"""
    return np.random.default_rng(seed).uniform(0.0, 2.0 * float(np.median(dist)), n).astype(F32)


def test_degenerate_triangles_give_finite_answers():
    verts, pts = CR.degenerate_mix()
    m = CR.mirror_full(CR.scene_of(verts), pts)
    assert (m["tri"] >= 0).all() and np.isfinite(m["dist"]).all() and np.isfinite(m["point"]).all() and np.isfinite(m["bary"]).all()
    assert (m["tri"] % 4 == 0).sum() >= 50                                # degenerate triangles do win
    d64 = CR.distances64(verts, pts).min(axis=1)
    bound = CR.slack(verts, pts) + CR.REL_SLACK * d64
    # never nearer than the nearest triangle (what the walk's pruning needs), whatever a degenerate triangle's arithmetic does
    assert (m["dist"].astype(np.float64) >= d64 - bound).all()


def test_far_clusters_mirror_is_conservative():
    verts, pts = CR.far_clusters()
    m = CR.mirror_full(CR.scene_of(verts), pts)
    d64 = CR.distances64(verts, pts).min(axis=1)
    bound = CR.slack(verts, pts) + CR.REL_SLACK * d64
    assert (m["tri"] >= 0).all()
    assert (m["dist"].astype(np.float64) >= d64 - bound).all()
    assert (np.abs(pts).max(axis=1) >= 1e5 * 2e3 * 0.2).sum() >= 100        # points about 1e5 scene sizes away


def test_relocate_arithmetic():
    from pbrpathtracer_amd import probes

    class Fake:
        """closest_points fed by hand: probe 0 too near, 1 on the surface (dist 0), 2 a miss, 3 too near along a slanted line"""
        def closest_points(self, points, max_dist=None):
            assert max_dist is not None and (np.asarray(max_dist) == F32(0.5)).all() and len(max_dist) == len(points)
            tri = np.array([4, 2, -1, 0], np.int32)
            point = np.array([[1, 1, 0], [2, 2, 2], [0, 0, 0], [0, 0, 0]], F32)
            dist = np.array([0.25, 0.0, np.inf, 0.3], F32)
            return tri, dist, point, np.zeros((4, 2), F32)

    pos = np.array([[1, 1, 0.25], [2, 2, 2], [9, 9, 9], [0.1, 0.2, 0.2]], F32)
    new, moved = probes.relocate(Fake(), pos, 0.5)
    assert new.dtype == F32 and new.shape == (4, 3) and moved.tolist() == [True, False, False, True]
    assert np.array_equal(new[1], pos[1]) and np.array_equal(new[2], pos[2])
    assert np.array_equal(new[0], np.array([1, 1, 0.5], F32))
    s = F32(0.5) / F32(0.3)
    assert np.array_equal(new[3], (pos[3] - F32(0)) * s)
    d, p, t = probes.clearance(Fake2(), pos)
    assert np.array_equal(d, np.arange(4, dtype=F32)) and p.shape == (4, 3) and t.dtype == np.int32


class Fake2:
    def closest_points(self, points, max_dist=None):
        assert max_dist is None
        n = len(points)
        return np.zeros(n, np.int32), np.arange(n, dtype=F32), np.zeros((n, 3), F32), np.zeros((n, 2), F32)
