"""Overlap queries (include/ptk.h ptk_overlap_boxes, ptk_overlap_spheres) without a GPU: the entry points exist, the
numpy mirror of the two rules (tests/overlap_rule.py) really finds the triangles that meet a box or a sphere - held to an independent
float64 separating-axis gap and to float64 distances -, every one of the 13 axes decides pairs of its own, the query sets of
tests/test_gpu_overlap.py are cut off by k for some queries and not for others, and overlap.py's paging and voxel arithmetic."""
import os
import re

import numpy as np
import pytest

import closest_rule as CR
import overlap_rule as OR
import ray_cases as RC

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("s_cornell", "random16", "random300", "random6000")
GAP, LEFT_OUT = 1e-5, 1e-4


_sets = {}


def query_set(name):
    """(verts, lo, hi) of a case or of a generated scene (n, sig, seed); computed once, not to be modified"""
    if name not in _sets:
        if isinstance(name, tuple):
            _sets[name] = OR.generated(*name)
        else:
            arrays, _ = RC.scene(name)
            _sets[name] = (np.asarray(arrays["verts"], F32).reshape(-1, 9),) + OR.boxes_in_bounds(arrays, 400, 7)
    return _sets[name]


def test_symbols_are_exported_and_declared():
    from pbrpathtracer_amd import ptk, pathtracer
    L = ptk.load()
    text = open(os.path.join(ROOT, "include", "ptk.h")).read() + open(os.path.join(ROOT, "include", "ptk_host.h")).read()
    declared = set(re.findall(r"\b(p(?:tk|th)_[a-z0-9_]+)\s*\(", text))
    for name in ("ptk_overlap_boxes", "ptk_overlap_boxes_device", "ptk_overlap_spheres", "ptk_overlap_spheres_device", "ptk_last_overlap_ms",
                 "ptk_overlap_stats", "pth_overlap_boxes", "pth_overlap_spheres"):
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in ptk.SYMBOLS + pathtracer.HOST_SYMBOLS, name
    assert ptk.OVERLAP_MAX_K == OR.MAX_K == int(re.search(r"#define PTK_OVERLAP_MAX_K (\d+)", text).group(1))


@pytest.mark.parametrize("name", CASES + OR.GENERATED, ids=str)
def test_box_rule_against_float64(name):
    """accepted == (gap <= 0) wherever the float64 gap is decided, |gap| > 1e-5, and all but 1e-4 of the pairs are decided"""
    verts, lo, hi = query_set(name)
    acc = OR.accepted_boxes(verts, lo, hi)
    gap = OR.sat_gap64(verts, lo, hi)
    decided = np.abs(gap) > GAP
    left = float((~decided).mean())
    wrong = int((acc != (gap <= 0))[decided].sum())
    print(f"{name}: left out {left:.2e}, mismatches {wrong}, accepted per box {acc.sum(axis=1).mean():.2f}")
    assert left <= LEFT_OUT, left
    assert wrong == 0, wrong


@pytest.mark.parametrize("name", CASES + OR.GENERATED, ids=str)
def test_sphere_rule_against_float64(name):
    """accepted == (distance < r) outside a band of slack + REL x r around r (the closest rule's slack)"""
    verts, lo, hi = query_set(name)
    centers, radius = OR.spheres_of(lo, hi)
    acc = OR.accepted_spheres(verts, centers, radius)
    d64 = CR.distances64(verts, centers)
    r = radius.astype(np.float64)[:, None]
    decided = np.abs(d64 - r) > CR.slack(verts, centers)[:, None] + CR.REL_SLACK * r
    left = float((~decided).mean())
    wrong = int((acc != (d64 < r))[decided].sum())
    print(f"{name}: left out {left:.2e}, mismatches {wrong}, accepted per sphere {acc.sum(axis=1).mean():.2f}")
    assert left <= LEFT_OUT, left
    assert wrong == 0, wrong


def test_census_every_axis_decides_and_k_cuts_some_lists():
    verts, lo, hi = query_set(OR.GENERATED[0])
    sep, valid = OR.box_axes(verts, lo, hi)
    assert valid.all() and sep.shape == (13, 400, 300)
    alone = {OR.AXES[a]: int(((sep.sum(axis=0) == 1) & sep[a]).sum()) for a in range(13)}
    print(alone)
    for a in OR.AXES[3:]:
        assert alone[a] >= 8, (a, alone)
    per_box = (~sep.any(axis=0)).sum(axis=1)
    print(f"accepted per box: mean {per_box.mean():.2f}, max {per_box.max()}, empty {(per_box == 0).mean():.3f}")
    for k in (4, 16):                                                      # cut off for some queries, not for others
        assert (per_box > k).any() and (per_box < k).any() and (per_box == 0).any(), k


@pytest.mark.parametrize("shape", ("boxes", "spheres"))
def test_tri_from_and_k(shape):
    verts, lo, hi = query_set(OR.GENERATED[0])
    acc = OR.accepted_boxes(verts, lo, hi) if shape == "boxes" else OR.accepted_spheres(verts, *OR.spheres_of(lo, hi))
    full_count, full = OR.answer(acc, OR.MAX_K)
    for k in (0, 1, 4, 5):
        count, tris = OR.answer(acc, k)
        assert count.dtype == np.int32 and tris.dtype == np.int32 and tris.shape == (400, k)
        assert np.array_equal(count, full_count) and np.array_equal(tris, full[:, :k])           # the prefix property; count without k
    assert np.array_equal(full_count, acc.sum(axis=1))
    for i in (0, 7, 399):
        want = np.nonzero(acc[i])[0]
        assert full[i, :min(len(want), 16)].tolist() == want[:16].tolist() and (full[i, len(want):] == -1).all()
    # tri_from: negative stands for 0, beyond the scene considers nothing
    assert all(np.array_equal(a, b) for a, b in zip(OR.answer(acc, 4, np.full(400, -5)), OR.answer(acc, 4)))
    count, tris = OR.answer(acc, 4, np.full(400, 300))
    assert (count == 0).all() and (tris == -1).all()
    # paging with k = 2 rebuilds the full lists
    offsets, indices = OR.csr(acc)
    tf = np.zeros(400, np.int32)
    pages = [[] for _ in range(400)]
    for _ in range(acc.sum(axis=1).max() // 2 + 1):
        count, tris = OR.answer(acc, 2, tf)
        for i in range(400):
            pages[i] += tris[i][tris[i] >= 0].tolist()
        tf = np.where(tris[:, 1] >= 0, tris[:, 1] + 1, 300).astype(np.int32)
    for i in range(400):
        assert pages[i] == indices[offsets[i]:offsets[i + 1]].tolist(), i


def test_invalid_and_degenerate_boxes():
    verts, lo, hi = query_set(OR.GENERATED[0])
    acc = OR.accepted_boxes(verts, lo, hi)
    busy = np.nonzero(acc.sum(axis=1) > 0)[0][:12]
    for axis in range(3):                                                   # reversed on one axis; NaN in lo or in hi
        rl, rh = lo[busy].copy(), hi[busy].copy()
        rl[:, axis], rh[:, axis] = hi[busy, axis], lo[busy, axis]
        assert not OR.accepted_boxes(verts, rl, rh).any(), axis
        for bad_lo in (True, False):
            nl, nh = lo[busy].copy(), hi[busy].copy()
            (nl if bad_lo else nh)[:, axis] = np.nan
            assert not OR.accepted_boxes(verts, nl, nh).any(), (axis, bad_lo)
    # lo == hi on a triangle's first vertex accepts that triangle: v0 = a - a = 0 exactly, so every axis tests 0 against 0 on its
    # side (the other two vertices are a + e1, a + e2 only up to rounding, and a point box has no extent to cover that)
    a = verts[:, :3]
    assert OR.accepted_boxes(verts, a, a)[np.arange(len(a)), np.arange(len(a))].all()
    # a box around the whole scene: every triangle, the first k indices
    count, tris = OR.answer(OR.accepted_boxes(verts, [[-9, -9, -9]], [[9, 9, 9]]), 16)
    assert count.tolist() == [300] and tris[0].tolist() == list(range(16))


def test_grid_mesh_is_a_fixed_table():
    verts, _ = CR.grid_mesh()
    lo, hi = OR.grid_boxes()
    acc = OR.accepted_boxes(verts, lo, hi)
    assert np.array_equal(acc, OR.grid_expected(lo, hi))
    assert acc.sum(axis=1).tolist() == [7, 16, 38, 70, 7, 0, 4608, 22]


def test_degenerate_mix_keeps_what_truly_overlaps():
    verts, pts = CR.degenerate_mix()
    rng = np.random.default_rng(8)
    half = rng.uniform(0.005, 0.1, (len(pts), 3))
    lo, hi = (pts - half).astype(F32), (pts + half).astype(F32)
    acc = OR.accepted_boxes(verts, lo, hi)
    gap = OR.sat_gap64(verts, lo, hi)
    assert acc[gap < -GAP].all()
    degenerate = np.zeros(len(verts), bool); degenerate[::4] = True
    assert acc[:, degenerate].sum() >= 50                                  # degenerate triangles are found
    # (they can also be accepted while apart: with zero axes skipped, 13 axes do not separate every segment from every box)
    assert (acc == (gap <= 0))[:, ~degenerate][(np.abs(gap) > GAP)[:, ~degenerate]].all()


@pytest.mark.parametrize("case", ("random16", "random300"))
def test_sphere_list_holds_the_closest_point(case):
    arrays, _ = RC.scene(case)
    pts = RC.rays_in_box(arrays, 400, 5)[0]
    free = CR.mirror(arrays, pts)
    r = np.random.default_rng(11).uniform(0.0, 2.0 * float(np.median(free[1])), len(pts)).astype(F32)
    tri = CR.mirror(arrays, pts, r)[0]
    acc = OR.accepted_spheres(arrays["verts"], pts, r)
    count, _ = OR.answer(acc, 0)
    assert np.array_equal(count > 0, tri >= 0) and 0.15 <= (tri >= 0).mean() <= 0.85
    hit = tri >= 0
    assert acc[np.nonzero(hit)[0], tri[hit]].all()
    for bad in (np.nan, 0.0, -0.0, -1.0, -np.inf):
        assert not OR.accepted_spheres(arrays["verts"], pts[:20], np.full(20, bad, F32)).any(), bad
    assert OR.accepted_spheres(arrays["verts"], pts[:20], np.full(20, np.inf, F32)).all()


class FakeContext:
    """overlap_boxes / overlap_spheres / contains_points fed from an accepted matrix by hand"""

    def __init__(self, acc, inside=None):
        self.acc, self.inside, self.calls, self.row_of = acc, inside, 0, None

    def _rows(self, a):
        return np.array([self.row_of[tuple(x)] for x in np.asarray(a).tolist()], int)

    def overlap_boxes(self, lo, hi, k=0, tri_from=None):
        self.calls += 1
        assert lo.dtype == F32 and hi.dtype == F32 and (tri_from is None or tri_from.dtype == np.int32)
        rows = self._rows(lo) if self.row_of else np.arange(len(lo))
        return OR.answer(self.acc[rows], k, tri_from)

    overlap_spheres = overlap_boxes

    def contains_points(self, points):
        return self.inside


def test_all_in_paging_on_hand_fed_arrays():
    from pbrpathtracer_amd import overlap
    rng = np.random.default_rng(3)
    acc = rng.uniform(size=(9, 100)) < np.array([0, 0.05, 0.16, 0.17, 0.4, 1.0, 0.33, 0.01, 0.16])[:, None]
    acc[2] = False; acc[2, :16] = True                                      # exactly one full page
    acc[8] = False; acc[8, 83:] = True                                      # 17: one index on the second page, the last triangle
    lo = np.arange(27, dtype=F32).reshape(9, 3)
    fake = FakeContext(acc); fake.row_of = {tuple(x): i for i, x in enumerate(lo.tolist())}
    offsets, indices = overlap.all_in_boxes(fake, lo, lo + 1)
    want = OR.csr(acc)
    assert offsets.dtype == np.int64 and indices.dtype == np.int32
    assert np.array_equal(offsets, want[0]) and np.array_equal(indices, want[1])
    assert fake.calls == 7                                                  # ceil(100 / 16) pages for the full row
    fake.calls = 0
    offsets, indices = overlap.all_in_spheres(fake, lo, np.ones(9, F32))
    assert np.array_equal(offsets, want[0]) and np.array_equal(indices, want[1])
    none = FakeContext(np.zeros((0, 100), bool))
    offsets, indices = overlap.all_in_boxes(none, np.zeros((0, 3), F32), np.zeros((0, 3), F32))
    assert offsets.tolist() == [0] and len(indices) == 0


def test_voxel_occupancy_arithmetic_and_layout():
    from pbrpathtracer_amd import overlap
    origin, spacing = np.array([1.0, 2.0, 3.0], F32), np.array([0.5, 0.25, 2.0], F32)
    lo, hi, centres = overlap.voxel_boxes(origin, spacing, (4, 3, 2))
    assert lo.dtype == F32 and lo.shape == (24, 3)
    # x fastest: voxel (ix, iy, iz) at (iz * 3 + iy) * 4 + ix
    at = (1 * 3 + 2) * 4 + 3
    assert centres[at].tolist() == [2.5, 2.5, 5.0] and lo[at].tolist() == [2.25, 2.375, 4.0] and hi[at].tolist() == [2.75, 2.625, 6.0]
    acc = np.zeros((24, 5), bool); acc[at, 2] = True; acc[0, 0] = True
    inside = np.zeros(24, np.uint8); inside[5] = 1
    occ = overlap.voxel_occupancy(FakeContext(acc, inside), origin, spacing, (4, 3, 2))
    assert occ.dtype == bool and occ.shape == (2, 3, 4) and occ.sum() == 2 and occ[1, 2, 3] and occ[0, 0, 0]
    solid = overlap.voxel_occupancy(FakeContext(acc, inside), origin, spacing, (4, 3, 2), solid=True)
    assert solid.sum() == 3 and solid[0, 1, 1] and solid[1, 2, 3]
