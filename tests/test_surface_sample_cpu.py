"""Surface sampling without a device (include/ptk.h ptk_sample_surface): the numpy restatement of the rule
(tests/surface_sample_rule.py) is what it claims - it draws triangles in proportion to their float64 areas, its points lie on their
triangles, its quantiser has the edges the header states, and a sample is a function of (seed, key_base + j, sample) alone - and the
library exports and declares what the feature adds.  tests/test_gpu_surface_sample.py holds the kernels to this restatement bit for
bit."""
import math
import os
import re

import numpy as np
import pytest

import surface_sample_rule as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SEED = 12345 | 7 << 32
N = 1 << 18
BOUND = 255 + 6 * math.sqrt(2 * 255)            # six standard deviations of chi-square with 255 degrees of freedom

NEW_PTK = ["ptk_surface_weights", "ptk_surface_weights_device", "ptk_sample_surface", "ptk_sample_surface_device", "ptk_surface_info",
           "ptk_last_surface_ms", "ptk_probe_surface_table", "ptk_probe_scan_u64"]
NEW_PTH = ["pth_sample_surface", "pth_set_surface_weights", "pth_surface_info"]


def test_symbols_are_exported_and_declared():
    from pbrpathtracer_amd import ptk, pathtracer, surface
    L = ptk.load()
    head = open(os.path.join(ROOT, "include", "ptk.h")).read()
    text = head + open(os.path.join(ROOT, "include", "ptk_host.h")).read()
    declared = set(re.findall(r"\b(p(?:tk|th)_[a-z0-9_]+)\s*\(", text))
    for name in NEW_PTK + NEW_PTH:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in ptk.SYMBOLS + pathtracer.HOST_SYMBOLS, name
    assert int(re.search(r"#define PTK_SURFACE_SCAN_ITEMS (\d+)", head).group(1)) == ptk.SURFACE_SCAN_ITEMS
    for cls, names in ((ptk.Context, ("set_surface_weights", "sample_surface", "surface_info", "last_surface_ms")),
                       (pathtracer.PathTracer, ("set_surface_weights", "sample_surface", "surface_info", "SampleSurface", "SetSurfaceWeights"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("material_weights", "emissive_weights", "bake_points"):
        assert callable(getattr(surface, name)), name
    cls = open(os.path.join(ROOT, "include", "pathtracer.h")).read()
    assert "bool SampleSurface(" in cls and "bool SetSurfaceWeights(" in cls
    assert "NEVER DRAWN" in head and "2^-36" in head                      # the header states what the quantiser drops


@pytest.fixture(scope="module")
def torus():
    v = SR.stretched_torus()
    assert v.shape == (256, 9) and v.dtype == F32
    d = v.astype(np.float64)
    a64 = 0.5 * np.linalg.norm(np.cross(d[:, 3:6] - d[:, 0:3], d[:, 6:9] - d[:, 0:3]), axis=1)
    assert 4.0 < a64.max() / a64.min() < 6.5                              # an area ratio of about 5
    return v, a64


@pytest.fixture(scope="module")
def draws(torus):
    """the rule's samples of the two runs, computed once: (weights, outputs)"""
    v, _ = torus
    from pbrpathtracer_amd import ptk, surface
    mats = np.zeros(2, ptk.MATERIAL_DTYPE)
    mats["emissive"][1] = (1.0, 0.5, 0.25); mats["emissive_intensity"] = (3.0, 2.0)    # material 0 is black whatever its intensity
    ids = (np.arange(len(v)) % 2).astype(np.int32)                        # half the triangles emit
    w = surface.emissive_weights(mats, ids)
    assert w.dtype == F32 and (w[ids == 0] == 0).all() and (w[ids == 1] > 0).all() and len(np.unique(w[ids == 1])) == 1
    nrm = np.zeros((len(v), 3), F32); nrm[:, 2] = 1
    return {"area": (None, SR.sample(v, N, SEED, 0, 0, normals=nrm, material=ids)),
            "emissive": (w, SR.sample(v, N, SEED, 0, 0, weights=w, normals=nrm, material=ids))}


def _chi2(tri, expected):
    counts = np.bincount(tri, minlength=len(expected)).astype(np.float64)
    keep = expected > 0
    assert (counts[~keep] == 0).all()
    return float(((counts[keep] - expected[keep]) ** 2 / expected[keep]).sum()), int(keep.sum())


def test_triangles_are_drawn_in_proportion_to_area(torus, draws):
    """Pearson's chi-square of the per-triangle counts against n * area64_i / sum(area64).  Measured with the rule as written: the
    statistic is 232.55, the smallest expected count 356."""
    _, a64 = torus
    expected = N * a64 / a64.sum()
    assert expected.min() >= 5, expected.min()                             # the precondition of the statistic
    chi2, cells = _chi2(draws["area"][1][0], expected)
    print(f"chi2 {chi2:.2f} over {cells} triangles, smallest expected count {expected.min():.0f}, bound {BOUND:.2f}")
    assert cells == 256 and chi2 <= BOUND, chi2


def test_zero_weights_are_never_drawn_and_the_rest_keeps_its_proportions(torus, draws):
    """emissive_weights-style weights that zero half the triangles: the same bound, over the 128 that are left (the bound of 255
    degrees of freedom is the wider one for 127)"""
    _, a64 = torus
    w, out = draws["emissive"]
    tri = out[0]
    assert (w[tri] > 0).all() and (out[4] == 1).all()
    mass = a64 * (w > 0)
    expected = N * mass / mass.sum()
    assert expected[w > 0].min() >= 5
    chi2, cells = _chi2(tri, expected)
    print(f"chi2 {chi2:.2f} over {cells} triangles, bound {BOUND:.2f}")
    assert cells == 128 and chi2 <= BOUND, chi2


@pytest.mark.parametrize("run", ["area", "emissive"])
def test_points_lie_on_their_triangles(torus, draws, run):
    """u >= 0, v >= 0, u + v <= 1 for every sample (measured: no violation, largest u + v 0.99999964), and the position, in float64,
    lies within 1e-6 x the triangle's longest edge of its plane and inside it"""
    v, _ = torus
    tri, bary, pos, _, _ = draws[run][1]
    u, w = bary[:, 0], bary[:, 1]
    assert bary.dtype == F32 and (u >= 0).all() and (w >= 0).all()
    s = u.astype(np.float64) + w.astype(np.float64)
    print(f"{run}: largest u + v {s.max():.8f}")
    assert (u + w <= F32(1)).all() and (s <= 1).all()
    t = v.reshape(-1, 3, 3).astype(np.float64)[tri]
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    longest = np.maximum(np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)), np.linalg.norm(t[:, 2] - t[:, 1], axis=1))
    n = np.cross(e1, e2); n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = pos.astype(np.float64) - t[:, 0]
    tol = 1e-6 * longest
    assert (np.abs((d * n).sum(axis=1)) <= tol).all()
    # inside: its barycentrics in float64, from the position alone, are within the same distance of [0, 1]
    d11, d12, d22 = (e1 * e1).sum(axis=1), (e1 * e2).sum(axis=1), (e2 * e2).sum(axis=1)
    b1, b2 = (d * e1).sum(axis=1), (d * e2).sum(axis=1)
    det = d11 * d22 - d12 * d12
    p, q = (d22 * b1 - d12 * b2) / det, (d11 * b2 - d12 * b1) / det
    slack = tol / np.sqrt(det / np.maximum(d11, d22))                      # a distance of tol across the nearest edge, in barycentric units
    assert (p >= -slack).all() and (q >= -slack).all() and (p + q <= 1 + slack).all()
    # ... and they are the sample's own (u, v): five float32 roundings per component - three products, two sums, none of a value
    # larger than the triangle's largest coordinate - move the point by at most 2.5 ulp of that per component, and the weights' own
    # four roundings (w0 + w1 + w2 is 1 within 4 x 2^-25) by one more: 4 x 2^-23 x it; a barycentric coordinate changes by at most
    # that distance over the triangle's smallest altitude, 2 area / longest edge
    moved = 4 * 2.0 ** -23 * np.abs(t).max(axis=(1, 2)) * math.sqrt(3)
    own = moved / (np.sqrt(det) / longest)
    assert (np.abs(p - u) <= own).all() and (np.abs(q - w) <= own).all()


def test_quantiser_edges():
    """areas 1, 2^-20, 2^-35, 2^-36, 2^-37 times the largest, the largest a power of two: q = 2^35, 2^15, 1, 0, 0 - a weight at
    2^-35 of the largest is the smallest that can be drawn; at 2^-36 and below q = 0 and the triangle never is"""
    v, factors = SR.edge_table_scene()
    a = SR.areas(v)
    assert [float(x) / float(a[0]) for x in a] == factors
    q, E = SR.quantise(a)
    assert E == -1 and [int(x) for x in q] == [1 << 35, 1 << 15, 1, 0, 0]
    incl = SR.table(v)[0]
    sums = [sum(int(x) for x in q[:i + 1]) for i in range(5)]
    assert [int(x) for x in incl] == sums and SR.info(v) == (sums[-1], -1, 3, F32(0.5))
    tri = SR.pick(incl, SEED, 0, 1 << 16, 0)[0]
    assert not np.isin(tri, [3, 4]).any() and set(np.unique(tri)) <= {0, 1, 2}
    assert (tri == 0).sum() > 65000                                       # (the q = 1 triangle may be drawn; at 2^-35 it practically never is)
    # the largest mantissa: q stays below 2^36, and the same factors give 1, 0, 0 again
    big = F32(2.0) - F32(2.0 ** -23)
    q2, E2 = SR.quantise((a * big).astype(F32))
    assert E2 == -1 and int(q2[0]) == (1 << 36) - (1 << 12) and [int(x) for x in q2[2:]] == [1, 0, 0]
    with pytest.raises(ValueError):
        SR.quantise(np.zeros(4, F32))
    with pytest.raises(ValueError):
        SR.quantise(np.array([1, np.inf], F32))
    # the high half of the product, against Python integers
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 64, 2000, dtype=np.uint64); y = rng.integers(0, 1 << 63, 2000, dtype=np.uint64)
    assert [int(h) for h in SR.mulhi64(x, y)] == [(int(p) * int(r)) >> 64 for p, r in zip(x, y)]


def test_cutting_and_streams(torus):
    v, _ = torus
    whole = SR.sample(v, 1000, SEED)
    a, b = SR.sample(v, 333, SEED), SR.sample(v, 667, SEED, key_base=333)
    for w, x, y in zip(whole, a, b):
        assert np.array_equal(w, np.concatenate([x, y]))
    for other in (dict(sample=1), dict(seed=SEED ^ 1), dict(seed=SEED ^ (1 << 32)), dict(key_base=1)):
        args = dict(seed=SEED, key_base=0, sample=0); args.update(other)
        got = SR.sample(v, 1000, **args)
        assert (got[0] != whole[0]).mean() > 0.9 and not np.array_equal(got[1], whole[1]), other
    shifted = SR.sample(v, 999, SEED, key_base=1)
    assert all(np.array_equal(s, w[1:]) for s, w in zip(shifted, whole))  # sample j depends on key_base + j only
    wrap = SR.sample(v, 4, SEED, key_base=0xfffffffe)
    assert all(np.array_equal(s[2:], w[:2]) for s, w in zip(wrap, whole))  # ... mod 2^32


def test_weight_tables():
    from pbrpathtracer_amd import surface
    ids = np.array([0, 2, 1, 2, 5], np.int32)
    assert np.array_equal(surface.material_weights(ids, 2), np.array([0, 1, 0, 1, 0], F32))
    assert np.array_equal(surface.material_weights(ids, [0, 5]), np.array([1, 0, 0, 0, 1], F32))
    p, n = np.array([[1, 2, 3]], F32), np.array([[0, 0, 1]], F32)
    o, d = surface.bake_rays(p, n, 0.1)
    assert o.dtype == F32 and np.array_equal(o, p + n * F32(0.1)) and np.array_equal(d, -n)
