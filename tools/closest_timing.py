#!/usr/bin/env python3
"""Measures closest-point queries (ptk_closest_points) - not a test, bench.py is untouched.  One process, one JSON
line, medians of REPS runs after a warm-up; kernel times are HIP-event times (ptk_last_closest_ms), the work per query comes from
the counting variant of the kernel (ptk_closest_stats).

  per scene       random6000 (tests/test_gpu_random_scenes.py random_scene(16, 6000)) and the configs named by --configs (C5: the
                  1 M-triangle scene of BASELINE.md): N_POINTS points uniform in the vertex bounds grown by 10 % per side
  no radius       kernel ms, points per second, interior nodes fetched and triangle records tested per query
  radius          the same with max_dist = RADIUS_OF_EXTENT x the scene's extent for every point, and the share of points that
                  find surface within it

    python tools/closest_timing.py [--configs C5] [--points N]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5
N_POINTS = 1 << 20
RADIUS_OF_EXTENT = 0.02


def points_in_box(verts, n, seed):
    """tests/ray_cases.py rays_in_box's origins: uniform in the vertex bounds grown by 10 % per side"""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    pad = 0.1 * (hi - lo)
    return np.ascontiguousarray(rng.uniform(lo - pad, hi + pad, (n, 3)), np.float32), float((hi - lo).max())


def measure(c, arrays, n_points):
    import torch
    pts, extent = points_in_box(arrays["verts"], n_points, 5)
    dev = torch.device("cuda", c.device_ordinal())
    d_pts = torch.from_numpy(pts).to(dev)
    d_md = torch.full((n_points,), RADIUS_OF_EXTENT * extent, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    out = {"triangles": len(arrays["verts"]), "points": n_points, "built_on_device": c.upload_timing()["built_on_device"],
           "bvh_layout": list(c.bvh_layout())}
    for name, md in (("no_radius", None), ("radius", d_md)):
        ms = []
        for _ in range(REPS + 1):
            res = c.closest_points(d_pts, md)
            ms.append(c.last_closest_ms())
        k = float(np.median(ms[1:]))
        nodes, tris = c.closest_stats(d_pts, md)
        out[name] = {"kernel_ms": round(k, 4), "runs_ms": [round(x, 4) for x in ms[1:]], "points_per_s": round(n_points / (k * 1e-3)),
                     "node_visits_per_query": round(nodes / n_points, 3), "tri_tests_per_query": round(tris / n_points, 3),
                     "found_fraction": round(float((res[0] >= 0).float().mean().item()), 4)}
    out["radius"]["max_dist"] = RADIUS_OF_EXTENT * extent
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="C5")
    ap.add_argument("--points", type=int, default=N_POINTS)
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    out = {}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_random_scenes import random_scene
    arrays, _ = random_scene(16, 6000, True)
    c = ptk.Context(0)
    c.upload_scene(arrays)
    out["random6000"] = measure(c, arrays, a.points)
    c.close()
    for cfg in [x for x in a.configs.split(",") if x]:
        tmp = tempfile.mkdtemp(prefix="closest_")
        pts_file, _, _ = S.build_config(cfg, tmp)
        pt = PathTracer(0)
        pt.LoadSceneFile(pts_file)
        arrays = pt.StagedScene()
        pt.closest_points(np.zeros((1, 3), np.float32))          # (the scene is on the GPU from here on)
        out[cfg] = measure(pt.context(), arrays, a.points)
        pt.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
