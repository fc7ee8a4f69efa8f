#!/usr/bin/env python3
"""Measures crossing counts, containment and the signed distance (ptk_crossings_rays, ptk_contains_points, ptk_signed_distance;
DESIGN.md §4.24) beside the queries they are built like - not a test, bench.py is untouched.  One process, one JSON line; per
figure the median of REPS runs after a warm-up run of the same shape, with the runs themselves (their spread is the noise).  Kernel
times are HIP-event times (ptk_last_crossings_ms, ptk_last_hits_ms, ptk_last_closest_ms); the calls of a group are alternated run
by run, so that whatever else the machine does falls on all of them alike.

  per scene   the configs named by --configs (C1: the Cornell box; C4: a deep scene, 70 k triangles inside the Cornell shell; C5:
              the 1 M-triangle scene of BASELINE.md)
  rays        N rays, origins uniform in the vertex bounds grown by 10 % per side, directions uniform on the sphere:
              crossings_rays with tmax = inf, intersect_rays and occluded_rays (tmax = inf) over the same rays
  points      the same N origins as points: contains_points (the built-in 3 directions), signed_distance and closest_points
  ratios      crossings / intersect, contains / (3 x intersect) and signed_distance / closest: a walk that prunes nothing visits at
              least the nodes a closest-hit walk visits

    python tools/crossings_timing.py [--configs C1,C4] [--queries N]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 7
N_QUERIES = 1 << 20


def rays_in_box(verts, n, seed):
    """tests/ray_cases.py rays_in_box"""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    pad = 0.1 * (hi - lo)
    d = rng.normal(0.0, 1.0, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(rng.uniform(lo - pad, hi + pad, (n, 3)), np.float32), np.ascontiguousarray(d, np.float32)


def alternate(calls):
    """{name: (median ms, runs)} of the calls {name: (run, last_ms)}: one warm-up round, then REPS rounds through all of them"""
    runs = {k: [] for k in calls}
    for r in range(REPS + 1):
        for k, (run, last_ms) in calls.items():
            run()
            if r:
                runs[k].append(last_ms())
    return {k: {"kernel_ms": round(float(np.median(v)), 4), "runs_ms": [round(x, 4) for x in v]} for k, v in runs.items()}


def measure(c, arrays, n):
    import torch
    ro, rd = rays_in_box(arrays["verts"], n, 5)
    dev = torch.device("cuda", c.device_ordinal())
    d_ro, d_rd = torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev)
    d_inf = torch.full((n,), float("inf"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    out = {"triangles": len(arrays["verts"]), "queries": n, "built_on_device": c.upload_timing()["built_on_device"],
           "bvh_layout": list(c.bvh_layout())}
    keep = {}

    def call(name, fn):
        def run():
            keep[name] = fn()
        return run
    out["rays"] = alternate({
        "crossings": (call("crossings", lambda: c.crossings_rays(d_ro, d_rd, d_inf)), c.last_crossings_ms),
        "intersect": (call("intersect", lambda: c.intersect_rays(d_ro, d_rd)), c.last_hits_ms),
        "occluded": (call("occluded", lambda: c.occluded_rays(d_ro, d_rd, d_inf)), c.last_hits_ms)})
    out["points"] = alternate({
        "contains": (call("contains", lambda: c.contains_points(d_ro)), c.last_crossings_ms),
        "signed_distance": (call("signed_distance", lambda: c.signed_distance(d_ro)), c.last_crossings_ms),
        "closest": (call("closest", lambda: c.closest_points(d_ro)), c.last_closest_ms)})
    c.synchronize()
    front, back = keep["crossings"]
    out["crossings_per_ray"] = round(float((front + back).float().mean().item()), 4)
    out["inside_fraction"] = round(float(keep["contains"].float().mean().item()), 4)
    out["rays_that_cross"] = round(float((front + back > 0).float().mean().item()), 4)
    out["rays_that_hit"] = round(float((keep["intersect"][0] >= 0).float().mean().item()), 4)
    ms = lambda g, k: out[g][k]["kernel_ms"]
    out["ratios"] = {"crossings_over_intersect": round(ms("rays", "crossings") / ms("rays", "intersect"), 3),
                     "crossings_over_occluded": round(ms("rays", "crossings") / ms("rays", "occluded"), 3),
                     "contains_over_3_intersect": round(ms("points", "contains") / (3.0 * ms("rays", "intersect")), 3),
                     "signed_distance_over_closest": round(ms("points", "signed_distance") / ms("points", "closest"), 3)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="C1,C4")
    ap.add_argument("--queries", type=int, default=N_QUERIES)
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    from pbrpathtracer_amd import scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    out = {}
    for cfg in [x for x in a.configs.split(",") if x]:
        tmp = tempfile.mkdtemp(prefix="crossings_")
        pts_file, _, _ = S.build_config(cfg, tmp)
        pt = PathTracer(0)
        pt.LoadSceneFile(pts_file)
        arrays = pt.StagedScene()
        pt.closest_points(np.zeros((1, 3), np.float32))          # (the scene is on the GPU from here on)
        out[cfg] = measure(pt.context(), arrays, a.queries)
        pt.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
