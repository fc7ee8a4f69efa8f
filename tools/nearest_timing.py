#!/usr/bin/env python3
"""Measures K-nearest triangle queries (ptk_nearest_triangles) beside the two queries they sit between - not a
test, bench.py is untouched.  One process, one JSON line; per figure the median of REPS runs after a warm-up run of the same shape,
with the runs themselves (their spread is the noise).  Kernel times are HIP-event times (ptk_last_nearest_ms, ptk_last_closest_ms,
ptk_last_overlap_ms); the calls are alternated run by run, so that whatever else the machine does falls on all of them alike.

  per scene   the configs named by --configs (C1: the Cornell box; C4: 70 k triangles inside the Cornell shell; C5: 1 M triangles)
  points      N points uniform in the vertex bounds grown by 10 % per side, no max_dist:
              nearest_triangles for K = 1, 4 and 16 and closest_points (closest_kernel); for K = 4 and 16 also overlap_spheres with
              k = 16 and the radius set to the next float above each point's K-th distance (what a caller who knew it would ask)
  work        interior nodes fetched and triangle records tested per query (ptk_nearest_stats, ptk_closest_stats, ptk_overlap_stats)
  ratios      nearest K over closest, and nearest K over overlap_spheres at the K-th distance

    python tools/nearest_timing.py [--configs C1,C4,C5] [--queries N]"""
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
KS = (1, 4, 16)


def points_in_box(verts, n, seed):
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    pad = 0.1 * (hi - lo)
    return np.ascontiguousarray(rng.uniform(lo - pad, hi + pad, (n, 3)), np.float32)


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
    from pbrpathtracer_amd import ptk
    pts = points_in_box(arrays["verts"], n, 5)
    dev = torch.device("cuda", c.device_ordinal())
    d_p = torch.from_numpy(pts).to(dev)
    torch.cuda.synchronize()
    out = {"triangles": len(arrays["verts"]), "queries": n, "built_on_device": c.upload_timing()["built_on_device"],
           "bvh_layout": list(c.bvh_layout())}
    # the radius of the overlap query that lists the same triangles: the next float above the K-th distance
    radius = {}
    for K in KS[1:]:
        dist = c.nearest_triangles(d_p, K)[2]
        c.synchronize()
        kth = dist[:, K - 1].contiguous()
        radius[K] = torch.nextafter(kth, torch.full_like(kth, float("inf"))).contiguous()
    torch.cuda.synchronize()
    calls = {f"nearest_{K}": ((lambda K=K: c.nearest_triangles(d_p, K)), c.last_nearest_ms) for K in KS}
    calls["closest"] = ((lambda: c.closest_points(d_p)), c.last_closest_ms)
    for K in KS[1:]:
        calls[f"overlap_at_{K}th"] = ((lambda K=K: c.overlap_spheres(d_p, radius[K], 16)), c.last_overlap_ms)
    out["points"] = alternate(calls)
    c.synchronize()
    per = lambda pair: [round(x / n, 3) for x in pair]
    out["work_per_query"] = {"closest": per(c.closest_stats(d_p))}
    for K in KS:
        out["work_per_query"][f"nearest_{K}"] = per(c.nearest_stats(d_p, K))
    for K in KS[1:]:
        out["work_per_query"][f"overlap_at_{K}th"] = per(c.overlap_stats(ptk.OVERLAP_SPHERE, d_p, radius[K])[:3])
    ms = lambda k: out["points"][k]["kernel_ms"]
    out["ratios"] = {f"nearest_{K}_over_closest": round(ms(f"nearest_{K}") / ms("closest"), 3) for K in KS}
    for K in KS[1:]:
        out["ratios"][f"nearest_{K}_over_overlap_at_{K}th"] = round(ms(f"nearest_{K}") / ms(f"overlap_at_{K}th"), 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="C1,C4,C5")
    ap.add_argument("--queries", type=int, default=N_QUERIES)
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    from pbrpathtracer_amd import scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    out = {}
    for cfg in [x for x in a.configs.split(",") if x]:
        tmp = tempfile.mkdtemp(prefix="nearest_")
        print(f"{cfg}: building the scene", file=sys.stderr, flush=True)
        pts_file, _, _ = S.build_config(cfg, tmp)
        pt = PathTracer(0)
        pt.LoadSceneFile(pts_file)
        arrays = pt.StagedScene()
        pt.nearest_triangles(np.zeros((1, 3), np.float32), 1)                 # (the scene is on the GPU from here on)
        print(f"{cfg}: measuring", file=sys.stderr, flush=True)
        out[cfg] = measure(pt.context(), arrays, a.queries)
        pt.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
