#!/usr/bin/env python3
"""Measures overlap queries (ptk_overlap_boxes, ptk_overlap_spheres) - not a test, bench.py is untouched.  One
process per library, one JSON line each, medians of REPS runs after a warm-up; kernel times are HIP-event times
(ptk_last_overlap_ms), the work per query comes from the counting variant of the kernel (ptk_overlap_stats).

  per scene       the configs named by --configs (C1: the Cornell box, C4: 70 k triangles, C5: the 1 M-triangle scene of
                  BASELINE.md): N_QUERIES queries centred uniformly in the vertex bounds grown by 10 % per side, with half extent /
                  radius = EXTENT_SHARE x the scene's extent
  per shape       count only (k = 0) and k = 16: kernel ms and queries per second; interior nodes fetched, triangle records tested
                  and triangles accepted per query; for boxes the share of tested records the three box axes did not separate
  against         closest_kernel (ptk_closest_points) with max_dist = the same radius on the same centres: its kernel ms, and
                  each overlap time as a ratio to it - a description, not a gate

    python tools/overlap_timing.py [--configs C1,C4,C5] [--queries N] [--libs libptk.so,libptk_vote.so]

--libs runs the measurement once per library, each in a process of its own, one after the other: the two arms of an experiment
in one GPU visit (a library other than libptk.so is one built with make OUT=../libptk_NAME.so BUILD=build_NAME EXTRA=...)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5
N_QUERIES = 1 << 20
EXTENT_SHARE = 0.02


def queries_in_box(verts, n, seed):
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    pad = 0.1 * (hi - lo)
    extent = float((hi - lo).max())
    c = rng.uniform(lo - pad, hi + pad, (n, 3))
    r = EXTENT_SHARE * extent
    return (np.ascontiguousarray(c - r, np.float32), np.ascontiguousarray(c + r, np.float32), np.ascontiguousarray(c, np.float32),
            np.full(n, r, np.float32), extent)


def measure(c, arrays, n):
    import torch
    from pbrpathtracer_amd import ptk
    lo, hi, centers, radius, extent = queries_in_box(arrays["verts"], n, 5)
    dev = torch.device("cuda", c.device_ordinal())
    d = {k: torch.from_numpy(v).to(dev) for k, v in dict(lo=lo, hi=hi, centers=centers, radius=radius).items()}
    torch.cuda.synchronize()
    out = {"triangles": len(arrays["verts"]), "queries": n, "half_extent": EXTENT_SHARE * extent,
           "built_on_device": c.upload_timing()["built_on_device"], "bvh_layout": list(c.bvh_layout())}
    ms = []
    for _ in range(REPS + 1):
        c.closest_points(d["centers"], d["radius"])
        ms.append(c.last_closest_ms())
    closest = float(np.median(ms[1:]))
    nodes, tris = c.closest_stats(d["centers"], d["radius"])
    out["closest"] = {"kernel_ms": round(closest, 4), "runs_ms": [round(x, 4) for x in ms[1:]],
                      "node_visits_per_query": round(nodes / n, 3), "tri_tests_per_query": round(tris / n, 3)}
    for shape, fn, a, b, code in (("boxes", c.overlap_boxes, d["lo"], d["hi"], ptk.OVERLAP_BOX),
                                  ("spheres", c.overlap_spheres, d["centers"], d["radius"], ptk.OVERLAP_SPHERE)):
        nodes, tris, accepted, past = c.overlap_stats(code, a, b)
        res = {"node_visits_per_query": round(nodes / n, 3), "tri_tests_per_query": round(tris / n, 3), "mean_count": round(accepted / n, 3)}
        if shape == "boxes":
            res["past_box_axes_share"] = round(past / max(tris, 1), 4)
            res["accepted_share_of_tested"] = round(accepted / max(tris, 1), 4)
        for k in (0, 16):
            ms = []
            for _ in range(REPS + 1):
                fn(a, b, k)
                ms.append(c.last_overlap_ms())
            t = float(np.median(ms[1:]))
            res[f"k{k}"] = {"kernel_ms": round(t, 4), "runs_ms": [round(x, 4) for x in ms[1:]], "queries_per_s": round(n / (t * 1e-3)),
                            "ratio_to_closest": round(t / closest, 3)}
        out[shape] = res
    return out


def run(configs, n):
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    out = {"library": os.path.basename(ptk.LIB_PATH)}
    for cfg in configs:
        tmp = tempfile.mkdtemp(prefix="overlap_")
        pts_file, _, _ = S.build_config(cfg, tmp)
        pt = PathTracer(0)
        pt.LoadSceneFile(pts_file)
        arrays = pt.StagedScene()
        pt.closest_points(np.zeros((1, 3), np.float32))          # (the scene is on the GPU from here on)
        out[cfg] = measure(pt.context(), arrays, n)
        pt.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="C1,C4,C5")
    ap.add_argument("--queries", type=int, default=N_QUERIES)
    ap.add_argument("--libs", default=None, help="comma-separated library file names beside libptk.so: one child process each")
    ap.add_argument("--timeout", type=float, default=480.0, help="--libs: seconds a child may take")
    a = ap.parse_args()
    if a.libs is None:
        return run([x for x in a.configs.split(",") if x], a.queries)
    pkg = os.path.join(ROOT, "pbrpathtracer_amd")
    for lib in a.libs.split(","):
        env = dict(os.environ)
        if lib != "libptk.so":
            env.update(PTK_DEV_TOOLS="1", PTK_LIB_PATH=os.path.join(pkg, lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--configs", a.configs, "--queries", str(a.queries)], env=env,
                           timeout=a.timeout)
        if r.returncode != 0:                                     # nothing more is started behind a failed arm
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
