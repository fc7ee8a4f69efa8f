#!/usr/bin/env python3
"""Measures ray queries (ptk_trace_rays) on C4 - not a test, bench.py is untouched.  One process, one JSON line,
kernel times from HIP events (ptk_last_rays_ms, ptk_last_kernel_ms), medians of REPS runs after a warm-up:

  coherent   the camera's own rays of the 1920 x 1080 frame (ptk_probe_primary_dirs, normalised), 8 spp, depth 8: paths per second
             of rays_kernel beside those of ptk_render's trace kernel with "primary_cache", "lens_cull" and "overlap" off, so that
             it walks every camera ray too; `ratio` = the first over the second
  wide       2^20 rays inside the scene's bounds x 4 spp       } the two regimes of the work distribution: many rays with few
  deep       4096 such rays x 1024 spp                         } samples, few rays with many
  fold_ms    rays_fold_kernel's time beside each trace_ms

    python tools/rays_timing.py [--render-only]      (--render-only: the render's trace kernel alone, e.g. of another build)"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (one ROCm runtime in the process, as tests/conftest.py)

from pbrpathtracer_amd import scenes as S  # noqa: E402
from pbrpathtracer_amd.pathtracer import PathTracer  # noqa: E402

REPS = 5
W, H, DEPTH, SEED = 1920, 1080, 8, 7


def rays_in_box(arrays, n, seed):
    """tests/ray_cases.py rays_in_box: origins uniform in the vertex bounds grown by 10 % per side, directions uniform on the sphere"""
    rng = np.random.default_rng(seed)
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    pad = 0.1 * (hi - lo)
    ro = rng.uniform(lo - pad, hi + pad, (n, 3))
    rd = rng.normal(0.0, 1.0, (n, 3))
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    return np.ascontiguousarray(ro, np.float32), np.ascontiguousarray(rd, np.float32)


def med(xs):
    return float(np.median(xs))


def measure_render(c, spp):
    for k, v in (("primary_cache", 0), ("lens_cull", 0), ("overlap", 0)):
        c.set_option(k, v)
    ms = []
    for i in range(REPS + 1):
        c.reset(); c.render(0, spp, SEED); c.synchronize()
        ms.append(c.last_kernel_ms()[0])
    t = med(ms[1:])
    return {"trace_ms": round(t, 4), "runs_ms": [round(x, 4) for x in ms[1:]], "paths_per_s": round(W * H * spp / (t * 1e-3))}


def measure_rays(c, ro, rd, spp, **kw):
    tr, fo = [], []
    for i in range(REPS + 1):
        c.trace_rays(ro, rd, DEPTH, 0, spp, SEED, **kw)
        t, f = c.last_rays_ms()
        tr.append(t); fo.append(f)
    t, f = med(tr[1:]), med(fo[1:])
    return {"rays": len(ro), "spp": spp, "trace_ms": round(t, 4), "fold_ms": round(f, 4), "runs_ms": [round(x, 4) for x in tr[1:]],
            "paths_per_s": round(len(ro) * spp / (t * 1e-3)), "fold_share": round(f / t, 4)}


def main():
    render_only = "--render-only" in sys.argv[1:]
    tmp = tempfile.mkdtemp(prefix="rays_")
    pts, scene, _ = S.build_config("C4", tmp, width=W, height=H, depth=DEPTH)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    pt.SetCameraAperture(0.0)
    pt.RenderFrames(1)
    c = pt.context()
    out = {"config": "C4", "triangles": pt.GetTriangleCount(), "frame": [W, H], "depth": DEPTH}
    if not render_only:
        arrays = pt.StagedScene()
        d = c.primary_dirs().reshape(-1, 3).astype(np.float64)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rd = np.ascontiguousarray(d, np.float32)
        ro = np.ascontiguousarray(np.broadcast_to(pt.GetCamera()[0], rd.shape), np.float32)
        out["coherent"] = measure_rays(c, ro, rd, 8)
        ro, rd = rays_in_box(arrays, 1 << 20, 5)
        out["wide"] = measure_rays(c, ro, rd, 4)
        out["deep"] = measure_rays(c, ro[:4096], rd[:4096], 1024)
        out["deep_over_wide"] = round(out["deep"]["paths_per_s"] / out["wide"]["paths_per_s"], 4)
    out["render"] = measure_render(c, 8)
    if not render_only:
        out["ratio"] = round(out["coherent"]["paths_per_s"] / out["render"]["paths_per_s"], 4)
    pt.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
