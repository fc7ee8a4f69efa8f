#!/usr/bin/env python3
"""Measures probe visibility (ptk_bake_probe_visibility, ptk_probes_irradiance_visible) on C4 - not a test, bench.py
is untouched.  One process, one JSON line, medians of REPS runs after a warm-up:

  raygen_ms, hits_ms, moments_ms   the bake's three stages (HIP events, ptk_last_probe_visibility_ms): a grid of 16 x 16 x 16 probes
                                   over the scene's vertex bounds, 256 directions of probes.fibonacci_dirs, res 8,
                                   max_dist = probes.default_max_dist
  lookup                           2^20 query points in the grid's box with random unit normals through probe_irradiance_kernel
                                   (plain) and probe_irradiance_visible_kernel (visible, with the baked moments, bias 0.05): HIP
                                   events around one device-entry call each, in ms and queries per second

    python tools/probe_visibility_timing.py"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (one ROCm runtime in the process, as tests/conftest.py)

from pbrpathtracer_amd import scenes as S  # noqa: E402
from pbrpathtracer_amd.pathtracer import PathTracer  # noqa: E402

REPS = 5
DIMS, DIRS, RES, DEPTH, SEED, POINTS = (16, 16, 16), 256, 8, 8, 7, 1 << 20


def med(xs):
    return float(np.median(xs))


def measure_bake(c, t_pos, t_dirs, max_dist):
    runs = []
    for _ in range(REPS + 1):
        _, moments = c.bake_probe_visibility(t_pos, t_dirs, RES, max_dist, 0, SEED, want_depth=False)
        runs.append(c.last_probe_visibility_ms())
    out = {k: round(med([r[k] for r in runs[1:]]), 4) for k in runs[0]}
    out["hits_runs_ms"] = [round(r["hits_ms"], 4) for r in runs[1:]]
    return out, moments


def timed(stream, call):
    """ms of REPS calls (after a warm-up) between two events on the context's stream"""
    ms = []
    for _ in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); call(); b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms[1:]


def measure_lookup(c, stream, origin, spacing, coefs, moments):
    rng = np.random.default_rng(3)
    ext = np.asarray(spacing, np.float64) * (np.asarray(DIMS) - 1)
    pts = rng.uniform(np.asarray(origin, np.float64), np.asarray(origin, np.float64) + ext, (POINTS, 3)).astype(np.float32)
    nrm = rng.normal(0.0, 1.0, (POINTS, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    t_pts, t_nrm = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
    c.set_stream(stream.cuda_stream)        # (from here to the context's end its work runs on this stream)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):             # (the output tensors are allocated on the stream that writes them)
        plain = timed(stream, lambda: c.probes_irradiance(DIMS, origin, spacing, coefs, t_pts, t_nrm))
        visible = timed(stream, lambda: c.probes_irradiance_visible(DIMS, origin, spacing, coefs, RES, moments, t_pts, t_nrm, 0.05))
    stream.synchronize()
    return {"points": POINTS,
            "plain_ms": round(med(plain), 4), "plain_mqps": round(POINTS / med(plain) / 1e3, 1), "plain_runs_ms": [round(x, 4) for x in plain],
            "visible_ms": round(med(visible), 4), "visible_mqps": round(POINTS / med(visible) / 1e3, 1),
            "visible_runs_ms": [round(x, 4) for x in visible]}


def main():
    from pbrpathtracer_amd.probes import default_max_dist, fibonacci_dirs, grid_over_bounds, grid_positions, sh_weight
    tmp = tempfile.mkdtemp(prefix="probe_vis_")
    out = {"dims": DIMS, "dirs": DIRS, "res": RES}
    config = "C4"
    pts, _, _ = S.build_config(config, tmp, width=64, height=64, depth=DEPTH)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    pt.RenderFrames(1)                  # BuildBVH's upload; the frame itself is not used
    c = pt.context()
    v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
    origin, spacing = grid_over_bounds(v.min(axis=0), v.max(axis=0), DIMS)
    pos, dirs = grid_positions(DIMS, origin, spacing), fibonacci_dirs(DIRS)
    t_pos, t_dirs = torch.from_numpy(pos).cuda(), torch.from_numpy(dirs).cuda()
    torch.cuda.synchronize()
    max_dist = default_max_dist(spacing)
    bake, moments = measure_bake(c, t_pos, t_dirs, max_dist)
    _, coefs = c.bake_probes(t_pos, t_dirs, DEPTH, 0, 1, SEED, sh_weight(DIRS, 1), want_radiance=False)
    c.synchronize()
    stream = torch.cuda.Stream()
    out[config] = dict(bake, triangles=pt.GetTriangleCount(), rays=len(pos) * DIRS, max_dist=round(max_dist, 4),
                       lookup=measure_lookup(c, stream, origin, spacing, coefs, moments))
    pt.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
