#!/usr/bin/env python3
"""Measures irradiance probe baking (ptk_bake_probes) on C4 - not a test, bench.py is untouched.  One process, one
JSON line, kernel times from HIP events (ptk_last_probes_ms, ptk_last_rays_ms), medians of REPS runs after a warm-up: a grid of
32 x 32 x 32 probes over the scene's vertex bounds, 256 directions of probes.fibonacci_dirs, 4 spp, depth 8.

  raygen_ms, trace_ms, project_ms   the bake's three stages; streaming_share = (raygen + project) / trace
  --dump-rays DIR    also writes the expanded rays (origins, dirs; ray p * D + j) to DIR/C4_rays.npz
  --rays-only DIR    instead of baking, traces those rays through ptk_trace_rays_device (e.g. with the parent commit's library,
                     PTK_LIB_PATH) and prints ptk_last_rays_ms' trace + fold for the identical ray set: bake trace_ms / that sum is
                     the trace-time ratio

    python tools/probes_timing.py [--dump-rays DIR | --rays-only DIR]"""
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
DIMS, DIRS, SPP, DEPTH, SEED = (32, 32, 32), 256, 4, 8, 7


def med(xs):
    return float(np.median(xs))


def measure_bake(c, t_pos, t_dirs, weight):
    runs = []
    for _ in range(REPS + 1):
        c.bake_probes(t_pos, t_dirs, DEPTH, 0, SPP, SEED, weight, want_radiance=False)
        runs.append(c.last_probes_ms())
    out = {k: round(med([r[k] for r in runs[1:]]), 4) for k in runs[0]}
    out["trace_runs_ms"] = [round(r["trace_ms"], 4) for r in runs[1:]]
    out["streaming_share"] = round((out["raygen_ms"] + out["project_ms"]) / out["trace_ms"], 4)
    return out


def measure_rays_only(c, path):
    z = np.load(path)
    ro, rd = torch.from_numpy(z["origins"]).cuda(), torch.from_numpy(z["dirs"]).cuda()
    torch.cuda.synchronize()
    tr = []
    for _ in range(REPS + 1):
        c.trace_rays(ro, rd, DEPTH, 0, SPP, SEED)
        tr.append(sum(c.last_rays_ms()))
    return {"rays": len(z["origins"]), "trace_ms": round(med(tr[1:]), 4), "runs_ms": [round(x, 4) for x in tr[1:]]}


def main():
    args = sys.argv[1:]
    dump = args[args.index("--dump-rays") + 1] if "--dump-rays" in args else None
    rays_only = args[args.index("--rays-only") + 1] if "--rays-only" in args else None
    tmp = tempfile.mkdtemp(prefix="probes_")
    out = {"dims": DIMS, "dirs": DIRS, "spp": SPP, "depth": DEPTH}
    config = "C4"
    pts, _, _ = S.build_config(config, tmp, width=64, height=64, depth=DEPTH)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    pt.RenderFrames(1)                  # BuildBVH's upload; the frame itself is not used
    c = pt.context()
    if rays_only:
        out[config] = measure_rays_only(c, os.path.join(rays_only, f"{config}_rays.npz"))
    else:
        from pbrpathtracer_amd.probes import fibonacci_dirs, grid_over_bounds, grid_positions, sh_weight
        v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
        origin, spacing = grid_over_bounds(v.min(axis=0), v.max(axis=0), DIMS)
        pos, dirs = grid_positions(DIMS, origin, spacing), fibonacci_dirs(DIRS)
        t_pos, t_dirs = torch.from_numpy(pos).cuda(), torch.from_numpy(dirs).cuda()
        torch.cuda.synchronize()
        out[config] = dict(measure_bake(c, t_pos, t_dirs, sh_weight(DIRS, SPP)), triangles=pt.GetTriangleCount(), rays=len(pos) * DIRS)
        if dump:
            os.makedirs(dump, exist_ok=True)
            np.savez(os.path.join(dump, f"{config}_rays.npz"), origins=np.repeat(pos, DIRS, axis=0), dirs=np.tile(dirs, (len(pos), 1)))
    pt.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
