#!/usr/bin/env python3
"""Measures the adaptive lightmap bake (ptk_bake_lightmap_adaptive) on C4 - not a test, bench.py is untouched.  One
process, one JSON line, medians of REPS runs after a warm-up: lightmap.grid_atlas at 1024 x 1024, depth 8, offset = 1e-3 of the
scene extent, max_spp 256, rounds of 8 samples, 16 before the first test, thresholds 0.05 and 0.1; every call through the device
entries, wall times from a host clock around calls that end in a stream synchronise.

  plain_max_ms          (b) ptk_bake_lightmap at spp = max_spp
  per threshold:
    adaptive_ms         (a) the adaptive bake, wall; mean_count, rounds, active texels left, the counts' histogram
    plain_floor_ms      (c) ptk_bake_lightmap at spp = round(mean count): what the same samples cost without any round
    loop_ms, trace_ms, other_ms, host_ms   ptk_last_rays_adaptive_ms: the round loop's wall time, its rays_keyed_kernel launches, its
                        other kernels (gather, fold, converge, compaction), and loop - trace - other: the host's share (the wait per
                        round, launches); outside_share = (d) = (loop - trace) / loop

    python tools/rays_adaptive_timing.py [CONFIG (default C4)]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (one ROCm runtime in the process, as tests/conftest.py)

from pbrpathtracer_amd import scenes as S  # noqa: E402
from pbrpathtracer_amd.lightmap import grid_atlas  # noqa: E402
from pbrpathtracer_amd.pathtracer import PathTracer  # noqa: E402

REPS = 5
SIZE, DEPTH, SEED, MIN_SPP, STEP, MAX_SPP = 1024, 8, 7, 16, 8, 256
THRESHOLDS = (0.05, 0.1)


def med(xs):
    return round(float(np.median(xs)), 3)


def wall(c, fn):
    c.synchronize()
    t0 = time.perf_counter()
    r = fn()
    c.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def plain(c, uvs, offset, spp):
    return med([wall(c, lambda: c.bake_lightmap(SIZE, SIZE, offset, DEPTH, 0, spp, SEED, uvs=uvs, device=True))[0] for _ in range(REPS + 1)][1:])


def main():
    config = sys.argv[1] if len(sys.argv) > 1 else "C4"
    tmp = tempfile.mkdtemp(prefix="radapt_")
    pts, _, _ = S.build_config(config, tmp, width=64, height=64, depth=DEPTH)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    pt.RenderFrames(1)                  # BuildBVH's upload; the frame itself is not used
    c = pt.context()
    v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
    offset = float(np.float32(1e-3 * (v.max(axis=0) - v.min(axis=0)).max()))
    uvs = torch.from_numpy(grid_atlas(pt.GetTriangleCount(), SIZE, SIZE)).cuda()
    torch.cuda.synchronize()
    out = {"config": config, "triangles": pt.GetTriangleCount(), "size": SIZE, "depth": DEPTH, "min_spp": MIN_SPP, "step": STEP,
           "max_spp": MAX_SPP, "plain_max_ms": plain(c, uvs, offset, MAX_SPP)}
    for thr in THRESHOLDS:
        runs, hooks = [], []
        for _ in range(REPS + 1):
            ms, (_, counts, owner, res) = wall(c, lambda: c.bake_lightmap_adaptive(SIZE, SIZE, offset, DEPTH, thr, MIN_SPP, STEP, MAX_SPP, SEED,
                                                                                  uvs=uvs, device=True))
            runs.append(ms); hooks.append(c.last_rays_adaptive_ms())
        covered = int((owner >= 0).sum().item())
        mean = res["ray_samples"] / max(covered, 1)
        n = counts.cpu().numpy().view(np.uint32)[owner.cpu().numpy() >= 0]
        loop, trace, other = (med([h[k] for h in hooks[1:]]) for k in ("total_ms", "trace_ms", "other_ms"))
        out[f"threshold_{thr}"] = {
            "adaptive_ms": med(runs[1:]), "adaptive_runs_ms": [round(x, 3) for x in runs[1:]], "covered": covered,
            "mean_count": round(mean, 2), "rounds": res["rounds"], "active_left": res["active_rays"],
            "at_min": int((n == MIN_SPP).sum()), "at_max": int((n == MAX_SPP).sum()),
            "plain_floor_spp": int(round(mean)), "plain_floor_ms": plain(c, uvs, offset, max(int(round(mean)), 1)),
            "loop_ms": loop, "trace_ms": trace, "other_ms": other, "host_ms": round(loop - trace - other, 3),
            "outside_share": round((loop - trace) / loop, 4) if loop > 0 else None,
        }
    pt.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
