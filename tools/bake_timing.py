#!/usr/bin/env python3
"""Measures lightmap baking (ptk_bake_lightmap) on C2 and C4 - not a test, bench.py is untouched.  One process, one
JSON line, kernel times from HIP events (ptk_last_bake_ms, ptk_last_rays_ms), medians of REPS runs after a warm-up: lightmap.grid_atlas
at 1024 x 1024, 8 spp, depth 8, offset = 1e-3 of the scene extent.

  coverage_ms, raygen_ms, trace_ms, scatter_ms   the bake's four stages; new_share = (coverage + raygen + scatter) / trace
  --dump-rays DIR    also writes each configuration's compacted rays (origins, dirs; ascending texel index) to DIR/<config>_rays.npz
  --rays-only DIR    instead of baking, traces those rays through ptk_trace_rays_device (e.g. with the parent commit's library,
                     PTK_LIB_PATH) and prints ptk_last_rays_ms for the identical ray set: bake trace_ms / that = the keyed kernel's cost

    python tools/bake_timing.py [--dump-rays DIR | --rays-only DIR]"""
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
SIZE, SPP, DEPTH, SEED = 1024, 8, 8, 7


def med(xs):
    return float(np.median(xs))


def scene_offset(arrays):
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    return float(np.float32(1e-3 * (v.max(axis=0) - v.min(axis=0)).max()))


def bake_rays(c, arrays, uvs, offset):
    """the bake's compacted rays, rebuilt from ptk_bake_coverage's planes in the header's float32 arithmetic"""
    owner, _, pos = c.bake_coverage(SIZE, SIZE, uvs)
    t = np.flatnonzero(owner.reshape(-1) >= 0)
    n = np.ascontiguousarray(arrays["tbn"], np.float32).reshape(-1, 9)[owner.reshape(-1)[t], 0:3]
    return np.ascontiguousarray(pos.reshape(-1, 3)[t] + n * np.float32(offset)), np.ascontiguousarray(-n)


def measure_bake(c, uvs, offset):
    runs = []
    for _ in range(REPS + 1):
        _, owner = c.bake_lightmap(SIZE, SIZE, offset, DEPTH, 0, SPP, SEED, uvs=uvs, device=True)
        runs.append(c.last_bake_ms())
    out = {k: round(med([r[k] for r in runs[1:]]), 4) for k in runs[0]}
    out["trace_runs_ms"] = [round(r["trace_ms"], 4) for r in runs[1:]]
    out["covered"] = int((owner >= 0).sum().item())
    out["new_share"] = round((out["coverage_ms"] + out["raygen_ms"] + out["scatter_ms"]) / out["trace_ms"], 4)
    return out


def measure_rays_only(c, path):
    z = np.load(path)
    ro, rd = torch.from_numpy(z["origins"]).cuda(), torch.from_numpy(z["dirs"]).cuda()
    torch.cuda.synchronize()
    tr = []
    for _ in range(REPS + 1):
        c.trace_rays(ro, rd, DEPTH, 0, SPP, SEED)
        tr.append(c.last_rays_ms()[0])
    return {"rays": len(z["origins"]), "trace_ms": round(med(tr[1:]), 4), "runs_ms": [round(x, 4) for x in tr[1:]]}


def main():
    args = sys.argv[1:]
    dump = args[args.index("--dump-rays") + 1] if "--dump-rays" in args else None
    rays_only = args[args.index("--rays-only") + 1] if "--rays-only" in args else None
    from pbrpathtracer_amd.lightmap import grid_atlas
    tmp = tempfile.mkdtemp(prefix="bake_")
    out = {"size": SIZE, "spp": SPP, "depth": DEPTH}
    for config in ("C2", "C4"):
        pts, _, _ = S.build_config(config, tmp, width=64, height=64, depth=DEPTH)
        pt = PathTracer(0)
        pt.LoadSceneFile(pts)
        pt.RenderFrames(1)                  # BuildBVH's upload; the frame itself is not used
        c = pt.context()
        if rays_only:
            out[config] = measure_rays_only(c, os.path.join(rays_only, f"{config}_rays.npz"))
        else:
            arrays = pt.StagedScene()
            uvs = grid_atlas(pt.GetTriangleCount(), SIZE, SIZE)
            offset = scene_offset(arrays)
            t_uvs = torch.from_numpy(uvs).cuda()
            torch.cuda.synchronize()
            out[config] = dict(measure_bake(c, t_uvs, offset), triangles=pt.GetTriangleCount())
            if dump:
                os.makedirs(dump, exist_ok=True)
                ro, rd = bake_rays(c, arrays, uvs, offset)
                np.savez(os.path.join(dump, f"{config}_rays.npz"), origins=ro, dirs=rd)
        pt.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
