#!/usr/bin/env python3
"""Measures closest-hit and occlusion queries (ptk_intersect_rays, ptk_occluded_rays) - not a test, bench.py is
untouched.  One process, one JSON line, medians of REPS runs after a warm-up; kernel times are HIP-event times (ptk_last_hits_ms).

  (a) hit rate    rays per second of hits_kernel on 2^20 rays inside the scene's bounds (tests/ray_cases.py rays_in_box) of C4 and
                  of C5, the 1 M-triangle scene.  Beside it ptk_probe_hits - the parity probe, the same walk in 256-thread
                  workgroups without the pipelined node record - on the same rays: it has no timing hook, so its figure is the
                  WALL time of the host call (staging and copies included), next to the wall time of ptk_intersect_rays' host call
  (b) occlusion   occluded_kernel over hits_kernel on the same rays with tmax = inf (`occluded_over_hits` = rate ratio; above 1:
                  the walk stops at the first accepted triangle), and with tmax = the scene's extent / 4
  (c) bench       with --bench: bench.py --gpus 1 at C2 and C4, each in a process of its own, ROUNDS times; with
                  --parent-lib pbrpathtracer_amd/libptk_NAME.so (a build of the parent commit) alternating with that library
                  (PTK_DEV_TOOLS=1 PTK_LIB_PATH=...), ms_per_step medians side by side

    python tools/hits_timing.py [--configs C4,C5] [--bench [--parent-lib LIB] [--steps N]]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, ROUNDS = 5, 3
N_RAYS = 1 << 20
SEED = 7


def rays_in_box(arrays, n, seed):
    """tests/ray_cases.py rays_in_box: origins uniform in the vertex bounds grown by 10 % per side, directions uniform on the sphere"""
    rng = np.random.default_rng(seed)
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    pad = 0.1 * (hi - lo)
    ro = rng.uniform(lo - pad, hi + pad, (n, 3))
    rd = rng.normal(0.0, 1.0, (n, 3))
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    return np.ascontiguousarray(ro, np.float32), np.ascontiguousarray(rd, np.float32), float((hi - lo).max())


def med(xs):
    return float(np.median(xs))


def timed(call, kernel_ms=None):
    """medians over REPS runs after a warm-up of (kernel ms or None, wall ms of the call)"""
    k, w = [], []
    for _ in range(REPS + 1):
        t0 = time.perf_counter()
        call()
        w.append((time.perf_counter() - t0) * 1e3)
        if kernel_ms:
            k.append(kernel_ms())
    return (med(k[1:]) if kernel_ms else None), med(w[1:]), ([round(x, 4) for x in k[1:]] if kernel_ms else [round(x, 3) for x in w[1:]])


def measure_config(cfg):
    import torch
    from pbrpathtracer_amd import scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    tmp = tempfile.mkdtemp(prefix="hits_")
    pts, _, _ = S.build_config(cfg, tmp)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    arrays = pt.StagedScene()
    ro, rd, extent = rays_in_box(arrays, N_RAYS, 5)
    pt.IntersectRays(ro[:64], rd[:64])          # (the scene is on the GPU from here on)
    c = pt.context()
    dev = torch.device("cuda", c.device_ordinal())
    d_ro, d_rd = torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev)
    d_inf = torch.full((N_RAYS,), float("inf"), dtype=torch.float32, device=dev)
    d_near = torch.full((N_RAYS,), extent / 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    out = {"triangles": pt.GetTriangleCount(), "rays": N_RAYS}
    res = {}

    def hits():
        res["hits"] = c.intersect_rays(d_ro, d_rd, 0, SEED)
    k, _, runs = timed(hits, c.last_hits_ms)
    rate = lambda ms: round(N_RAYS / (ms * 1e-3))
    out["hit_fraction"] = round(float((res["hits"][0] >= 0).float().mean().item()), 4)
    out["hits"] = {"kernel_ms": round(k, 4), "runs_ms": runs, "rays_per_s": rate(k)}
    for name, tm in (("occluded_inf", d_inf), ("occluded_near", d_near)):
        def occ():
            res[name] = c.occluded_rays(d_ro, d_rd, tm, 0, SEED)
        k2, _, runs = timed(occ, c.last_hits_ms)
        out[name] = {"kernel_ms": round(k2, 4), "runs_ms": runs, "rays_per_s": rate(k2), "occluded_fraction": round(float(res[name].float().mean().item()), 4),
                     "occluded_over_hits": round(k / k2, 4)}
    _, w_hits, runs = timed(lambda: c.intersect_rays(ro, rd, 0, SEED))
    out["hits_host_call"] = {"wall_ms": round(w_hits, 3), "runs_ms": runs, "rays_per_s_wall": rate(w_hits)}
    _, w_probe, runs = timed(lambda: c.probe_hits(ro, rd))
    out["probe_hits_host_call"] = {"wall_ms": round(w_probe, 3), "runs_ms": runs, "rays_per_s_wall": rate(w_probe), "kernel_ms": "no timing hook: wall time only"}
    out["hits_over_probe_wall"] = round(w_probe / w_hits, 4)
    pt.close()
    return out


def bench_once(cfg, steps, lib):
    env = dict(os.environ)
    if lib:
        env["PTK_DEV_TOOLS"] = "1"; env["PTK_LIB_PATH"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "10", "--config", cfg],
                       env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py {cfg} failed ({p.returncode}): {p.stderr[-400:]}")
    for line in reversed(p.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)["ms_per_step"]
    raise RuntimeError("bench.py printed no JSON line")


def measure_bench(steps, parent_lib):
    out = {}
    for cfg in ("C2", "C4"):
        tree, parent = [], []
        for _ in range(ROUNDS):
            tree.append(bench_once(cfg, steps, None))
            if parent_lib:
                parent.append(bench_once(cfg, steps, parent_lib))
        out[cfg] = {"steps": steps, "ms_per_step": med(tree), "runs": tree}
        if parent_lib:
            out[cfg].update({"parent_ms_per_step": med(parent), "parent_runs": parent, "tree_over_parent": round(med(tree) / med(parent), 4)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="C4,C5")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--steps", type=int, default=100)
    a = ap.parse_args()
    out = {}
    if a.bench:          # (before this process opens the GPU itself: one process on it at a time)
        out["bench"] = measure_bench(a.steps, a.parent_lib)
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    for cfg in [x for x in a.configs.split(",") if x]:
        out[cfg] = measure_config(cfg)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
