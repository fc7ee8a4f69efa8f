#!/usr/bin/env python3
"""Measures surface sampling (ptk_sample_surface) beside its floor and its yardstick - not a test, bench.py is
untouched.  One process, one JSON line; per figure the median of REPS runs after a warm-up run of the same shape, with the runs
themselves (their spread is the noise).  Kernel times are HIP-event times (ptk_last_surface_ms, ptk_geometry_timing, torch events
around the copy); the calls are alternated run by run, so that whatever else the machine does falls on all of them alike.

  per scene   the configs named by --configs (C1: the Cornell box; C4: 70 k triangles; C5: 1 M triangles)
  samples     N samples, all five outputs, device tensors: the sampler's two variants ("surface_variant" 0 / 1: plain probes of the
              L2-resident sums / a coarse table staged in LDS first)
  copy        a device-to-device copy of the 40 N bytes the sampling writes: the floor
  table       the table build (weights, quantiser, prefix sum, coarse table; one host wait inside), forced by an identity
              ptk_update_geometry, beside that update's refit: the yardstick for a rebuild

    python tools/surface_sample_timing.py [--configs C1,C4,C5] [--samples N]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 7
N_SAMPLES = 1 << 20
VARIANTS = {"plain": 0, "coarse": 1}         # ("deal": 2, "coarse_deal": 3 with tools/experiments/surface_deal.patch applied)


def med(v):
    return {"ms": round(float(np.median(v)), 4), "runs_ms": [round(float(x), 4) for x in v]}


def measure(c, arrays, n):
    import torch
    dev = torch.device("cuda", c.device_ordinal())
    out = {"triangles": len(arrays["verts"]), "samples": n, "info": [int(x) for x in c.surface_info()[:3]]}
    src = torch.empty(n * 10, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    runs = {k: [] for k in list(VARIANTS) + ["copy"]}
    for r in range(REPS + 1):
        for name, variant in VARIANTS.items():
            c.set_option("surface_variant", variant)
            c.sample_surface(n, seed=3, sample=r, device=True)
            if r:
                runs[name].append(c.last_surface_ms()[1])
        c.synchronize(); torch.cuda.synchronize()
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        if r:
            runs["copy"].append(e0.elapsed_time(e1))
    c.set_option("surface_variant", 1)                                      # (the default)
    out["sample"] = {k: med(v) for k, v in runs.items()}
    table, refit, repack = [], [], []
    for r in range(REPS + 1):
        c.update_geometry(0, arrays["verts"])                               # (identity: marks the table stale)
        c.sample_surface(64, seed=3, device=True)
        if r:
            table.append(c.last_surface_ms()[0])
            g = c.geometry_timing()
            refit.append(g["refit_ms"]); repack.append(g["repack_ms"])
    out["table"] = {"build": med(table), "refit": med(refit), "repack": med(repack)}
    ms = lambda k: out["sample"][k]["ms"]
    out["ratios"] = {f"{k}_over_copy": round(ms(k) / ms("copy"), 3) for k in VARIANTS}
    out["ratios"].update({f"{k}_over_plain": round(ms(k) / ms("plain"), 3) for k in VARIANTS if k != "plain"})
    out["ratios"]["table_over_refit"] = round(out["table"]["build"]["ms"] / out["table"]["refit"]["ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="C1,C4,C5")
    ap.add_argument("--samples", type=int, default=N_SAMPLES)
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    from pbrpathtracer_amd import scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    out = {}
    for cfg in [x for x in a.configs.split(",") if x]:
        tmp = tempfile.mkdtemp(prefix="surface_")
        pts_file, _, _ = S.build_config(cfg, tmp)
        pt = PathTracer(0)
        pt.LoadSceneFile(pts_file)
        arrays = pt.StagedScene()
        pt.sample_surface(1)                                                # (the scene is on the GPU from here on)
        out[cfg] = measure(pt.context(), arrays, a.samples)
        pt.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
