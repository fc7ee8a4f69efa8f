#!/usr/bin/env python3
"""Measures surface attribute queries (ptk_surface_attributes) beside their floor and their yardstick - not a test,
bench.py is untouched.  One process, one JSON line; per figure the median of REPS runs after a warm-up run of the same shape, with
the runs themselves (their spread is the noise).  Kernel times are HIP-event times (ptk_last_attributes_ms, torch events around the
copy and around a train of ptk_render_features launches); the calls are alternated run by run, so that whatever else the machine
does falls on all of them alike.

  per scene   the configs named by --configs (C1: the Cornell box; C3: the textured spheres; C4: 70 k triangles)
  queries     N (triangle, bary) pairs from ptk_sample_surface, random non-unit dirs, device tensors
  all         all nine outputs with dirs, and the same queries sorted by triangle (how much of the time is gather locality); with
              tools/experiments/attributes_stage_dirs.patch applied also the kernel's two variants ("attributes_variant" 0 / 1:
              dirs read at 12 B per lane / dealt through LDS)
  two         MATERIAL + ALBEDO only, no dirs
  copy        a device-to-device copy of a buffer as large as what the kernel reads of the queries plus what it writes (108 B per
              query for `all`, 28 B for `two`): the floor
  frame       --frame CONFIG: at that config's resolution, features_kernel for the six shading planes with the primary-hit cache
              valid, per launch of a train of launches, beside attributes_kernel fed that frame's TRIANGLE and BARY planes and its
              rays for the same six outputs.  --frame-only prints this alone: run it under two builds of the library in turn to set
              features_kernel against another build's.

    python tools/attributes_timing.py [--configs C1,C3,C4] [--queries N] [--frame C4] [--frame-only]"""
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
TRAIN = 40                  # ptk_render_features launches between two events


def med(v):
    return {"ms": round(float(np.median(v)), 4), "runs_ms": [round(float(x), 4) for x in v]}


def measure(c, n):
    import torch
    from pbrpathtracer_amd import ptk
    dev = torch.device("cuda", c.device_ordinal())
    tri, bary = c.sample_surface(n, seed=3, device=True, want=(True, True, False, False, False))[:2]
    g = torch.Generator(device=dev); g.manual_seed(7)
    dirs = torch.randn((n, 3), generator=g, device=dev, dtype=torch.float32) * 3.0
    order = torch.argsort(tri.to(torch.int64))
    s_tri, s_bary, s_dirs = tri[order].contiguous(), bary[order].contiguous(), dirs[order].contiguous()
    c.synchronize(); torch.cuda.synchronize()
    two = 1 << ptk.ATTR_MATERIAL | 1 << ptk.ATTR_ALBEDO
    bytes_all, bytes_two = 24 + 84, 12 + 16
    src = {"copy_all": torch.empty(n * bytes_all // 4, dtype=torch.float32, device=dev).normal_(),
           "copy_two": torch.empty(n * bytes_two // 4, dtype=torch.float32, device=dev).normal_()}
    dst = {k: torch.empty_like(v) for k, v in src.items()}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = {"all": (tri, bary, dirs, ptk.ATTR_ALL), "all_sorted": (s_tri, s_bary, s_dirs, ptk.ATTR_ALL),
             "two": (tri, bary, None, two), "two_sorted": (s_tri, s_bary, None, two)}
    runs = {k: [] for k in list(calls) + list(src)}
    for r in range(REPS + 1):
        for name, (t, b, d, want) in calls.items():
            c.surface_attributes(t, b, d, want)
            if r:
                runs[name].append(c.last_attributes_ms())
        c.synchronize(); torch.cuda.synchronize()
        for name in src:
            e0.record(); dst[name].copy_(src[name]); e1.record(); torch.cuda.synchronize()
            if r:
                runs[name].append(e0.elapsed_time(e1))
    out = {"triangles": c.num_triangles(), "queries": n, "bytes_per_query": {"all": bytes_all, "two": bytes_two}}
    out["kernel"] = {k: med(v) for k, v in runs.items()}
    ms = lambda k: out["kernel"][k]["ms"]
    out["ratios"] = {"all_over_copy": round(ms("all") / ms("copy_all"), 3), "two_over_copy": round(ms("two") / ms("copy_two"), 3),
                     "sorted_over_unsorted_all": round(ms("all_sorted") / ms("all"), 3),
                     "sorted_over_unsorted_two": round(ms("two_sorted") / ms("two"), 3)}
    return out


def frame(config, with_attributes):
    """features_kernel (six shading planes, cached hits) per launch, and attributes_kernel over the same frame's hits"""
    import torch
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    pts, _, _ = S.build_config(config, tempfile.mkdtemp(prefix="attr_frame_"))
    pt = PathTracer(0); pt.LoadSceneFile(pts); pt.SetCameraAperture(0.0)
    pt.RenderFeatures(ptk.FEAT_ALL)                      # stages camera and frame, allocates the planes, fills the primary-hit cache
    c = pt.context()
    w, h = pt.GetResolution()
    dev = torch.device("cuda", c.device_ordinal())
    shading = sum(1 << k for k in (ptk.FEAT_MATERIAL, ptk.FEAT_NORMAL_GEOM, ptk.FEAT_NORMAL, ptk.FEAT_ALBEDO, ptk.FEAT_EMISSION, ptk.FEAT_GLOSS))
    tri = pt.ReadFeature(ptk.FEAT_TRIANGLE); bary = pt.ReadFeature(ptk.FEAT_BARY); pos = pt.ReadFeature(ptk.FEAT_POSITION)
    out = {"config": config, "width": w, "height": h, "triangles": pt.GetTriangleCount(), "hit_fraction": round(float((tri >= 0).mean()), 4),
           "library": os.path.basename(ptk.LIB_PATH), "launches_per_run": TRAIN}
    s = torch.cuda.Stream(device=dev)
    c.set_stream(s.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    feat, attr = [], []
    if with_attributes:
        rd = pos.reshape(-1, 3) - np.asarray(pt.GetCamera()[0], np.float32)           # (the rays' directions, not normalised: only the sign counts)
        t_tri = torch.from_numpy(np.ascontiguousarray(tri.reshape(-1))).to(dev)
        t_bary = torch.from_numpy(np.ascontiguousarray(bary.reshape(-1, 2))).to(dev)
        t_rd = torch.from_numpy(np.ascontiguousarray(rd)).to(dev)
        want = sum(1 << k for k in (ptk.ATTR_MATERIAL, ptk.ATTR_NORMAL_GEOM, ptk.ATTR_NORMAL, ptk.ATTR_ALBEDO, ptk.ATTR_EMISSION, ptk.ATTR_GLOSS))
    torch.cuda.synchronize()
    for r in range(REPS + 1):
        with torch.cuda.stream(s):
            e0.record(s)
            for _ in range(TRAIN):
                c.render_features(shading)
            e1.record(s)
        s.synchronize()
        if r:
            feat.append(e0.elapsed_time(e1) / TRAIN)
        if with_attributes:
            with torch.cuda.stream(s):
                c.surface_attributes(t_tri, t_bary, t_rd, want)
            s.synchronize()
            if r:
                attr.append(c.last_attributes_ms())
    out["features_kernel"] = med(feat)
    if with_attributes:
        out["attributes_kernel"] = med(attr)
        out["attributes_over_features"] = round(out["attributes_kernel"]["ms"] / out["features_kernel"]["ms"], 3)
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="C1,C3,C4")
    ap.add_argument("--queries", type=int, default=N_QUERIES)
    ap.add_argument("--frame", default="C4")
    ap.add_argument("--frame-only", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    from pbrpathtracer_amd import scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    if a.frame_only:
        print(json.dumps({"frame": frame(a.frame, False)}), flush=True)
        return
    out = {}
    for cfg in [x for x in a.configs.split(",") if x]:
        tmp = tempfile.mkdtemp(prefix="attributes_")
        pts_file, _, _ = S.build_config(cfg, tmp)
        pt = PathTracer(0)
        pt.LoadSceneFile(pts_file)
        pt.sample_surface(1)                                                # (the scene is on the GPU from here on)
        out[cfg] = measure(pt.context(), a.queries)
        pt.close()
    if a.frame:
        out["frame"] = frame(a.frame, True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
