"""Adaptive render (include/ptk.h ptk_render_adaptive) on C2, C3, C4 at their BASELINE sizes: how many pixel samples it takes
at a few thresholds, its wall time, the per-round overhead (adaptive at threshold 0 - every pixel to max_spp in rounds - against
one ptk_render of max_spp), and the RMSE against a high-spp reference of the adaptive image and of a uniform image rendered in
the same wall time.  One JSON line per config.

    python tools/adaptive_probe.py [--configs C2,C3,C4] [--step 8] [--min-spp 16] [--thresholds 0.1,0.05,0.02] [--ref-mult 4]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, r


def mean_image(ctx, counts=None):
    tot = ctx.read_accum().astype(np.float64)
    n = counts if counts is not None else np.full(tot.shape[:2], ctx.samples())
    return tot / np.maximum(n, 1)[..., None]


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C4")
    ap.add_argument("--step", type=int, default=8)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--thresholds", default="0.1,0.05,0.02")
    ap.add_argument("--ref-mult", type=int, default=4)
    a = ap.parse_args()
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer, camera_from_scene
    tmp = tempfile.mkdtemp(prefix="adaptive_probe_")
    for name in a.configs.split(","):
        pts, scene, spp = S.build_config(name, tmp)
        pt = PathTracer(device=0)
        pt.LoadSceneFile(pts)
        arrays = pt.StagedScene()
        W, H = pt.GetResolution()
        ctx = ptk.Context(0)
        ctx.upload_scene(arrays); ctx.set_camera(**camera_from_scene(scene)); ctx.set_frame(W, H, int(scene.trace_depth))
        ctx.set_option("overlap", 1)
        seed = 1
        # warm-up (allocations, caches) and the reference
        ctx.reset(); ctx.render(0, a.step, seed); ctx.synchronize()
        ctx.reset()
        t_ref, _ = timed(ctx, lambda: ctx.render(0, spp * a.ref_mult, 1000))
        ref = mean_image(ctx)
        ctx.reset()
        t_uni, _ = timed(ctx, lambda: ctx.render(0, spp, seed))
        uni_rmse = rmse(mean_image(ctx), ref)
        t_a0, r0 = timed(ctx, lambda: ctx.render_adaptive(0.0, a.min_spp, a.step, spp, seed))
        line = dict(config=name, width=W, height=H, max_spp=spp, step=a.step, min_spp=a.min_spp, ref_spp=spp * a.ref_mult,
                    uniform_s=round(t_uni, 4), uniform_rmse=uni_rmse, adaptive_t0_s=round(t_a0, 4), rounds_t0=r0["rounds"],
                    overhead_per_round_ms=round((t_a0 - t_uni) / max(1, r0["rounds"]) * 1e3, 4), thresholds=[])
        per_spp = t_uni / spp
        for thr in [float(x) for x in a.thresholds.split(",")]:
            t_ad, r = timed(ctx, lambda: ctx.render_adaptive(thr, a.min_spp, a.step, spp, seed))
            ad_rmse = rmse(mean_image(ctx, ctx.read_sample_counts()), ref)
            eq = max(1, int(round(t_ad / per_spp)))
            ctx.reset()
            t_eq, _ = timed(ctx, lambda: ctx.render(0, eq, seed))
            line["thresholds"].append(dict(threshold=thr, samples_fraction=round(r["pixel_samples"] / (W * H * spp), 4),
                                           rounds=r["rounds"], active_pixels=r["active_pixels"], adaptive_s=round(t_ad, 4),
                                           adaptive_rmse=ad_rmse, uniform_equal_time_spp=eq, uniform_equal_time_s=round(t_eq, 4),
                                           uniform_equal_time_rmse=rmse(mean_image(ctx), ref)))
        print(json.dumps(line), flush=True)
        ctx.close()
        del pt


if __name__ == "__main__":
    main()
