#!/usr/bin/env python3
"""Measures the a-trous denoiser (ptk_denoise_frame) - not a test, bench.py is untouched.  One process, one JSON
line; every time is a HIP-event time (ptk_last_denoise_ms: pack kernel, the filter launches together, unpack kernel), the median
of REPS calls after WARMUP calls.

  per size        the C2 scene (the 12-triangle Cornell box of BASELINE.md) at 1280x720 and at 3840x2160, --sizes for others
  plain           8 samples per pixel by ptk_render, the five guide planes, ptk_denoise_frame with denoise_defaults
  variance        an adaptive render (threshold 0.05, 8..32 samples), the same with PTK_DENOISE_VARIANCE
  all_valid       the planes entry (ptk_denoise_planes_device, torch tensors) over a synthetic image of the same size in which EVERY
                  pixel is valid - two perpendicular planes, multiplicative noise, albedo - plain and with a variance plane: the
                  frame of C2 is mostly background (valid_fraction), whose pixels the filter only copies
  floor_ms        the unique bytes of the filter - 48 B read and 16 B written per pixel and iteration - at the 6.29 TB/s copy rate
  c2_step_ms      (1280x720 only) one 256-sample ptk_render of C2, for scale

    python tools/denoise_timing.py [--sizes 1280x720,3840x2160] [--iterations 5]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 25, 3
COPY_RATE = 6.29e12             # B/s, the measured device copy rate
FIVE = (1 << 1) | (1 << 4) | (1 << 6) | (1 << 7) | (1 << 8)


def timed(c, call):
    """the medians of the three event times and of their sum over REPS calls of call() after WARMUP"""
    runs = []
    for _ in range(WARMUP + REPS):
        call()
        runs.append(c.last_denoise_ms())
    runs = runs[WARMUP:]
    total = [sum(r.values()) for r in runs]
    return dict({k: round(float(np.median([r[k] for r in runs])), 4) for k in runs[0]}, total_ms=round(float(np.median(total)), 4),
                total_min_ms=round(min(total), 4), total_max_ms=round(max(total), 4))


def synthetic(w, h, dev):
    """two perpendicular planes meeting at the middle column, every pixel valid; torch tensors on dev"""
    import torch
    rng = np.random.default_rng(1)
    x = np.arange(w, dtype=np.float32)[None, :].repeat(h, 0) / w
    y = np.arange(h, dtype=np.float32)[:, None].repeat(w, 1) / w
    left = x < 0.5
    pos = np.where(left[..., None], np.stack([x, y, np.zeros_like(x)], -1), np.stack([np.full_like(x, 0.5), y, x - 0.5], -1))
    nrm = np.where(left[..., None], np.float32([0, 0, 1]), np.float32([1, 0, 0]))
    albedo = np.where(left[..., None], np.float32([0.7, 0.3, 0.3]), np.float32([0.3, 0.7, 0.3]))
    noise = rng.gamma(8.0, 1.0 / 8.0, (h, w, 1)).astype(np.float32)
    color = albedo * np.where(left, 0.5, 2.0)[..., None].astype(np.float32) * noise
    var = np.full((h, w), (1.25 ** 2) / 8.0 / 8.0, np.float32)
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    return dict(color=t(color), mask=t(np.zeros((h, w)), np.int32), normal=t(nrm), position=t(pos), albedo=t(albedo), variance=t(var))


def timed_planes(c, pl, prm, variance):
    return timed(c, lambda: c.denoise_planes(pl["color"], pl["mask"], pl["normal"], pl["position"], prm, albedo=pl["albedo"],
                                             variance=pl["variance"] if variance else None))


def timed_frame(c, prm, variance):
    return timed(c, lambda: c.denoise_frame(prm, variance=variance, render_features=False))


def measure(w, h, iterations):
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    tmp = tempfile.mkdtemp(prefix="denoise_")
    pts_file, _, _ = S.build_config("C2", tmp, width=w, height=h)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    pt.SetSeed(1)
    pt.RenderFrames(8)
    c = pt.context()
    v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
    extent = float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))
    c.render_features(FIVE, 0, 1)
    out = {"pixels": w * h, "iterations": iterations,
           "floor_ms": round(w * h * 64.0 * iterations / COPY_RATE * 1e3, 4),
           "plain": timed_frame(c, ptk.denoise_defaults(extent, False, iterations), False)}
    valid = c.read_feature(ptk.FEAT_TRIANGLE) >= 0
    out["valid_fraction"] = round(float(valid.mean()), 4)
    c.render_adaptive(0.05, 8, 8, 32, 1)
    c.render_features(FIVE, 0, 1)
    out["variance"] = timed_frame(c, ptk.denoise_defaults(extent, True, iterations), True)
    import torch
    pl = synthetic(w, h, torch.device("cuda", c.device_ordinal()))
    torch.cuda.synchronize()
    out["all_valid"] = {"plain": timed_planes(c, pl, ptk.denoise_defaults(1.0, False, iterations), False),
                        "variance": timed_planes(c, pl, ptk.denoise_defaults(1.0, True, iterations), True)}
    del pl
    if (w, h) == (1280, 720):
        c.reset()
        c.render(0, 256, 1); c.synchronize()
        steps = []
        for k in range(5):
            t0 = time.perf_counter()
            c.render(256 * (k + 1), 256, 1); c.synchronize()
            steps.append((time.perf_counter() - t0) * 1e3)
        out["c2_step_ms"] = round(float(np.median(steps)), 3)
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="1280x720,3840x2160")
    ap.add_argument("--iterations", type=int, default=5)
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    out = {}
    for size in a.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        out[size] = measure(w, h, a.iterations)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
