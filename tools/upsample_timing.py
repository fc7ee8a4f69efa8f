#!/usr/bin/env python
"""Measures guided upsampling (ptk_upsample_frame, ptk_render_guides) - not a test, bench.py is untouched.
One process, one JSON line.  Every kernel time is a HIP-event time through ptk_last_upsample_ms, the median of 25 calls after 3
warm-up calls.  Beside each kernel stands a device-to-device copy that moves the kernel's unique bytes (a copy of half as many:
it reads them once and writes them once), timed with events in the same process in the same way, and the ratio of the two.  Per pair
of sizes, over the C2 scene after a plain 4-sample render at the low size:

  pack      the low planes into texels: 52 B read and 64 B written per LOW pixel (colour, id, position, normal, albedo).
  kernel    upsample_kernel with albedo planes and ring 1 on: the 64 B texels of every low pixel once, 40 B of guide planes read and
            16 B written per HIGH pixel.
  guides    ptk_render_guides of the four planes at the high size: host wall time from the call to the end of the stream, the
            median of the same number of calls (two kernels; there is no event pair around them).
  classes   the shares of the three classes over the whole image, for the record.

There is no parent to compare with and so no gate.

    python tools/upsample_timing.py [--pairs 1280x720:2560x1440,1920x1080:3840x2160]"""
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


def median_of(call, read):
    runs = []
    for _ in range(WARMUP + REPS):
        call()
        runs.append(read())
    runs = runs[WARMUP:]
    return dict(ms=round(float(np.median(runs)), 4), min_ms=round(min(runs), 4), max_ms=round(max(runs), 4))


def copy_ms(dev, traffic_bytes):
    """a device-to-device copy that reads and writes traffic_bytes in all"""
    import torch
    n = max(int(traffic_bytes) // 2, 1)
    src = torch.empty(n, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    runs = []
    for _ in range(WARMUP + REPS):
        a.record(); dst.copy_(src); b.record(); b.synchronize()
        runs.append(a.elapsed_time(b))
    return round(float(np.median(runs[WARMUP:])), 4)


def beside_copy(entry, dev, traffic_bytes):
    entry["bytes"] = int(traffic_bytes)
    entry["copy_ms"] = copy_ms(dev, traffic_bytes)
    entry["over_copy"] = round(entry["ms"] / entry["copy_ms"], 2)
    return entry


def pair(w, h, W, H):
    import torch
    from pbrpathtracer_amd import ptk, scenes as S, upscale
    from pbrpathtracer_amd.pathtracer import PathTracer
    tmp = tempfile.mkdtemp(prefix="upsample_")
    pts_file, _, _ = S.build_config("C2", tmp, width=w, height=h)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    pt.SetSeed(1)
    c = pt.context()
    dev = torch.device("cuda", c.device_ordinal())
    pt.RenderFrames(4)
    c.render_features(ptk.UPSAMPLE_GUIDES, 0, 1)
    c.synchronize()

    def guides():
        t = time.perf_counter()
        c.render_guides(W, H, ptk.UPSAMPLE_GUIDES, 0, 1)
        c.synchronize()
        return (time.perf_counter() - t) * 1e3

    wall = [guides() for _ in range(WARMUP + REPS)][WARMUP:]
    out = dict(low_pixels=w * h, high_pixels=W * H)
    out["guides"] = dict(wall_ms=round(float(np.median(wall)), 4), min_ms=round(min(wall), 4), max_ms=round(max(wall), 4))
    v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
    prm = ptk.upsample_defaults(float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))))
    call = lambda: c.upsample_frame(ptk.UPSAMPLE_ACCUM, prm)
    out["pack"] = beside_copy(median_of(call, lambda: c.last_upsample_ms()["pack_ms"]), dev, w * h * (52 + 64))
    out["kernel"] = beside_copy(median_of(call, lambda: c.last_upsample_ms()["kernel_ms"]), dev, w * h * 64 + W * H * (40 + 16))
    out["classes"] = [round(s, 5) for s in upscale.class_shares(c.read_upsampled()[1])]
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", default="1280x720:2560x1440,1920x1080:3840x2160")
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    out = {}
    for p in a.pairs.split(","):
        lo, hi = p.split(":")
        (w, h), (W, H) = ((int(x) for x in s.split("x")) for s in (lo, hi))
        out[p] = pair(w, h, W, H)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
