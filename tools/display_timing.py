#!/usr/bin/env python
"""Measures the display transform (ptk_display_planes_device, ptk_display_frame) - not a test, bench.py is untouched.
One process, one JSON line.  Every kernel time is a HIP-event time through ptk_last_display_ms, the median of 25 calls after 3
warm-up calls.  Beside each kernel stands a device-to-device copy that moves the kernel's unique bytes (a copy of half as many:
it reads them once and writes them once), timed with events in the same process in the same way, and the ratio of the two.  Per size:

  noise, constant   the planes entry over log-normal noise (sigma 2) and over a constant image: meter (12 B per pixel read), exposure
                    step (8 KB), apply (12 B read, 3 B written).  The pair shows what the meter's LDS atomics cost where every
                    pixel of a wave lands in one bin and where they scatter.
  manual            the apply kernel alone (manual exposure), ACES + sRGB and LINEAR + LINEAR.
  accum, accum_counts  the frame entry over the accumulator of the C2 scene after a plain 4-sample render (12 / 15 B per pixel) and
                    after an adaptive render, which adds the 4 B count per pixel to both kernels (16 / 19 B).

There is no parent to compare with and so no gate.

    python tools/display_timing.py [--sizes 1280x720,3840x2160]"""
import argparse
import json
import os
import sys
import tempfile

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


def kernels(c, call, dev, pixels, meter_bytes, apply_bytes, metered=True):
    out = {}
    if metered:
        out["meter"] = median_of(call, lambda: c.last_display_ms()["meter_ms"])
        out["meter"]["copy_ms"] = copy_ms(dev, pixels * meter_bytes)
        out["meter"]["over_copy"] = round(out["meter"]["ms"] / out["meter"]["copy_ms"], 2)
        out["exposure"] = median_of(call, lambda: c.last_display_ms()["exposure_ms"])
    out["apply"] = median_of(call, lambda: c.last_display_ms()["apply_ms"])
    out["apply"]["copy_ms"] = copy_ms(dev, pixels * apply_bytes)
    out["apply"]["over_copy"] = round(out["apply"]["ms"] / out["apply"]["copy_ms"], 2)
    return out


def planes(w, h):
    import torch
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    dev = torch.device("cuda", c.device_ordinal())
    rng = np.random.default_rng(1)
    images = {"noise": np.exp(rng.normal(0.0, 2.0, (h, w, 3))).astype(np.float32), "constant": np.full((h, w, 3), 0.37, np.float32)}
    out, keep = {}, {}
    for name, img in images.items():
        t = torch.from_numpy(img).to(dev)
        torch.cuda.synchronize()

        def call(p=ptk.display_defaults()):
            keep["out"] = c.display_planes(t, p)

        out[name] = kernels(c, call, dev, w * h, 12, 15)
        if name == "noise":
            for tag, p in (("manual_aces_srgb", ptk.display_defaults(mode=ptk.EXPOSURE_MANUAL)),
                           ("manual_linear_linear", ptk.display_defaults(mode=ptk.EXPOSURE_MANUAL, op=ptk.DISPLAY_LINEAR, transfer=ptk.TRANSFER_LINEAR))):
                out[tag] = kernels(c, lambda p=p: call(p), dev, w * h, 12, 15, metered=False)
        c.synchronize()
    out["constant_over_noise_meter"] = round(out["constant"]["meter"]["ms"] / out["noise"]["meter"]["ms"], 3)
    c.close()
    return out


def frame(w, h):
    import torch
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    tmp = tempfile.mkdtemp(prefix="display_")
    pts_file, _, _ = S.build_config("C2", tmp, width=w, height=h)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    pt.SetSeed(1)
    c = pt.context()
    dev = torch.device("cuda", c.device_ordinal())
    out = {}
    pt.RenderFrames(4)
    out["accum"] = kernels(c, lambda: c.display_frame(ptk.DISPLAY_ACCUM), dev, w * h, 12, 15)
    pt.RenderAdaptive(0.05, 4, 4, 8)
    out["accum_counts"] = kernels(c, lambda: c.display_frame(ptk.DISPLAY_ACCUM), dev, w * h, 16, 19)
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="1280x720,3840x2160")
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    out = {}
    for size in a.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        out[size] = dict(pixels=w * h, **planes(w, h), **frame(w, h))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
