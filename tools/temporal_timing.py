#!/usr/bin/env python
"""Measures temporal reprojection (ptk_temporal_frame) - not a test, bench.py is untouched.  One process, one JSON
line; every time is a HIP-event time (ptk_last_temporal_ms: the one kernel of a frame call), the median of 25 calls after 3 warm-up
calls.  Per size, on the C2 scene after a plain 4-sample render and a camera move of one degree about the scene's centre:

  frame           ptk_temporal_frame with temporal_defaults: each call reads the history the call before it wrote (after the first
                  call under the same view, so every pixel that sees the scene finds its four taps) and writes the next one
  reset           the same with PTK_TEMPORAL_RESET: no taps, the current frame goes through
  floor_ms        the unique bytes of a frame call at the device copy rate the other timing tools use: 40 B read of the current
                  frame (accumulator, id, position, normal), 48 B of history read, 48 B of history and 16 B of result written
  found_fraction  pixels whose count rose above the frame's own 4 samples
  all_valid       the planes entry (ptk_reproject_planes_device, torch tensors) over a synthetic image of the same size in which EVERY
                  pixel is valid and finds its four taps - the points of the image plane itself under the identity view: its pack
                  kernel and its reprojection kernel, with the latter's own floor (44 B read of the current planes, 48 B of history
                  read, 16 B of result written)

There is no parent to compare with and so no gate.

    python tools/temporal_timing.py [--sizes 1280x720,3840x2160]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 25, 3
COPY_RATE = 6.29e12             # B/s, the measured device copy rate
BYTES_PER_PIXEL = 40 + 48 + 48 + 16
SPP = 4


def timed(c, call):
    """the median, least and most kernel time over REPS calls of call() after WARMUP"""
    runs = []
    for _ in range(WARMUP + REPS):
        call()
        runs.append(c.last_temporal_ms()["kernel_ms"])
    runs = runs[WARMUP:]
    return dict(kernel_ms=round(float(np.median(runs)), 4), min_ms=round(min(runs), 4), max_ms=round(max(runs), 4))


def timed_planes(c, call):
    runs = []
    for _ in range(WARMUP + REPS):
        call()
        runs.append(c.last_temporal_ms())
    runs = runs[WARMUP:]
    return {k: round(float(np.median([r[k] for r in runs])), 4) for k in runs[0]}


def synthetic(view, w, h, dev):
    """the image plane of `view` as the scene: pixel (j, i) sees its own image point, so under the same view it projects onto itself;
    five planes as torch tensors on dev"""
    import torch
    v = {k: np.asarray(x, np.float64) for k, x in view.as_dict().items()}
    j = np.arange(w)[None, :]; i = (h - 1 - np.arange(h))[:, None]
    pos = v["top_left"] + v["right"] * (v["delta_x"] * j)[..., None] - v["up"] * (v["delta_y"] * i)[..., None]
    nrm = np.broadcast_to(np.cross(v["right"], v["up"]), (h, w, 3))
    rng = np.random.default_rng(1)
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    return [t(rng.uniform(0.0, 1.0, (h, w, 3))), t(np.full((h, w), SPP)), t(np.zeros((h, w)), np.int32), t(pos), t(nrm)]


def measure(w, h):
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    from pbrpathtracer_amd.render import orbit_cameras
    tmp = tempfile.mkdtemp(prefix="temporal_")
    pts_file, _, _ = S.build_config("C2", tmp, width=w, height=h)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    pt.SetSeed(1)
    v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
    prm = ptk.temporal_defaults(float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))))
    pt.RenderFrames(SPP)
    pt.TemporalFrame(prm)
    pos, dir_, up = orbit_cameras(pt, 1, 1.0)[0]
    pt.SetCamera(pos, dir_, up)
    pt.ResetImage()
    pt.RenderFrames(SPP)
    pt.TemporalFrame(prm)                        # (renders the guide planes of the new view)
    c = pt.context()
    _, count = c.read_temporal()
    out = {"pixels": w * h, "spp": SPP, "floor_ms": round(w * h * BYTES_PER_PIXEL / COPY_RATE * 1e3, 4),
           "found_fraction": round(float((count > SPP).mean()), 4),
           "valid_fraction": round(float((c.read_feature(ptk.FEAT_MATERIAL) >= 0).mean()), 4),
           "frame": timed(c, lambda: c.temporal_frame(prm, render_features=False)),
           "reset": timed(c, lambda: c.temporal_frame(prm, reset=True, render_features=False))}
    out["frame_over_floor"] = round(out["frame"]["kernel_ms"] / out["floor_ms"], 2)
    import torch
    view = c.get_view()
    planes = synthetic(view, w, h, torch.device("cuda", c.device_ordinal()))
    torch.cuda.synchronize()
    last = {}

    def call():
        last["out"] = c.reproject_planes(view, planes, planes, prm)

    out["all_valid"] = timed_planes(c, call)
    c.synchronize()
    out["all_valid"]["floor_ms"] = round(w * h * (44 + 48 + 16) / COPY_RATE * 1e3, 4)
    out["all_valid"]["found_fraction"] = round(float((last["out"][1] > SPP).float().mean().item()), 4)
    out["all_valid"]["kernel_over_floor"] = round(out["all_valid"]["kernel_ms"] / out["all_valid"]["floor_ms"], 2)
    del planes, last
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
        out[size] = measure(w, h)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
