#!/usr/bin/env python
"""Measures the temporal moments and the variance made of them (ptk_temporal_frame_moments, ptk_variance_planes_device; DESIGN.md
§4.21) - not a test, bench.py is untouched.  One process, one JSON line; every time is a HIP-event time, the median of 25 calls after
3 warm-up calls, and every floor is the call's unique bytes at the device copy rate the other timing tools use.  Per size:

  plain, moments  on the C2 scene after a plain 4-sample render and a camera move of one degree, as tools/temporal_timing.py has it:
                  ptk_temporal_frame and ptk_temporal_frame_moments in the same process, each call reading the history the call
                  before it wrote (plain_again: the plain entry once more behind the moments runs - the drift of the process).
                  Floors: 152 B per pixel for the plain kernel; the moments kernel adds 12 B of albedo and 16 B of moment history
                  read, 16 B of moment history and 8 B of moments written: 204 B.  C2 shows sky in most pixels, which read and
                  write less than that, so both may run below their floors; all_valid has the same pair through the planes entries
                  (ptk_reproject_planes_device, ptk_reproject_moments_device) over tools/temporal_timing.py's synthetic image in which
                  every pixel finds its four taps: floors 108 B and, with albedo, moment history and moments, 144 B.
  temporal_variance  ptk_temporal_variance over what the last moments call left (variance_defaults): its two kernels.
  variance        variance_kernel (radius 3) through the planes entry over a synthetic image in which every pixel is valid and lies
                  on one plane, so that a pixel with a short history takes all 49 taps: no pixel with a short history, one in ten in
                  blocks of 64 x 16 pixels (how disocclusions come), one in ten scattered pixel by pixel (nearly every wave then holds
                  one and walks the window), and all of them.  Floor: 20 B per pixel - the moments image read, the raw variance
                  written - plus 32 B of position + id and normal where the window runs.
  prefilter       variance_prefilter_kernel behind it: 4 B read, 4 B written.

The cost of the moments kernel is to be judged against the plain one of the same run, not against a fixed figure; there is no parent
to compare with and so no gate.

    python tools/variance_timing.py [--sizes 1280x720,3840x2160]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

REPS, WARMUP = 25, 3
COPY_RATE = 6.29e12             # B/s, the measured device copy rate
PLAIN_BYTES, MOMENTS_BYTES = 152, 204
SPP = 4


def timed(c, call, read):
    """the median, least and most of read() over REPS calls of call() after WARMUP"""
    runs = []
    for _ in range(WARMUP + REPS):
        call()
        runs.append(read())
    runs = runs[WARMUP:]
    return dict(ms=round(float(np.median(runs)), 4), min_ms=round(min(runs), 4), max_ms=round(max(runs), 4))


def with_floor(t, pixels, bytes_per_pixel):
    t["floor_ms"] = round(pixels * bytes_per_pixel / COPY_RATE * 1e3, 4)
    t["over_floor"] = round(t["ms"] / t["floor_ms"], 2)
    return t


def frame_entries(w, h):
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    from pbrpathtracer_amd.render import orbit_cameras
    tmp = tempfile.mkdtemp(prefix="variance_")
    pts_file, _, _ = S.build_config("C2", tmp, width=w, height=h)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    pt.SetSeed(1)
    v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
    ext = float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))
    prm = ptk.temporal_defaults(ext); vp = ptk.variance_defaults(ext)
    pt.RenderFrames(SPP)
    pt.TemporalFrameMoments(prm)
    pos, dir_, up = orbit_cameras(pt, 1, 1.0)[0]
    pt.SetCamera(pos, dir_, up)
    pt.ResetImage()
    pt.RenderFrames(SPP)
    pt.TemporalFrameMoments(prm)                 # (renders the guide planes of the new view)
    c = pt.context()
    kernel = lambda: c.last_temporal_ms()["kernel_ms"]
    out = {}
    out["plain"] = with_floor(timed(c, lambda: c.temporal_frame(prm, render_features=False), kernel), w * h, PLAIN_BYTES)
    c.temporal_frame(prm, render_features=False, moments=True)          # (behind a plain call: starts over; the timed calls find history)
    out["moments"] = with_floor(timed(c, lambda: c.temporal_frame(prm, render_features=False, moments=True), kernel), w * h, MOMENTS_BYTES)
    out["found_fraction"] = round(float((c.read_temporal()[1] > SPP).mean()), 4)
    # the frame entry's variance over what the last call left: every pixel with history has had 29 frames by now
    out["temporal_variance"] = {k: timed(c, lambda: c.temporal_variance(vp), lambda: c.last_variance_ms()[k + "_ms"])["ms"] for k in ("variance", "prefilter")}
    out["all_valid"] = all_valid(c, prm, w, h)
    out["plain_again"] = with_floor(timed(c, lambda: c.temporal_frame(prm, render_features=False), kernel), w * h, PLAIN_BYTES)
    out["moments_over_plain"] = round(out["moments"]["ms"] / out["plain"]["ms"], 3)
    out["bytes_over_plain"] = round(MOMENTS_BYTES / PLAIN_BYTES, 3)
    pt.close()
    return out


def all_valid(c, prm, w, h):
    """the planes entries with and without moments over an image in which every pixel is valid and finds its four taps"""
    import torch
    from temporal_timing import synthetic
    view = c.get_view()
    dev = torch.device("cuda", c.device_ordinal())
    planes = synthetic(view, w, h, dev)
    rng = np.random.default_rng(2)
    mom = torch.from_numpy(rng.uniform(0.2, 1.0, (h, w, 2)).astype(np.float32)).to(dev)
    albedo = torch.from_numpy(rng.uniform(0.2, 0.8, (h, w, 3)).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    keep = {}

    def plain():
        keep["out"] = c.reproject_planes(view, planes, planes, prm)

    def moments():
        keep["out"] = c.reproject_moments(view, planes, planes + [mom], prm, albedo=albedo)

    kernel = lambda: c.last_temporal_ms()["kernel_ms"]
    out = {"plain": with_floor(timed(c, plain, kernel), w * h, 108), "moments": with_floor(timed(c, moments, kernel), w * h, 144)}
    c.synchronize()
    out["found_fraction"] = round(float((keep["out"][1] > SPP).float().mean().item()), 4)
    out["moments_over_plain"] = round(out["moments"]["ms"] / out["plain"]["ms"], 3)
    out["bytes_over_plain"] = round(144 / 108, 3)
    return out


def variance_planes(w, h):
    import torch
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    dev = torch.device("cuda", c.device_ordinal())
    rng = np.random.default_rng(1)
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    m1 = rng.uniform(0.5, 1.0, (h, w)).astype(np.float32)
    mom = t(np.stack([m1, m1 * m1 + rng.uniform(0.0, 0.1, (h, w)).astype(np.float32)], axis=-1))
    pos = np.zeros((h, w, 3), np.float32); pos[..., 0] = np.arange(w)[None, :] * 0.01; pos[..., 1] = np.arange(h)[:, None] * 0.01
    nrm = np.zeros((h, w, 3), np.float32); nrm[..., 2] = 1
    ident, pos, nrm, f = t(np.zeros((h, w)), np.int32), t(pos), t(nrm), t(np.full((h, w), 2.0))
    blocks = np.kron(rng.random(((h + 15) // 16, (w + 63) // 64)) < 0.1, np.ones((16, 64), bool))[:h, :w]
    short = {"none": np.zeros((h, w), bool), "tenth_in_blocks": blocks, "tenth_scattered": rng.random((h, w)) < 0.1, "all": np.ones((h, w), bool)}
    out = {}
    for prefilter in (0, 1):
        vp = ptk.VarianceParams(3, prefilter, 4.0, 1.0, 0.9)
        for name, mask in short.items():
            n = t(np.where(mask, 2.0, 32.0))
            torch.cuda.synchronize()
            keep = {}

            def call():
                keep["out"] = c.variance_planes(mom, n, f, ident, pos, nrm, vp)

            if not prefilter:
                r = with_floor(timed(c, call, lambda: c.last_variance_ms()["variance_ms"]), w * h, 20 + 32 * float(mask.mean()))
                r["short_fraction"] = round(float(mask.mean()), 4)
                out["variance_" + name] = r
            elif name == "none":
                out["prefilter"] = with_floor(timed(c, call, lambda: c.last_variance_ms()["prefilter_ms"]), w * h, 8)
            c.synchronize()
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="1280x720,3840x2160")
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    out = {}
    for size in a.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        out[size] = dict(pixels=w * h, spp=SPP, **frame_entries(w, h), **variance_planes(w, h))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
