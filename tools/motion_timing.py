#!/usr/bin/env python
"""Measures temporal reprojection over moving geometry (ptk_temporal_frame_moving) - not a test, bench.py is
untouched.  One process, one JSON line per scene; every time is a HIP-event time (ptk_last_motion_ms: motion_kernel and the MOVING
reprojection kernel behind it; ptk_last_temporal_ms for the plain entry), the median of 25 calls after 3 warm-up calls.  Per scene
(C2: 12 triangles; C5: about a million) and size, from a camera in the opening of the Cornell shell, so that every pixel sees the
scene, after a plain 4-sample render and a first call that left a history under the same view:

  plain           ptk_temporal_frame on the same frame: the kernel this feature leaves as it was
  none_moved      ptk_temporal_frame_moving with a snapshot equal to the resident vertices: every triangle compares unmoved
  all_moved       the same after every vertex was shifted by 1e-3 of the scene's size (ptk_update_geometry) and the frame rendered
                  again: every pixel that sees the scene takes the moved arm
  floor_ms        the unique bytes at the device copy rate the other timing tools use.  motion_kernel: 36 B of planes read (triangle,
                  bary, position, normal) and 32 B written per pixel, plus 72 B for each distinct triangle the frame sees (its two
                  vertex records).  The MOVING reprojection kernel: the plain kernel's 152 B per pixel plus the 24 B of X' and n'.

There is no parent to compare the new kernels with and so no gate.

    python tools/motion_timing.py [--sizes 1280x720,3840x2160] [--scenes C2,C5]"""
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
SPP = 4


def timed(call, read):
    """the median, least and most of every time read() reports over REPS calls of call() after WARMUP"""
    runs = []
    for _ in range(WARMUP + REPS):
        call()
        runs.append(read())
    runs = runs[WARMUP:]
    return {k: dict(median=round(float(np.median([r[k] for r in runs])), 4), min=round(min(r[k] for r in runs), 4),
                    max=round(max(r[k] for r in runs), 4)) for k in runs[0]}


def measure(scene, w, h):
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer
    tmp = tempfile.mkdtemp(prefix="motion_")
    pts_file, _, _ = S.build_config(scene, tmp, width=w, height=h)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts_file)
    pt.SetCameraAperture(0.0)
    pt.SetCamera((0.0, 0.0, -0.95), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0))        # in the box's opening: every pixel sees the scene
    pt.SetSeed(1)
    arrays = pt.StagedScene()
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    size = float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))
    prm = ptk.temporal_defaults(size)
    pt.RenderFrames(SPP)
    pt.TemporalFrameMoving(prm)                  # (renders the guide planes; leaves a history under this view)
    c = pt.context()
    tri = c.read_feature(ptk.FEAT_TRIANGLE)
    seen = int(len(np.unique(tri[tri >= 0])))
    px = w * h
    out = {"pixels": px, "triangles": len(arrays["verts"]), "triangles_seen": seen, "valid_fraction": round(float((tri >= 0).mean()), 4),
           "floor_ms": {"motion_ms": round((px * 68 + seen * 72) / COPY_RATE * 1e3, 4), "temporal_ms": round(px * 176 / COPY_RATE * 1e3, 4),
                        "plain_ms": round(px * 152 / COPY_RATE * 1e3, 4)}}
    plain = timed(lambda: c.temporal_frame(prm, render_features=False), c.last_temporal_ms)
    out["plain"] = plain["kernel_ms"]
    c.snapshot_geometry()
    out["none_moved"] = timed(lambda: c.temporal_frame(prm, render_features=False, moving=True), c.last_motion_ms)
    moved = (np.asarray(arrays["verts"], np.float32) + np.float32(1e-3 * size)).astype(np.float32)
    c.snapshot_geometry()
    c.update_geometry(0, moved)
    c.reset(); c.render(0, SPP, 1)
    c.render_features((1 << ptk.FEAT_MATERIAL) | (1 << ptk.FEAT_TRIANGLE) | (1 << ptk.FEAT_BARY) | (1 << ptk.FEAT_POSITION) | (1 << ptk.FEAT_NORMAL), 0, 1)
    out["all_moved"] = timed(lambda: c.temporal_frame(prm, render_features=False, moving=True), c.last_motion_ms)
    pp, _, mv = c.read_motion()
    hit = c.read_feature(ptk.FEAT_TRIANGLE) >= 0
    out["all_moved"]["moved_fraction_of_hits"] = round(float((pp != c.read_feature(ptk.FEAT_POSITION)).any(axis=-1)[hit].mean()), 4)
    out["all_moved"]["found_fraction"] = round(float((c.read_temporal()[1] > SPP).mean()), 4)
    out["all_moved"]["finite_motion_fraction"] = round(float(np.isfinite(mv).all(axis=-1).mean()), 4)
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="1280x720,3840x2160")
    ap.add_argument("--scenes", default="C2,C5")
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm runtime in the process, as tests/conftest.py)
    for scene in a.scenes.split(","):
        out = {"scene": scene}
        for size in a.sizes.split(","):
            w, h = (int(x) for x in size.split("x"))
            out[size] = measure(scene, w, h)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
