#!/usr/bin/env python3
"""Measures geometry updates (ptk_update_geometry) against a new upload on C4 and C5 - not a test, bench.py is untouched.

For each config: the update split into staging copies + bounds / record repack / refit (HIP events, ptk_geometry_timing) and its
wall time to synchronize, the wall time of ptk_upload_scene of the same arrays, and - after a per-vertex jitter and after a
non-uniform scale - sah_now / sah_built (ptk_geometry_info) and node visits per sample (ptk_collect_stats) of the refitted
tree beside those of a tree rebuilt from the moved arrays.  One JSON line per config.

    python tools/refit_timing.py [C4 C5]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (one ROCm runtime in the process, as tests/conftest.py)

from pbrpathtracer_amd import scenes as S  # noqa: E402
from pbrpathtracer_amd.pathtracer import PathTracer  # noqa: E402

REPS = 5


def med(xs):
    return round(float(np.median(xs)), 4)


def visits(c, spp=2):
    st = c.collect_stats(0, spp, 7)
    return round(st["node_visits"] / st["samples"], 3), round(st["tri_tests"] / st["samples"], 3)


def measure(name):
    tmp = tempfile.mkdtemp(prefix="refit_")
    pts, scene, _ = S.build_config(name, tmp, width=960, height=540)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    pt.SetCameraAperture(0.0)
    pt.RenderFrames(1)
    arrays = pt.StagedScene()
    c = pt.context()
    n = len(arrays["verts"])
    rng = np.random.default_rng(1)
    size = float(np.abs(arrays["verts"]).max())
    motions = {
        "jitter": (arrays["verts"] + rng.normal(0, 0.002 * size, arrays["verts"].shape)).astype(np.float32),
        "scale": (arrays["verts"] * np.tile(np.array([1.3, 0.8, 1.1], np.float32), 3)).astype(np.float32),
    }
    out = {"config": name, "triangles": n, "nodes": c.bvh_info()[0], "levels": c.bvh_info()[1]}
    c.update_geometry(0, arrays["verts"]); c.synchronize()          # the first update's tables
    wall, parts = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        c.update_geometry(0, arrays["verts"], arrays["normals"], arrays["tbn"]); c.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        parts.append(c.geometry_timing())
    out["update_ms"] = {"wall": med(wall), **{k: med([p[k] for p in parts]) for k in parts[0]}}
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        c.update_geometry(0, arrays["verts"]); c.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    out["update_verts_only_ms"] = med(wall)
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter(); c.upload_scene(arrays); c.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
    out["upload_ms"] = {"wall": med(wall), **c.upload_timing()}
    out["built"] = dict(zip(("node_visits", "tri_tests"), visits(c)))
    for kind, v in motions.items():
        c.upload_scene(arrays)
        c.update_geometry(0, v)
        gi = c.geometry_info()
        r = {"sah_ratio": round(gi["sah_now"] / gi["sah_built"], 4)}
        r["refitted"] = dict(zip(("node_visits", "tri_tests"), visits(c)))
        moved = dict(arrays); moved["verts"] = v
        c.upload_scene(moved)
        r["rebuilt"] = dict(zip(("node_visits", "tri_tests"), visits(c)))
        out[kind] = r
    pt.close()
    return out


if __name__ == "__main__":
    for cfg in (sys.argv[1:] or ["C4", "C5"]):
        print(json.dumps(measure(cfg)), flush=True)
