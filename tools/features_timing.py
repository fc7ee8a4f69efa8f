"""Launch times of features_kernel (include/ptk.h ptk_render_features) beside primary_hits_kernel, from one kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/features_timing.py --config C4 [--reps 8]
    python3 tools/features_timing.py --parse OUT

The run repeats, at the config's full frame:  set_camera (invalidates the primary-hit cache);  primary_cache 1 + full mask
(primary_hits_kernel, then features_kernel taking its hits from the cache);  primary_cache 0 + full mask (features_kernel walks);
primary_cache 0 + TRIANGLE | DEPTH (walks, two plane stores).  --parse reads the trace, puts the features_kernel launches into
those three groups by their order and prints median, min and max of each group and of primary_hits_kernel as one JSON line."""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(config: str, reps: int):
    from pbrpathtracer_amd import ptk, scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer, camera_from_scene
    pts, scene, _ = S.build_config(config, tempfile.mkdtemp(prefix="feat_"))
    pt = PathTracer(0); pt.LoadSceneFile(pts); pt.SetCameraAperture(0.0)
    pt.RenderFeatures(ptk.FEAT_ALL)                      # stages camera and frame, allocates the planes
    if pt.LastError():
        raise SystemExit(pt.LastError())
    c = pt.context()
    cam = dict(camera_from_scene(scene), aperture=0.0)
    hit_only = (1 << ptk.FEAT_TRIANGLE) | (1 << ptk.FEAT_DEPTH)
    c.render_features(hit_only); c.synchronize()
    for _ in range(reps):
        c.set_camera(**cam)
        c.set_option("primary_cache", 1); c.render_features(ptk.FEAT_ALL)
        c.set_option("primary_cache", 0); c.render_features(ptk.FEAT_ALL); c.render_features(hit_only)
        c.synchronize()
    w, h = pt.GetResolution()
    print(json.dumps(dict(config=config, width=w, height=h, triangles=pt.GetTriangleCount(), reps=reps)))
    pt.close()


def parse(d: str):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    feat = [us(r) for r in rows if "features_kernel" in r["Kernel_Name"]][2:]          # (the two launches before the loop)
    prim = [us(r) for r in rows if "primary_hits_kernel" in r["Kernel_Name"]][1:]
    assert len(feat) % 3 == 0 and len(feat) // 3 == len(prim), (len(feat), len(prim))

    def stat(x):
        x = sorted(x)
        return dict(median_us=round(x[len(x) // 2], 2), min_us=round(x[0], 2), max_us=round(x[-1], 2), n=len(x))
    print(json.dumps(dict(primary_hits_kernel=stat(prim), features_cached_full_mask=stat(feat[0::3]),
                          features_walk_full_mask=stat(feat[1::3]), features_walk_hit_only=stat(feat[2::3]))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="C2")
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--parse", default=None)
    a = ap.parse_args()
    parse(a.parse) if a.parse else run(a.config, a.reps)
