"""The counters of the STATS trace kernels (ptk_collect_stats) against the oracle's counts (Oracle.render_counted) - exactly where
the counter is a function of the paths, within per-ray bounds (tests/stats_bounds.py) where it depends on the order the walk
tests boxes and triangles in - plus the relations between the SIMD-utilisation counters, and independence of how the work is
launched.  include/ptk.h (ptk_stats) defines every counter; DESIGN.md §5 lists which are pinned how."""
import numpy as np
import pytest

import stats_bounds as SB
from conftest import load_golden, scene_from_golden
from oracle import oracle_binding as OB
from test_gpu_random_scenes import random_scene

pytestmark = pytest.mark.gpu

EXACT = ("paths_started", "rays", "shadow_rays", "hits_shaded")
UTIL = (("walk_wave_iters", "walk_lane_iters"), ("shade_wave_execs", "shade_lanes"), ("gen_wave_execs", "gen_lanes"),
        ("tri_wave_execs", "tri_lanes"))
# test_work_distribution_modes_agree's option sets
DEFAULTS = {"persistent": -1, "generations": 0, "max_batch": 1, "chunk": 0, "tri_threshold": 6}
MODES = ({"persistent": 1}, {"persistent": 0}, {"persistent": 1, "max_batch": 7}, {"persistent": 1, "generations": 3, "chunk": 2},
         {"persistent": 1, "chunk": 24}, {"persistent": 0, "chunk": 3}, {"persistent": 1, "tri_threshold": 0},
         {"persistent": 1, "tri_threshold": 64})


def _golden(name):
    z = load_golden(name)
    cam, proj = z["cam"], z["proj"]
    return scene_from_golden(z), dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]),
                                      focal_dist=float(z["focal_dist"]), aperture=float(z["aperture"]))


def _c4(tmp):
    from pbrpathtracer_amd import scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer, camera_from_scene
    pts, scene, _ = S.build_config("C4", tmp, width=96, height=54, grid=20)
    pt = PathTracer(0)
    pt.LoadSceneFile(pts)
    arrays = pt.StagedScene()
    pt.close()
    return arrays, camera_from_scene(scene)


class Expect:
    """The oracle's counts and ray records of one camera, and the walk bounds of the tree the context holds."""

    def __init__(self, ctx, o, arrays, cam, W, H, D, spp, seed, flat):
        self.ocam = OB.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"],
                                   normalise=True)
        r = o.render_counted(self.ocam, W, H, D, 0, spp, seed, dump=True)
        self.total = r["total"]
        c = r["counts"].reshape(W * H, -1)
        self.c = c
        self.rays = r["rays"]
        self.n_tris = len(arrays["verts"])
        self.flat = flat
        self.spp = spp
        self.samples = W * H * spp
        # pixels every path of which is one camera ray that misses: the only ones the kernels may leave out
        self.all_miss = (c[:, 1] == c[:, 0]) & (c[:, 2] == 0) & (c[:, 3] == 0) & (c[:, 4] == 0)
        self.miss_px = int(self.all_miss.sum())
        self.opacity = (arrays["materials"]["tex"][:, 5] >= 0)[arrays["material"]]
        self.tex_shade = int(c[:, 5].sum())
        self.tex_opacity = int(c[:, 6].sum())
        if not flat:
            nodes, order = ctx.download_bvh()
            self.b = SB.ray_bounds(nodes, order, np.ascontiguousarray(arrays["verts"], np.float32), self.rays,
                                   self.opacity if self.opacity.any() else None, OB.intersect_many)

    def check(self, st, cached, label):
        """All assertions on one ptk_stats; cached: the pinhole primary-hit cache is in effect."""
        e, c = self, self.c
        assert st["samples"] == e.samples, label
        if cached:
            # the cache resolves every camera ray (primary_hits_kernel) and deals only the pixels whose camera ray hits
            paths = int(c[~e.all_miss, 0].sum())
            culled = 0                  # (no camera ray is walked at all)
            walked_camera = 0
        else:
            culled = e.samples - st["paths_started"]
            assert culled >= 0 and culled % e.spp == 0 and culled // e.spp <= e.miss_px, (label, culled, e.miss_px)
            paths = e.samples - culled
            walked_camera = e.samples - culled
        assert st["paths_started"] == paths, (label, st["paths_started"], paths)
        rays = int(c[:, 2:4].sum()) + walked_camera
        assert st["rays"] == rays, (label, st["rays"], rays)
        assert st["shadow_rays"] == int(c[:, 3].sum()), label
        assert st["hits_shaded"] == int(c[:, 4].sum()), label
        if e.flat or not e.opacity.any():
            assert st["tex_fetches"] == e.tex_shade + e.tex_opacity, (label, st["tex_fetches"], e.tex_shade, e.tex_opacity)
        # utilisation counters
        for execs, lanes in UTIL:
            assert st[lanes] <= 64 * st[execs], (label, lanes)
        assert st["shade_lanes"] == st["hits_shaded"], label
        assert st["gen_lanes"] == (0 if cached else st["paths_started"]), label
        if e.flat:
            assert st["node_visits"] == 0 and st["max_walk_nodes"] == 0, label
            assert st["tri_tests"] == st["rays"] * e.n_tris, (label, st["tri_tests"], st["rays"], e.n_tris)
            # one pass per bounce (or camera) ray of a lane, its shadow ray riding along
            assert st["walk_lane_iters"] == st["rays"] - st["shadow_rays"], label
            assert st["tri_wave_execs"] == 0 and st["tri_lanes"] == 0, label
            return
        assert st["node_visits"] <= st["walk_lane_iters"], label
        assert st["tri_lanes"] <= st["tri_tests"] - st["shadow_rays"] <= 2 * st["tri_lanes"], label
        # bounds: every ray the kernel walked; with an uncached camera `culled` camera rays of all-miss pixels were not walked
        b, kind = e.b, e.rays["kind"]
        walked = np.ones(len(kind), bool) if not cached else kind != OB.RAY_CAMERA
        miss_cam = (kind == OB.RAY_CAMERA) & e.all_miss[e.rays["pixel"]]
        certain = walked & ~miss_cam
        for name, lo, hi in (("node_visits", b["node_lo"], b["node_hi"]), ("tri_tests", b["tri_lo"], b["tri_hi"])):
            s_lo = int(lo[walked].sum()) - (culled and culled * int(lo[miss_cam].max()))
            s_hi = int(hi[walked].sum()) - (culled and culled * int(hi[miss_cam].min()))
            assert s_lo <= st[name] <= s_hi, (label, name, s_lo, st[name], s_hi)
        assert int(b["node_lo"][certain].max()) <= st["max_walk_nodes"] <= int(b["node_hi"][walked].max()), \
            (label, int(b["node_lo"][certain].max()), st["max_walk_nodes"], int(b["node_hi"][walked].max()))
        if e.opacity.any():
            opa = st["tex_fetches"] - e.tex_shade
            o_lo = int(b["opa_lo"][walked].sum()) - (culled and culled * int(b["opa_lo"][miss_cam].max()))
            o_hi = int(b["opa_hi"][walked].sum()) - (culled and culled * int(b["opa_hi"][miss_cam].min()))
            assert o_lo <= opa <= o_hi, (label, o_lo, opa, o_hi)


def _setup(ctx, arrays, cam, W, H, D, aperture):
    cam = dict(cam, aperture=aperture)
    ctx.set_camera(**cam)
    ctx.set_frame(W, H, D)
    ctx.set_tile(0, 1)
    return cam


def _exact(st):
    return {k: st[k] for k in EXACT}


def _run_case(arrays, cam, W, H, D, spp, seed, sweep=True):
    """Pinhole with the primary-hit cache on and off, thin lens with the lens cull on and off (trees of >= 4096 triangles are
    built on the GPU, smaller ones by the host builder); sweep: the launch-configuration checks too."""
    from pbrpathtracer_amd import ptk
    ctx = ptk.Context(0)
    o = OB.Oracle(arrays)
    try:
        ctx.upload_scene(arrays)
        n = len(arrays["verts"])
        flat = n <= 16
        has_opacity = bool((arrays["materials"]["tex"][:, 5] >= 0)[arrays["material"]].any())
        lens = cam["aperture"] if cam["aperture"] != 0.0 else 0.05
        for aperture in (0.0, lens):
            cam_a = _setup(ctx, arrays, cam, W, H, D, aperture)
            e = Expect(ctx, o, arrays, cam_a, W, H, D, spp, seed, flat)
            # the setup itself: the kernels render the oracle's accumulator
            ctx.reset(); ctx.render(0, spp, seed)
            assert np.array_equal(ctx.read_accum(), e.total), ("setup", aperture)
            option = "primary_cache" if aperture == 0.0 else "lens_cull"
            for on in (1, 0):
                ctx.set_option(option, on)
                cached = aperture == 0.0 and on == 1 and not has_opacity
                label = f"{n} triangles, aperture {aperture}, {option} {on}"
                st = ctx.collect_stats(0, spp, seed)
                e.check(st, cached, label)
                if not sweep or on == 0:
                    continue
                ref = _exact(st)
                if flat or not has_opacity:
                    ref["tex_fetches"] = st["tex_fetches"]
                if flat:
                    ref["tri_tests"] = st["tri_tests"]
                # launch configuration changes no exact counter and keeps the bounded ones in their bounds
                for opts in MODES:
                    for k, v in {**DEFAULTS, **opts}.items():
                        ctx.set_option(k, v)
                    s2 = ctx.collect_stats(0, spp, seed)
                    e.check(s2, cached, f"{label} {opts}")
                    assert {k: s2[k] for k in ref} == ref, (label, opts)
                for k, v in DEFAULTS.items():
                    ctx.set_option(k, v)
                # several passes: the smallest budget (1 MiB) holds 42 samples of this frame, so 96 samples take three passes
                tiles = ((W + 15) // 16) * ((H + 15) // 16)
                assert 2 ** 20 // (tiles * 4 * 64 * 16) < 48
                one = ctx.collect_stats(0, 96, seed)
                ctx.set_option("pass_bytes", 2 ** 20)
                several = ctx.collect_stats(0, 96, seed)
                ctx.set_option("pass_bytes", 16 * 2 ** 30)
                assert {k: several[k] for k in ref} == {k: one[k] for k in ref}, (label, "pass_bytes")
                # sample ranges and tile shares add up
                h = spp // 2
                a, b = ctx.collect_stats(0, h, seed), ctx.collect_stats(h, spp - h, seed)
                assert {k: a[k] + b[k] for k in ref} == ref, (label, "sample ranges")
                parts = []
                for r in range(3):
                    ctx.set_tile(r, 3)
                    parts.append(ctx.collect_stats(0, spp, seed))
                ctx.set_tile(0, 1)
                assert {k: sum(p[k] for p in parts) for k in ref} == ref, (label, "tiles")
                assert sum(p["samples"] for p in parts) == st["samples"]
                if not flat:
                    e.check(dict(st, **{k: sum(p[k] for p in parts) for k in ("node_visits", "tri_tests", "tex_fetches")}),
                            cached, f"{label} tiles")
    finally:
        o.close()
        ctx.close()


W, H, D, SPP = 48, 32, 6, 4


@pytest.mark.parametrize("seed,n,tex", [(11, 9, False), (12, 16, True), (14, 300, True), (15, 300, False), (16, 6000, True),
                                        (17, 6000, False)])
def test_counters_on_random_scenes(seed, n, tex):
    arrays, cam = random_scene(seed, n, tex)
    _run_case(arrays, cam, W, H, D, SPP, seed, sweep=n in (12, 14, 16, 17))


@pytest.mark.parametrize("name", ["tier_s_cornell.npz", "tier_s_opacity.npz", "tier_s_glass.npz"])
def test_counters_on_tier_s_scenes(name):
    arrays, cam = _golden(name)
    _run_case(arrays, cam, W, H, 5, SPP, 29, sweep=name != "tier_s_cornell.npz")


def test_counters_on_c4(tmp_path):
    arrays, cam = _c4(str(tmp_path))
    _run_case(arrays, cam, 96, 54, 5, 3, 21, sweep=False)
