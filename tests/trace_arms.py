"""Helper of tests/test_trace_arms_cpu.py and tests/test_gpu_trace_arms.py - no tests of its own: which scenes the GPU parity tests
render, under which trace kernel, and which arms of Trace (Oracle.render_census, oracle/pt_oracle.h ORC_ARM_*) each kernel can
reach at all.  A kernel is held to the oracle bit for bit only on the arms some scene drives it through: the census over this
registry is what says that every arm is driven."""
import glob
import os

import numpy as np

from conftest import GOLDEN, load_golden, scene_from_golden

VARIANTS = ("PLAIN", "FLAT", "BVH")
FLOOR = 32           # every reachable arm, per variant, at least this often: an arm met a handful of times in one wave proves little


def variant_of(arrays, cam=None) -> str:
    """the trace kernel a scene gets by the product's own rule: more than 16 triangles walk the tree, otherwise
    ptk_scene_is_plain decides between the PLAIN and the generic FLAT kernel (no device needed) - and the PLAIN kernel starts from
    the cached primary hits, which only a pinhole camera has: through a lens (cam["aperture"] != 0) a plain scene runs FLAT"""
    from pbrpathtracer_amd import ptk
    if len(arrays["verts"]) > 16:
        return "BVH"
    return "PLAIN" if ptk.scene_is_plain(arrays) and (cam is None or float(cam["aperture"]) == 0.0) else "FLAT"


def variants_admitted(arrays, cam=None):
    """every kernel a scene can be made to run on: "flat" 0 sends a small scene down the tree, "plain_kernel" 0 a plain one through
    the generic FLAT kernel"""
    v = variant_of(arrays, cam)
    return {"BVH": ("BVH",), "FLAT": ("FLAT", "BVH"), "PLAIN": ("PLAIN", "FLAT", "BVH")}[v]


def _golden_cam(z, aperture=None):
    cam, proj = z["cam"], z["proj"]
    return dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]), focal_dist=float(z["focal_dist"]),
                aperture=float(z["aperture"]) if aperture is None else aperture)


GOLDEN_FRAME = (64, 48, 8, 1234)                     # W, H, spp, seed of every golden entry


def golden_scenes():
    """(name, arrays, cam, W, H, D, spp, seed) of every tier_s_* / tier_f_* fixture that holds a camera, found by glob: once at the fixture's
    own aperture ("_lens") and once with none ("_pinhole"), at the fixture's depth.  tests/test_gpu_trace_arms.py renders exactly this
    list, each entry under every kernel it admits - so every scene on which a tape pins the oracle to the reference also holds the
    kernels to the oracle."""
    out = []
    W, H, spp, seed = GOLDEN_FRAME
    for path in sorted(glob.glob(os.path.join(GOLDEN, "tier_s_*.npz")) + glob.glob(os.path.join(GOLDEN, "tier_f_*.npz"))):
        z = load_golden(os.path.basename(path))
        if "cam" not in z.files:
            continue
        arrays = scene_from_golden(z)
        D = int(z["depth"]) if "depth" in z.files else 5
        name = os.path.basename(path)[:-4]
        out.append((name + "_lens", arrays, _golden_cam(z), W, H, D, spp, seed))
        out.append((name + "_pinhole", arrays, _golden_cam(z, 0.0), W, H, D, spp, seed))
    return out


def existing_scenes():
    """(name, arrays, cam, W, H, D, spp, seed, variants) of what the parity tests from before the census render, at their sizes, each
    under the kernel it gets by default - and the golden entries, each under every kernel it admits"""
    import test_gpu_edge_cases as EC
    import test_gpu_plain_frames as PF
    import test_gpu_random_scenes as RS
    out = []
    params = [m for m in RS.test_random_scene_matches_oracle.pytestmark if m.name == "parametrize"][0].args[1]
    for seed, n_tris, tex in params:
        if n_tris >= 6000:
            continue                                          # the floors are met without them; they take most of the time
        arrays, cam = RS.random_scene(seed, n_tris, tex)
        out.append((f"random_{seed}", arrays, cam, 56, 40, 7, 6, seed))
    params = [m for m in RS.test_grazing_light_hits_decide_shadow_rays_like_the_reference.pytestmark if m.name == "parametrize"][0].args[1]
    for seed, n_tris, tex, W, H, D in params:
        arrays, cam = RS.random_scene(seed, n_tris, tex)
        out.append((f"grazing_{seed}", arrays, cam, W, H, D, 4, seed))
    cams = {"open%d" % n: PF.open_plain_scene(seed, n)[1] for seed, n in PF.OPEN_SCENES}
    for name, arrays in PF.plain_scenes().items():
        out.append(("plain_frames_" + name, arrays, cams.get(name, PF.three_sampler_cornell()[1]), PF.W, PF.H, PF.D, PF.SPP, PF.SEED))
    a, cam = EC.no_lights_degenerate_scene()
    out.append(("no_lights_degenerate", a, cam, 48, 32, 6, 3, 5))
    z = load_golden("tier_s_cornell.npz")
    out.append(("empty", EC._empty_like(scene_from_golden(z)), EC._cam(z), 33, 17, 4, 3, 5))
    return [s + (variants_admitted(s[1], s[2]),) for s in golden_scenes()] + [s + ((variant_of(s[1], s[2]),),) for s in out]


# registry entry (by the prefix of its name) -> (test module, test function) that renders it.  tests/test_trace_arms_cpu.py checks every
# entry of the registry against that function's own parameter list, so a scene cannot stay registered after its test is gone.
RENDERED_BY = {
    "tier_s_": ("test_gpu_trace_arms", "test_golden_scene_renders"), "tier_f_": ("test_gpu_trace_arms", "test_golden_scene_renders"),
    "random_": ("test_gpu_random_scenes", "test_random_scene_matches_oracle"),
    "grazing_": ("test_gpu_random_scenes", "test_grazing_light_hits_decide_shadow_rays_like_the_reference"),
    "plain_frames_": ("test_gpu_plain_frames", "test_plain_equals_generic_equals_oracle"),
    "no_lights_degenerate": ("test_gpu_edge_cases", "test_no_lights_and_degenerate_triangles"),
    "empty": ("test_gpu_edge_cases", "test_empty_scene_renders_black"),
    "rr_cap_": ("test_gpu_trace_arms", "test_rr_cap_renders"), "tex_edges_": ("test_gpu_trace_arms", "test_tex_edges_renders"),
    "": ("test_gpu_trace_arms", "test_other_edge_scene_renders"),                  # every other edge scene, by its prefix there
}


def edge_scenes():
    """the scenes of tests/trace_edge_cases.py, each under every kernel it admits (tests/test_gpu_trace_arms.py renders them so)"""
    import trace_edge_cases as TE
    return [s + (variants_admitted(s[1], s[2]),) for s in TE.scenes()]


def registry():
    return existing_scenes() + edge_scenes()


# ---- which arms a kernel can reach -----------------------------------------------------------------------------------------------
NOWHERE = {
    "direct.light_id_clamped": "u01 is at most 1 - 2^-24 and nl * (1 - 2^-24) rounds to the float below nl, never to nl, for nl < 2^24 lights",
    "closest_hit.stack_guard": "the oracle's own tree is a median split, at most 32 deep for any nt an int32 counts; the walk holds one pending sibling per level, far below 128",
}
IN_INDEX_ORDER = {
    "test_triangle.tie_accepted_smaller_index": "the pass meets candidates in ascending index: at a tie the best so far has the smaller index",
}
_PLAIN_WHY = "a plain scene is untextured, opaque and unsmoothed (ptk_scene_is_plain)"


def _plain_unreachable(names):
    out = {}
    for n in names:
        if (n.startswith("tex2d.") or n.startswith("shade.glass.") or n.startswith("sample_about.glass_") or "_texel_" in n
                or n.startswith("test_triangle.opacity_") or n in ("shade.smoothing_on", "shade.normal_map_on", "shade.nt_z_clamped")):
            out[n] = _PLAIN_WHY
    return out


def unreachable(variant, names):
    """arm -> the one-line argument that no scene the upload accepts can take it under this kernel"""
    u = dict(NOWHERE)
    if variant in ("PLAIN", "FLAT"):
        u.update(IN_INDEX_ORDER)
    if variant == "PLAIN":
        u.update(_plain_unreachable(names))
    return u


def census(oracle_mod, scenes=None):
    """{variant: {arm: count}} summed over the registry, and the per-scene rows [(name, variant, {arm: count})]"""
    total = {v: {} for v in VARIANTS}; rows = []
    for name, arrays, cam, W, H, D, spp, seed, variants in (registry() if scenes is None else scenes):
        o = oracle_mod.Oracle(arrays)
        ocam = oracle_mod.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])
        done = {}
        for v in variants:
            brute = v != "BVH"                      # the FLAT and PLAIN passes take the candidates in index order
            if brute not in done:
                done[brute] = o.render_census(ocam, W, H, D, 0, spp, seed, brute=brute)
            rows.append((name, v, done[brute]))
            for k, c in done[brute].items():
                total[v][k] = total[v].get(k, 0) + c
        o.close()
    return total, rows


def format_table(total):
    names = list(total[VARIANTS[0]])
    w = max(len(n) for n in names)
    lines = [f"{'arm':<{w}} " + " ".join(f"{v:>9}" for v in VARIANTS)]
    for n in names:
        cells = []
        for v in VARIANTS:
            cells.append(f"{'-':>9}" if n in unreachable(v, names) and total[v][n] == 0 else f"{total[v][n]:>9}")
        lines.append(f"{n:<{w}} " + " ".join(cells))
    return "\n".join(lines)
