"""The PLAIN variant of the FLAT trace kernel (trace_kernel<false, true, true>, csrc/ptk_kernels.hip) and the host-side predicate
that selects it (csrc/ptk_api.hip plain_tables + the primary-hit cache; include/ptk.h "plain_kernel", ptk_trace_variant,
ptk_scene_is_plain).

The variant is the generic FLAT kernel with everything a plain scene cannot reach compiled out, so its images must be the
generic kernel's bit for bit: every comparison here is np.array_equal, float accumulator and RGB8, no tolerance.  The one way
the change can produce wrong pixels is a predicate that has gone stale after an edit, so each of its five conditions is broken
and restored through the public API, with the oracle as the judge after every step."""
import numpy as np
import pytest

from conftest import load_golden, scene_from_golden

gpu = pytest.mark.gpu


def _cam_from_golden(z):
    cam = z["cam"]; proj = z["proj"]
    return dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]),
                focal_dist=float(z["focal_dist"]), aperture=float(z["aperture"]))


def _oracle(OB, arrays, cam, W, H, D, spp, seed):
    o = OB.Oracle(arrays)
    ocam = OB.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])
    tot, rgb = o.render(ocam, W, H, D, 0, spp, seed)
    o.close()
    return tot, rgb


def _render(ctx, spp, seed):
    ctx.reset()
    ctx.render(0, spp, seed)
    return ctx.read_accum(), ctx.resolve_rgb8(), ctx.trace_variant()


def _config(cfg, tmp_path):
    """scene arrays, camera, frame and sample count of a bench.py config, at its full size"""
    from pbrpathtracer_amd import scenes as S
    from pbrpathtracer_amd.pathtracer import PathTracer, camera_from_scene
    pts, scene, spp = S.build_config(cfg, str(tmp_path))
    pt = PathTracer(0); pt.LoadSceneFile(pts)
    arrays = pt.StagedScene()
    W, H = pt.GetResolution(); D = pt.GetTraceDepth()
    pt.close()
    cam = camera_from_scene(scene)
    cam["aperture"] = 0.0                       # as bench.py renders the pinhole configs
    return arrays, cam, W, H, D, spp


@gpu
@pytest.mark.parametrize("cfg", ["C1", "C2"])
def test_plain_equals_generic_equals_oracle_at_full_size(tmp_path, oracle_mod, cfg):
    from pbrpathtracer_amd import ptk
    arrays, cam, W, H, D, spp = _config(cfg, tmp_path)
    assert len(arrays["verts"]) <= 16 and ptk.scene_is_plain(arrays)
    ctx = ptk.Context(0)
    try:
        ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, D)
        acc_p, rgb_p, var_p = _render(ctx, spp, 33)
        ctx.set_option("plain_kernel", 0)
        acc_g, rgb_g, var_g = _render(ctx, spp, 33)
        ctx.set_option("plain_kernel", 1)
        acc_p2, _, var_p2 = _render(ctx, spp, 33)
    finally:
        ctx.close()
    assert (var_p, var_g, var_p2) == (ptk.TRACE_FLAT_PLAIN, ptk.TRACE_FLAT, ptk.TRACE_FLAT_PLAIN)
    ref, ref8 = _oracle(oracle_mod, arrays, cam, W, H, D, spp, 33)
    assert (ref != 0).any()
    assert np.array_equal(acc_p, acc_g) and np.array_equal(rgb_p, rgb_g)
    assert np.array_equal(acc_p, ref) and np.array_equal(rgb_p, ref8)
    assert np.array_equal(acc_p2, ref)


@gpu
@pytest.mark.parametrize("cfg", ["C1", "C2"])
def test_contracted_plain_reproduces_contracted_generic(tmp_path, cfg):
    """contract = 2 is a recompilation of the same file: reproducible, so its PLAIN variant must reproduce its generic one."""
    from pbrpathtracer_amd import ptk
    arrays, cam, W, H, D, spp = _config(cfg, tmp_path)
    ctx = ptk.Context(0)
    try:
        ctx.set_option("contract", 2)
        ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, D)
        acc_p, rgb_p, var_p = _render(ctx, spp, 33)
        ctx.set_option("plain_kernel", 0)
        acc_g, rgb_g, var_g = _render(ctx, spp, 33)
    finally:
        ctx.close()
    assert (var_p, var_g) == (ptk.TRACE_FLAT_PLAIN, ptk.TRACE_FLAT)
    assert (acc_p != 0).any()
    assert np.array_equal(acc_p, acc_g) and np.array_equal(rgb_p, rgb_g)


# ---- the five conditions of the predicate, each broken by one edit of the 12-triangle Cornell box ----------------------------
def _base():
    z = load_golden("tier_s_cornell.npz")
    a = {k: np.array(v) for k, v in scene_from_golden(z).items()}
    # uvs and vertex normals that make a texture / a smoothed normal visible once an edit switches them on
    rs = np.random.RandomState(5)
    a["uvs"] = rs.rand(len(a["verts"]), 6).astype(np.float32)
    n = a["normals"].reshape(-1, 3, 3) + rs.uniform(-0.3, 0.3, (len(a["verts"]), 3, 3)).astype(np.float32)
    a["normals"] = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32).reshape(-1, 9)
    cam = _cam_from_golden(z)
    cam["aperture"] = 0.0                       # a pinhole: the primary-hit cache is on
    return a, cam, int(z["depth"])


def _with_texture(a, slot):
    from pbrpathtracer_amd import ptk
    b = dict(a)
    rs = np.random.RandomState(9)
    b["texels"] = rs.randint(0, 256, 16 * 16 * 4).astype(np.uint8)
    b["textures"] = np.array([(16, 16, 0)], dtype=ptk.TEXTURE_DTYPE)
    b["materials"] = a["materials"].copy()
    b["materials"]["tex"][0, slot] = 0
    return b


def _edit_glass(a, cam):
    b = dict(a); b["materials"] = a["materials"].copy()
    b["materials"]["type"][1] = 1; b["materials"]["translucency"][1] = 0.8; b["materials"]["roughness"][1] = 0.3
    return b, cam, "materials"


def _edit_texture(a, cam):
    return _with_texture(a, 0), cam, "upload"


def _edit_smoothing(a, cam):
    b = dict(a); b["smoothing"] = a["smoothing"].copy(); b["smoothing"][4] = 1
    return b, cam, "upload"


def _edit_opacity(a, cam):
    return _with_texture(a, 5), cam, "upload"


def _edit_aperture(a, cam):
    c = dict(cam); c["aperture"] = 0.05
    return a, c, "camera"


EDITS = {"glass": _edit_glass, "texture": _edit_texture, "smoothing": _edit_smoothing, "opacity": _edit_opacity, "aperture": _edit_aperture}


def _apply(ctx, arrays, cam, how):
    if how == "materials": ctx.update_materials(arrays["materials"])
    elif how == "upload": ctx.upload_scene(arrays)
    else: ctx.set_camera(**cam)


@gpu
@pytest.mark.parametrize("edit", sorted(EDITS))
def test_predicate_follows_every_edit_and_its_undo(oracle_mod, edit):
    from pbrpathtracer_amd import ptk
    W, H, spp, seed = 64, 48, 8, 77
    base, cam, D = _base()
    edited, ecam, how = EDITS[edit](base, cam)
    assert ptk.scene_is_plain(base)
    ref_base = _oracle(oracle_mod, base, cam, W, H, D, spp, seed)
    ref_edit = _oracle(oracle_mod, edited, ecam, W, H, D, spp, seed)
    assert not np.array_equal(ref_base[0], ref_edit[0])            # the edit is one the image shows
    ctx = ptk.Context(0)
    try:
        ctx.upload_scene(base); ctx.set_camera(**cam); ctx.set_frame(W, H, D)
        for arrays, c, ref, want in ((None, None, ref_base, ptk.TRACE_FLAT_PLAIN), (edited, ecam, ref_edit, ptk.TRACE_FLAT),
                                     (base, cam, ref_base, ptk.TRACE_FLAT_PLAIN)):
            if arrays is not None: _apply(ctx, arrays, c, how)
            acc, rgb, var = _render(ctx, spp, seed)
            assert var == want
            assert np.array_equal(acc, ref[0]) and np.array_equal(rgb, ref[1])
    finally:
        ctx.close()


# ---- the table half of the predicate needs no device ---------------------------------------------------------------------------
def test_scene_is_plain_on_staged_tables():
    from pbrpathtracer_amd import ptk
    base, cam, _ = _base()
    assert ptk.scene_is_plain(base)
    for name in ("glass", "texture", "smoothing", "opacity"):
        assert not ptk.scene_is_plain(EDITS[name](base, cam)[0]), name
    for slot in range(1, 5):                                       # each of the five shading slots
        assert not ptk.scene_is_plain(_with_texture(base, slot))
    # fields the PLAIN route reads may hold anything: a mirror-like, emissive, rough material is still plain
    b = dict(base); b["materials"] = base["materials"].copy()
    b["materials"]["reflectiveness"][2] = 0.7; b["materials"]["roughness"][2] = 0.4; b["materials"]["emissive_intensity"][2] = 3.0
    assert ptk.scene_is_plain(b)
    # a glass material that no triangle uses still breaks it ("every material"), as does a 17th triangle, as does no triangle
    b = dict(base); b["materials"] = np.concatenate([base["materials"], base["materials"][:1]]); b["materials"]["type"][-1] = 1
    assert not ptk.scene_is_plain(b)
    big = {k: (np.concatenate([v, v[:5]]) if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material") else v) for k, v in base.items()}
    assert len(big["verts"]) == 17 and not ptk.scene_is_plain(big)
    sixteen = {k: (np.concatenate([v, v[:4]]) if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material") else v) for k, v in base.items()}
    assert len(sixteen["verts"]) == 16 and ptk.scene_is_plain(sixteen)
    empty = {k: (v[:0] if k in ("verts", "normals", "uvs", "tbn", "smoothing", "material", "lights") else v) for k, v in base.items()}
    assert not ptk.scene_is_plain(empty)
    assert not ptk.scene_is_plain(scene_from_golden(load_golden("tier_s_glass.npz")))
