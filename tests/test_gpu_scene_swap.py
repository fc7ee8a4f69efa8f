"""A context that changes scenes against a fresh context, entry by entry (include/ptk.h ptk_upload_scene).

Context X is given scene A and used until every lazily made piece of state exists for A; then it is given scene B, with no wait in
between.  Context Y only ever sees B.  Everything the ray, point, region, surface, bake, probe, frame and geometry-update entries
answer must then be the same on X and Y, bit for bit - float arrays compared byte by byte, so that NaN payloads and signed zeros
count - and the render must also be the CPU oracle's of B.  The pairs A -> B (tests/scene_swap_cases.py) cross every boundary at
which an upload switches representation, in both directions.  Then: the frame state an upload drops and keeps; uploads behind work
in flight; and uploads that are refused, which must leave the resident scene exactly as it was."""
import ctypes as C
import struct

import numpy as np
import pytest

import scene_swap_cases as SC

pytestmark = pytest.mark.gpu
F32 = np.float32
BAD_ARG, LIMIT = -1, -4            # PTK_ERR_BAD_ARG, PTK_ERR_LIMIT
W, H, DEPTH, SPP, SEED = SC.W, SC.H, SC.DEPTH, SC.SPP, SC.SEED
GW, GH = 96, 64                    # the guide planes' resolution

_ref = {}


def cached(key, make):
    """a reference, computed once; shared, not to be modified"""
    if key not in _ref:
        _ref[key] = make()
    return _ref[key]


def oracle_render(oracle_mod, key, arrays, cam):
    def make():
        o = oracle_mod.Oracle(arrays)
        ocam = oracle_mod.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])
        out = o.render(ocam, W, H, DEPTH, 0, SPP, SEED)
        o.close()
        return out
    return cached(("oracle", key), make)


def new_context():
    from pbrpathtracer_amd import ptk
    return ptk.Context(0)


def stage(ctx, name, upload=True):
    arrays, cam = SC.scene(name)
    if upload:
        ctx.upload_scene(arrays)
    ctx.set_camera(**cam); ctx.set_frame(W, H, DEPTH); ctx.set_tile(0, 1); ctx.reset()


def params(name):
    from pbrpathtracer_amd import ptk
    e = SC.extent(SC.scene(name)[0])
    return dict(temporal=ptk.temporal_defaults(e), variance=ptk.variance_defaults(e), denoise=ptk.denoise_defaults(e), upsample=ptk.upsample_defaults(e),
                display=ptk.display_defaults())


def same_bits(a, b):
    """bitwise equality of answers: arrays by dtype, shape and bytes, floats by their eight bytes, containers element by element"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and \
            np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, float) and isinstance(b, float):
        return struct.pack("d", a) == struct.pack("d", b)
    return type(a) is type(b) and a == b


def differing(x, y):
    assert list(x) == list(y), (list(x), list(y))
    return [k for k in x if not same_bits(x[k], y[k])]


class Refused:
    """a call that answered PtkError: equal to another refusal with the same words"""

    def __init__(self, err):
        self.text = str(err)

    def __eq__(self, other):
        return isinstance(other, Refused) and self.text == other.text

    def __repr__(self):
        return "Refused(%r)" % self.text


def ask(fn, may_refuse):
    from pbrpathtracer_amd import ptk
    try:
        return fn()
    except ptk.PtkError as e:
        if not may_refuse:
            raise
        return Refused(e)


# ---- what a context is made to hold for scene A ------------------------------------------------------------------------------------
def exercise(ctx, name):
    """every lazily made piece of state, warm for the scene `name` (already staged)"""
    from pbrpathtracer_amd import ptk
    arrays, cam = SC.scene(name)
    n = len(arrays["verts"])
    soft = n == 0                                # the empty scene may refuse an entry; a scene with triangles may not
    prm, q = params(name), SC.queries(name)
    ctx.render(0, SPP, SEED)
    for fn in (lambda: ctx.render_adaptive(0.05, 2, 2, 6, SEED),
               lambda: (ctx.reset(), ctx.render(0, SPP, SEED)),
               lambda: ctx.render_features(ptk.FEAT_ALL, 0, SEED),
               lambda: ctx.render_guides(GW, GH, seed=SEED),
               lambda: ctx.temporal_frame(prm["temporal"], seed=SEED, moments=True),
               lambda: ctx.temporal_frame(prm["temporal"], seed=SEED, moments=True),
               lambda: ctx.temporal_variance(prm["variance"]),
               lambda: ctx.denoise_frame(prm["denoise"], render_features=False),       # (the moments call's planes hold its guides)
               lambda: ctx.display_frame(ptk.DISPLAY_ACCUM, prm["display"]),
               lambda: ctx.upsample_frame(ptk.UPSAMPLE_ACCUM, prm["upsample"]),
               ctx.snapshot_geometry):
        ask(fn, soft)
    if n:
        k = min(n, 5)
        ctx.update_geometry(0, SC.moved(arrays, k))
        # (with moments: a moments call behind a plain one starts over by itself, and the history left here has to be one that the
        # first call for the next scene would take)
        ctx.temporal_frame(prm["temporal"], seed=SEED, moving=True, moments=True)
        ctx.set_surface_weights(np.linspace(0.5, 2.0, n).astype(F32))
    ask(lambda: ctx.sample_surface(64, SEED), soft)
    pos, dirs = SC.probes(name)
    for fn in (lambda: ctx.trace_rays(q["ro"], q["rd"], DEPTH, 0, 1, SEED),
               lambda: ctx.intersect_rays(q["ro"], q["rd"], 0, SEED),
               lambda: ctx.occluded_rays(q["ro"], q["rd"], q["tmax"], 0, SEED),
               lambda: ctx.crossings_rays(q["ro"], q["rd"], q["tmax"]),
               lambda: ctx.contains_points(q["pts"]),
               lambda: ctx.signed_distance(q["pts"], q["max_dist"]),
               lambda: ctx.multihit_rays(q["ro"], q["rd"], 4, q["tmax"]),
               lambda: ctx.closest_points(q["pts"], q["max_dist"]),
               lambda: ctx.nearest_triangles(q["pts"], 4, q["max_dist"]),
               lambda: ctx.overlap_boxes(q["box_lo"], q["box_hi"], 4),
               lambda: ctx.overlap_spheres(q["pts"], q["radius"], 4),
               lambda: ctx.bake_lightmap(16, 16, 1e-3, DEPTH, 0, 1, SEED),
               lambda: ctx.bake_probes(pos, dirs, DEPTH, 0, 1, SEED, 0.785398),
               lambda: ctx.bake_probe_visibility(pos, dirs, 4, 2.0, 0, SEED),
               lambda: ctx.pick(24, 16, SEED)):
        ask(fn, soft)


# ---- what a context answers for scene B ----------------------------------------------------------------------------------------------
def answers(ctx, name, arrays=None):
    """name -> answer of every entry for the scene `name`, staged and reset on this context; the render is left in the accumulator"""
    from pbrpathtracer_amd import ptk
    arrays = SC.scene(name)[0] if arrays is None else arrays
    n = len(arrays["verts"])
    soft = n == 0
    q = SC.queries(name)
    pos, dirs = SC.probes(name)
    out = {}
    out["adaptive"] = ask(lambda: ctx.render_adaptive(0.05, 2, 2, 6, SEED), soft)
    out["adaptive counts"] = ask(ctx.read_sample_counts, soft); out["adaptive moments"] = ask(ctx.read_moments, soft)
    out["adaptive accum"] = ctx.read_accum()
    ctx.reset()
    ctx.render(0, SPP, SEED)
    out["accum"] = ctx.read_accum(); out["rgb8"] = ctx.resolve_rgb8(); out["samples"] = ctx.samples()
    out["trace"] = (ctx.trace_variant(), ctx.trace_unit(), ctx.trace_is_lambert())
    out["flat_classes"] = ask(ctx.flat_classes, True); out["flat_rect_pairs"] = ask(ctx.flat_rect_pairs, True)
    out["bvh_info"] = ctx.bvh_info(); out["bvh_layout"] = ctx.bvh_layout()
    ctx.render_features(ptk.FEAT_ALL, 0, SEED)
    for k, nm in enumerate(ptk.FEAT_NAMES):
        out["feature " + nm] = ctx.read_feature(k)
    out["pick"] = [ctx.pick(x, y, SEED) for x, y in SC.PICKS]
    out["trace_rays"] = ask(lambda: ctx.trace_rays(q["ro"], q["rd"], DEPTH, 0, 2, SEED), soft)
    out["intersect"] = ask(lambda: ctx.intersect_rays(q["ro"], q["rd"], 0, SEED), soft)
    out["occluded"] = ask(lambda: ctx.occluded_rays(q["ro"], q["rd"], q["tmax"], 0, SEED), soft)
    out["crossings"] = ask(lambda: ctx.crossings_rays(q["ro"], q["rd"], q["tmax"]), soft)
    out["contains"] = ask(lambda: ctx.contains_points(q["pts"], want_winding=True), soft)
    out["signed_distance"] = ask(lambda: ctx.signed_distance(q["pts"], q["max_dist"]), soft)
    out["multihit"] = ask(lambda: ctx.multihit_rays(q["ro"], q["rd"], 4, q["tmax"]), soft)
    out["closest"] = ask(lambda: ctx.closest_points(q["pts"], q["max_dist"]), soft)
    out["nearest"] = ask(lambda: ctx.nearest_triangles(q["pts"], 4, q["max_dist"]), soft)
    out["overlap_boxes"] = ask(lambda: ctx.overlap_boxes(q["box_lo"], q["box_hi"], 4), soft)
    out["overlap_spheres"] = ask(lambda: ctx.overlap_spheres(q["pts"], q["radius"], 4), soft)
    out["sample_surface"] = ask(lambda: ctx.sample_surface(SC.N_QUERIES, SEED), soft)
    out["surface_info"] = ask(ctx.surface_info, soft)
    out["bake_lightmap"] = ask(lambda: ctx.bake_lightmap(16, 16, 1e-3 * SC.extent(arrays), DEPTH, 0, 2, SEED), soft)
    out["bake_probes"] = ask(lambda: ctx.bake_probes(pos, dirs, DEPTH, 0, 2, SEED, 0.785398), soft)
    out["probe_visibility"] = ask(lambda: ctx.bake_probe_visibility(pos, dirs, 4, SC.extent(arrays), 0, SEED), soft)
    return out


def after_update(ctx, name):
    """... and after the first min(n, 8) triangles made a small rigid move"""
    arrays = SC.scene(name)[0]
    n = len(arrays["verts"])
    q = SC.queries(name)
    k = min(n, 8)
    ctx.update_geometry(0, SC.moved(arrays, k))
    info = ctx.geometry_info()
    ctx.reset(); ctx.render(0, SPP, SEED)
    return {"updates": info["updates"], "refitted": info["refitted"], "sah_built": info["sah_built"], "sah_now": info["sah_now"],
            "moved accum": ctx.read_accum(), "moved rgb8": ctx.resolve_rgb8(),
            "moved closest": ask(lambda: ctx.closest_points(q["pts"], q["max_dist"]), n == 0)}


def hold_to_fresh(oracle_mod, x, y, name):
    """x and y both hold the scene `name`, staged and reset: every answer equal, the render the oracle's, before and after an update"""
    arrays, cam = SC.scene(name)
    n = len(arrays["verts"])
    ax, ay = answers(x, name), answers(y, name)
    ref, ref8 = oracle_render(oracle_mod, name, arrays, cam)
    assert np.array_equal(ay["accum"].view(np.uint32), ref.view(np.uint32)) and np.array_equal(ay["rgb8"], ref8), "the fresh context misses the oracle"
    assert differing(ax, ay) == [], name
    for key, a in ay.items():
        if n and key not in ("flat_classes", "flat_rect_pairs"):
            assert not isinstance(a, Refused), (key, a)
    assert isinstance(ay["flat_classes"], Refused) == (not 0 < n <= 16) == isinstance(ay["flat_rect_pairs"], Refused)
    if n:
        hit = ay["intersect"][0] >= 0
        miss = np.arange(SC.N_QUERIES) % 3 == 2
        assert not hit[miss].any() and hit[~miss].any() and (ay["closest"][0][miss] < 0).all() and (ay["closest"][0][~miss] >= 0).any()
        assert (ay["sample_surface"][0] >= 0).all() and (ay["sample_surface"][0] < n).all()
    ux, uy = after_update(x, name), after_update(y, name)
    assert differing(ux, uy) == [], name
    assert uy["updates"] == (1 if n else 0) and ux["sah_built"] == uy["sah_built"]
    if n:
        mref, mref8 = oracle_render(oracle_mod, name + " moved", SC.after_move(arrays, min(n, 8)), cam)
        assert np.array_equal(ux["moved accum"].view(np.uint32), mref.view(np.uint32)) and np.array_equal(ux["moved rgb8"], mref8)
    return ax


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", SC.PAIRS, ids=SC.PAIR_IDS)
def test_a_context_that_changed_scenes_answers_like_a_fresh_one(oracle_mod, a, b):
    x, y = new_context(), new_context()
    try:
        stage(x, a)
        exercise(x, a)
        x.upload_scene(SC.scene(b)[0])           # no synchronize in between: the upload itself stands behind what is queued
        stage(x, b, upload=False)
        stage(y, b)
        got = hold_to_fresh(oracle_mod, x, y, b)
        if b == "empty":
            # the documented answers for a scene without triangles: misses, zeros, -1s, black
            assert not got["accum"].any() and not got["rgb8"].any() and got["bvh_info"][2] == 0
            assert (got["feature triangle"] == -1).all() and (got["feature material"] == -1).all() and np.isinf(got["feature depth"]).all()
            assert all(p[0] == -1 and p[1] == -1 for p in got["pick"])
            for key, want in (("intersect", -1), ("closest", -1), ("signed_distance", -1)):
                if not isinstance(got[key], Refused):
                    assert (got[key][0] == want).all() and np.isinf(got[key][1]).all(), key
            for key in ("occluded", "trace_rays"):
                if not isinstance(got[key], Refused):
                    assert not got[key].any(), key
            for key in ("crossings", "multihit", "nearest", "overlap_boxes", "overlap_spheres"):
                if not isinstance(got[key], Refused):
                    assert not got[key][0].any(), key
            if not isinstance(got["bake_lightmap"], Refused):
                assert not got["bake_lightmap"][0].any() and (got["bake_lightmap"][1] == -1).all()
    finally:
        x.close(); y.close()


# ---- frame state after the swap ------------------------------------------------------------------------------------------------------------
def refusal(ctx, fn, *words):
    """fn raises PtkError for PTK_ERR_BAD_ARG and ptk_last_error carries one of the refusal's words"""
    from pbrpathtracer_amd import ptk
    with pytest.raises(ptk.PtkError) as e:
        fn()
    text = ctx.L.ptk_last_error(ctx.h).decode()
    assert "(%d)" % BAD_ARG in str(e.value) and text in str(e.value) and any(w in text for w in words), (str(e.value), words)


def frame_products(ctx, name):
    """the frame entries over a fresh 4-spp render of the staged scene: everything they leave readable"""
    from pbrpathtracer_amd import ptk
    arrays = SC.scene(name)[0]
    prm = params(name)
    out = {}
    ctx.render(0, SPP, SEED)
    ctx.temporal_frame(prm["temporal"], seed=SEED, moments=True)
    out["temporal"] = ctx.read_temporal()
    out["moments"] = ctx.read_temporal_variance(variance=False)[0]
    ctx.temporal_variance(prm["variance"])
    out["variance"] = ctx.read_temporal_variance()
    ctx.denoise_frame(prm["denoise"], seed=SEED)
    out["denoised"] = ctx.read_denoised()
    ctx.temporal_frame(prm["temporal"], seed=SEED, moments=True)
    ctx.temporal_variance(prm["variance"])
    ctx.denoise_temporal(prm["denoise"])
    out["denoised temporal"] = ctx.read_denoised()
    ctx.render_guides(GW, GH, seed=SEED)
    out["guides"] = [ctx.read_guide(k) for k in (ptk.FEAT_MATERIAL, ptk.FEAT_POSITION, ptk.FEAT_NORMAL, ptk.FEAT_ALBEDO)]
    ctx.render_features(ptk.FEAT_ALL, 0, SEED)
    ctx.upsample_frame(ptk.UPSAMPLE_ACCUM, prm["upsample"])
    out["upsampled"] = ctx.read_upsampled()
    ctx.upsample_frame(ptk.UPSAMPLE_TEMPORAL, prm["upsample"])
    out["upsampled temporal"] = ctx.read_upsampled()
    ctx.display_frame(ptk.DISPLAY_ACCUM, prm["display"])
    out["display"] = ctx.read_display()
    ctx.display_frame(ptk.DISPLAY_DENOISED, prm["display"])
    out["display denoised"] = ctx.read_display()
    ctx.snapshot_geometry()
    ctx.update_geometry(0, SC.moved(arrays, 4))
    ctx.reset(); ctx.render(0, SPP, SEED)
    ctx.temporal_frame(prm["temporal"], seed=SEED, moving=True)
    out["temporal moving"] = ctx.read_temporal()
    out["motion"] = ctx.read_motion()
    return out


@pytest.mark.parametrize("a,b", [("flat_plain", "flat_generic"), ("flat_generic", "flat_plain")])
def test_an_upload_drops_the_frame_state_of_the_scene_that_goes(a, b):
    """The two boxes share walls and material indices (tests/test_scene_swap_cpu.py: by the rule, the old history would be taken at
    some 600 of the 1536 pixels): a history, a plane or a motion table that survived the upload shows here."""
    from pbrpathtracer_amd import ptk
    x, y = new_context(), new_context()
    try:
        stage(x, a)
        exercise(x, a)
        prm = params(b)
        view = x.get_view()
        before_state, before_accum, before_samples = x.display_state(), x.read_accum(), x.samples()
        assert before_samples == SPP and before_accum.any() and before_state["has_prev"]
        x.upload_scene(SC.scene(b)[0])
        # nothing derived from the old scene is handed out or consumed
        F = ptk.FEAT_MATERIAL
        for fn, words in ((lambda: x.read_feature(F), ("ptk_render_features first",)), (lambda: x.feature_device_ptr(F), ("ptk_render_features first",)),
                          (lambda: x.read_guide(F), ("ptk_render_guides first",)), (lambda: x.guide_device_ptr(F), ("ptk_render_guides first",)),
                          (x.read_denoised, ("no denoised frame",)), (x.read_temporal, ("no reprojected frame",)),
                          (lambda: x.read_temporal_variance(), ("no moments",)), (lambda: x.read_temporal_variance(variance=False), ("no moments",)),
                          (x.read_motion, ("no motion planes",)), (x.read_upsampled, ("no upsampled frame",)), (x.read_display, ("no display image",)),
                          (lambda: x.render_motion(view), ("first", "no feature planes")),
                          (lambda: x.temporal_frame(prm["temporal"], render_features=False), ("ptk_render_features first",)),
                          (lambda: x.temporal_frame(prm["temporal"], render_features=False, moving=True), ("first", "no feature planes")),
                          (lambda: x.temporal_frame(prm["temporal"], render_features=False, moments=True), ("ptk_render_features first",)),
                          (lambda: x.temporal_variance(prm["variance"]), ("no moments",)),
                          (lambda: x.denoise_temporal(prm["denoise"]), ("no reprojected frame", "no moments")),
                          (lambda: x.upsample_frame(ptk.UPSAMPLE_ACCUM, prm["upsample"]), ("ptk_render_features first", "ptk_render_guides first")),
                          (lambda: x.upsample_frame(ptk.UPSAMPLE_DENOISED, prm["upsample"]), ("first", "no denoised frame")),
                          (lambda: x.upsample_frame(ptk.UPSAMPLE_TEMPORAL, prm["upsample"]), ("first", "no temporal frame")),
                          (lambda: x.display_frame(ptk.DISPLAY_DENOISED, prm["display"]), ("no denoised frame",)),
                          (lambda: x.display_frame(ptk.DISPLAY_TEMPORAL, prm["display"]), ("no temporal frame",))):
            refusal(x, fn, *words)
        # what an upload keeps: the viewer's exposure state; the accumulator and the sample count, until the caller's reset
        assert same_bits(x.display_state(), before_state)
        assert np.array_equal(x.read_accum().view(np.uint32), before_accum.view(np.uint32)) and x.samples() == before_samples
        stage(x, b, upload=False)
        stage(y, b)
        assert not x.read_accum().any() and x.samples() == 0
        # the viewer's exposure state is not the scene's: give both contexts the same one before the display entries are compared
        x.display_reset(); y.display_reset()
        px, py = frame_products(x, b), frame_products(y, b)
        count = px["temporal"][1]
        assert (count == SPP).all() and (py["temporal"][1] == SPP).all(), "a fresh temporal frame counts the frame's own samples alone"
        assert differing(px, py) == [], (a, b)
    finally:
        x.close(); y.close()


# ---- work in flight ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_stream", [True, False], ids=["own stream", "caller's stream"])
def test_an_upload_behind_work_in_flight(oracle_mod, own_stream):
    """Three overlapped render batches, a geometry update and a ray query with a device output are queued on the device-built scene
    with no host wait; the upload of the flat scene follows at once.  It waits for the context's stream (ptk_api.hip: why that is
    enough), so the query's tensor holds the old scene's answer and the context then answers for the new scene like a fresh one."""
    import torch
    a, b = "bvh_device", "flat_plain"
    arrays = SC.scene(a)[0]
    q = SC.queries(a)
    dev = torch.device("cuda", 0)
    x, y, z = new_context(), new_context(), new_context()
    stream = None
    try:
        # the old scene's answer, from a context that waits at every step
        stage(z, a)
        z.update_geometry(0, SC.moved(arrays, 8))
        want = z.trace_rays(q["ro"], q["rd"], DEPTH, 0, 2, SEED)
        assert want.any()
        stage(x, a)
        ro, rd = torch.from_numpy(q["ro"]).to(dev), torch.from_numpy(q["rd"]).to(dev)
        out = torch.full((SC.N_QUERIES, 3), -7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        if not own_stream:
            stream = torch.cuda.Stream(device=dev)
            x.set_stream(stream.cuda_stream)
        x.reset()
        for k in range(3):
            x.render(k * SPP, SPP, SEED)
        x.update_geometry(0, SC.moved(arrays, 8))
        x.L.ptk_trace_rays_device(x.h, SC.N_QUERIES, C.c_void_p(ro.data_ptr()), C.c_void_p(rd.data_ptr()), DEPTH, 0, 2, SEED, 0, 0,
                                  C.c_void_p(out.data_ptr()))
        x.upload_scene(SC.scene(b)[0])
        got = out.cpu().numpy()                  # (the upload waited for the stream the query ran on)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        stage(x, b, upload=False)
        stage(y, b)
        hold_to_fresh(oracle_mod, x, y, b)
    finally:
        x.close(); y.close(); z.close()
        del stream


# ---- refused uploads ------------------------------------------------------------------------------------------------------------------------
def resident(ctx, name):
    from pbrpathtracer_amd import ptk
    q = SC.queries(name)
    ctx.reset(); ctx.render(0, SPP, SEED)
    out = {"accum": ctx.read_accum(), "rgb8": ctx.resolve_rgb8()}
    for k, nm in enumerate(ptk.FEAT_NAMES):
        out["feature " + nm] = ctx.read_feature(k)           # (the planes of the render_features before the refused calls)
    out["closest"] = ctx.closest_points(q["pts"], q["max_dist"])
    out["sample_surface"] = ctx.sample_surface(SC.N_QUERIES, SEED)
    out["surface_info"] = ctx.surface_info()
    out["geometry_info"] = ctx.geometry_info()
    out["bvh_info"] = ctx.bvh_info()
    return out


def test_a_refused_upload_leaves_the_resident_scene_as_it_was(oracle_mod):
    from pbrpathtracer_amd import ptk
    name = "bvh_textured"
    arrays, cam = SC.scene(name)
    good = ptk.normalise_arrays(arrays)
    n = len(good["verts"])

    def edited(key, index, value):
        a = dict(good)
        a[key] = good[key].copy()
        a[key][index] = value
        return a

    def tex_edit(field, index, value):
        a = dict(good)
        a[field[0]] = good[field[0]].copy()
        a[field[0]][field[1]][index] = value
        return a

    cases = [("material index", edited("material", 5, len(good["materials"])), None, BAD_ARG, "triangle material index out of range"),
             ("negative material index", edited("material", n - 1, -1), None, BAD_ARG, "triangle material index out of range"),
             ("light index", edited("lights", 0, n), None, BAD_ARG, "light triangle index out of range"),
             ("texture outside the atlas", tex_edit(("textures", "offset"), 1, good["texels"].size), None, BAD_ARG, "texture outside the texel atlas"),
             ("material texture index", tex_edit(("materials", "tex"), (2, 0), len(good["textures"])), None, BAD_ARG, "material texture index out of range"),
             ("NaN coordinate", edited("verts", (n // 2, 4), np.nan), None, LIMIT, "not finite or exceeds 2^61"),
             ("infinite coordinate", edited("verts", (n - 1, 8), -np.inf), None, LIMIT, "not finite or exceeds 2^61"),
             ("coordinate of 2^61", edited("verts", (0, 0), 2.0 ** 61), None, LIMIT, "not finite or exceeds 2^61"),
             ("null vertices", good, dict(verts=None), BAD_ARG, "null triangle/material array"),
             ("null materials", good, dict(materials=None), BAD_ARG, "null triangle/material array"),
             ("null lights", good, dict(lights=None), BAD_ARG, "null light array"),
             ("null textures", good, dict(textures=None), BAD_ARG, "null texture array"),
             ("negative triangle count", good, dict(num_triangles=-1), BAD_ARG, "negative count"),
             ("negative light count", good, dict(num_lights=-3), BAD_ARG, "negative count"),
             ("negative material count", good, dict(num_materials=-1), BAD_ARG, "negative count"),
             ("negative texture count", good, dict(num_textures=-2), BAD_ARG, "negative count")]
    x = new_context()
    try:
        stage(x, name)
        x.set_surface_weights(np.linspace(0.25, 3.0, n).astype(F32))
        x.update_geometry(0, SC.moved(arrays, 8))
        x.render_features(ptk.FEAT_ALL, 0, SEED)
        before = resident(x, name)
        assert before["geometry_info"]["updates"] == 1 and before["accum"].any()
        ref, _ = oracle_render(oracle_mod, name + " moved", SC.after_move(arrays, 8), cam)
        assert np.array_equal(before["accum"].view(np.uint32), ref.view(np.uint32))
        for what, a, fields, code, words in cases:
            d = ptk.scene_desc(a)
            for k, v in (fields or {}).items():
                setattr(d, k, v)
            rc = x.L.ptk_upload_scene(x.h, C.byref(d))
            text = x.L.ptk_last_error(x.h).decode()
            assert rc == code and words in text, (what, rc, text)
            assert differing(resident(x, name), before) == [], what
    finally:
        x.close()
