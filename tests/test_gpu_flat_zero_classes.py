"""Zero classes in the exact PLAIN trace kernels (csrc/ptk_kernels.hip: the pass's class switch; csrc/ptk_flat_mt.h: the bodies;
csrc/ptk_frame.hip classify_flat_kernel; include/ptk.h "flat_zero_classes", ptk_flat_classes).

A record whose edge words hold stored zeros goes to a body of the triangle test from which the operations on those words are
deleted.  Nothing a path computes may change: every comparison is np.array_equal on the float accumulator and the RGB8 image -
classes on against classes off ("flat_zero_classes" 0: every record general) and against the CPU oracle.  The device's class
table is read back and held to the host rule, and across the scenes every built class is selected by some triangle.

Frames of 96 x 64, 8 spp, depth 8 (and 1, 2); every oracle image is computed once per module and shared."""
import numpy as np
import pytest

import flat_zero_scenes as Z

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 96, 64, 8, 23
DEPTHS = (8, 1, 2)


class _Refs:
    def __init__(self, OB):
        self.OB = OB; self.images = {}
        self.scenes = Z.all_scenes()
        _, self.cam = Z.cornell()

    def image(self, scene, D, spp=SPP, arrays=None):
        key = (scene, D, spp)
        if key not in self.images:
            c = self.cam
            o = self.OB.Oracle(self.scenes[scene] if arrays is None else arrays)
            tot, rgb = o.render(self.OB.make_camera(c["pos"], c["dir"], c["up"], c["focal"], c["fovy"], c["focal_dist"], c["aperture"]),
                                W, H, D, 0, spp, SEED)
            o.close()
            tot.setflags(write=False); rgb.setflags(write=False)
            self.images[key] = (tot, rgb)
        return self.images[key]


@pytest.fixture(scope="module")
def refs(oracle_mod):
    return _Refs(oracle_mod)


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def _setup(ctx, arrays, cam, D=8):
    ctx.set_option("flat_zero_classes", 1)
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(0, 1)


def _render(ctx, spp=SPP):
    ctx.reset(); ctx.render(0, spp, SEED)
    return ctx.read_accum(), ctx.resolve_rgb8()


def _same(got, ref, label):
    assert np.array_equal(got[0], ref[0]), (label, "accumulator", int((got[0] != ref[0]).sum()))
    assert np.array_equal(got[1], ref[1]), (label, "rgb8", int((got[1] != ref[1]).sum()))


def _host_classes(arrays):
    from pbrpathtracer_amd import ptk
    return [ptk.flat_zero_class(t[0], t[1], t[2]) for t in np.asarray(arrays["verts"], np.float32).reshape(-1, 3, 3)]


def _on_off_oracle(ctx, refs, name, depths=DEPTHS, lambert=True):
    from pbrpathtracer_amd import ptk
    arrays = refs.scenes[name]
    _setup(ctx, arrays, refs.cam)
    classes = ctx.flat_classes()
    assert classes == _host_classes(arrays), name
    for D in depths:
        ctx.set_frame(W, H, D)
        want = refs.image(name, D)
        for use in (1, 0, 1):
            ctx.set_option("flat_zero_classes", use)
            got = _render(ctx)
            assert ctx.trace_variant() == ptk.TRACE_FLAT_PLAIN and ctx.trace_is_lambert() == lambert, name
            _same(got, want, (name, D, use))
            assert ctx.flat_classes() == classes                    # the option does not touch the classification
        assert D < 8 or len(classes) < 12 or (want[0] != 0).any(), name
    return classes


SCENES = ["cornell", "in-plane", "skewed", "mixed", "one", "sixteen"] + [f"rolled{j}" for j in range(6)]


def test_classes_on_equal_off_equal_oracle_and_every_class_is_selected(ctx, refs):
    """the box, its quads in every vertex rotation and both windings, axis-plane triangles without an axis-parallel edge, the box
    turned about a skew axis, a mixed scene; 1, 12 and 16 triangles"""
    reached = {}
    for name in SCENES:
        for c in _on_off_oracle(ctx, refs, name, DEPTHS if name in ("cornell", "mixed") else (8,)):
            reached.setdefault(c, name)
    assert set(reached) == set(range(16)), sorted(set(range(16)) - set(reached))
    assert all(c >= 4 for c in _host_classes(refs.scenes["cornell"])) and _host_classes(refs.scenes["skewed"]) == [0] * 12


def test_a_mirror_material_runs_the_generic_level_of_the_plain_kernel(ctx, refs):
    from pbrpathtracer_amd import ptk
    assert ptk.scene_is_plain(refs.scenes["mirror"]) and not ptk.scene_is_lambert(refs.scenes["mirror"])
    for name in ("mirror",):
        _on_off_oracle(ctx, refs, name, DEPTHS, lambert=False)
    # ... and the Lambert scenes through that level as well
    ctx.set_option("lambert_kernel", 0)
    try:
        for name in ("cornell", "rolled3", "mixed"):
            _on_off_oracle(ctx, refs, name, (8,), lambert=False)
    finally:
        ctx.set_option("lambert_kernel", 1)


@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_tile_split_and_resumed_sample_range(ctx, refs, name):
    _setup(ctx, refs.scenes[name], refs.cam)
    want, want24 = refs.image(name, 8), refs.image(name, 8, 24)
    for use in (1, 0):
        ctx.set_option("flat_zero_classes", use)
        total = np.zeros_like(want[0])
        for r in range(3):
            ctx.set_tile(r, 3); ctx.reset(); ctx.render(0, SPP, SEED)
            part = ctx.read_accum()
            assert not np.any((part != 0) & (total != 0))
            total += part
        ctx.set_tile(0, 1)
        assert np.array_equal(total, want[0]), (name, use, "tiles")
        ctx.reset()
        for first, n in ((0, 5), (5, 1), (6, 18)):
            ctx.render(first, n, SEED)
        _same((ctx.read_accum(), ctx.resolve_rgb8()), want24, (name, use, "resumed"))
    ctx.set_option("flat_zero_classes", 1)


def test_geometry_updates_reclassify_on_the_device(ctx, refs):
    """tilt the back wall out of its plane through the public API: its two records read general, the frame equals a fresh
    context's and the oracle's; move it back: specialised again, the first frame again; a refused update leaves the table alone"""
    from pbrpathtracer_amd import ptk
    a = refs.scenes["cornell"]
    back = [k for k in range(12) if Z.plane_axis(a["verts"][k]) == 2]
    assert len(back) == 2 and back[1] == back[0] + 1
    tilted = Z.transformed(a, Z._rot((1.0, 0.0, 0.0), 8.0), back, about=(0.0, 0.0, 1.0))
    _setup(ctx, a, refs.cam)
    c0 = ctx.flat_classes()
    assert all(c >= 4 for c in c0)
    first = _render(ctx)
    _same(first, refs.image("cornell", 8), "before")
    ctx.update_geometry(back[0], tilted["verts"][back], tilted["normals"][back], tilted["tbn"][back])
    c1 = ctx.flat_classes()
    assert [c1[k] for k in back] == [0, 0] and [c for k, c in enumerate(c1) if k not in back] == [c for k, c in enumerate(c0) if k not in back]
    assert c1 == _host_classes(tilted)
    got = _render(ctx)
    fresh = ptk.Context(0)
    try:
        _setup(fresh, tilted, refs.cam)
        assert fresh.flat_classes() == c1
        _same(got, _render(fresh), "fresh context")
    finally:
        fresh.close()
    want = refs.image("tilted", 8, arrays=tilted)
    _same(got, want, "oracle")
    assert not np.array_equal(want[0], first[0])
    # a refused update (a coordinate that is not finite) changes nothing, the table included
    bad = tilted["verts"][back].copy(); bad[0, 0] = np.inf
    with pytest.raises(ptk.PtkError):
        ctx.update_geometry(back[0], bad)
    assert ctx.flat_classes() == c1
    _same(_render(ctx), want, "after the refused update")
    # vertices only, back into the plane (the tilted normals stay: compare with a fresh upload of exactly that, and the oracle)
    ctx.update_geometry(back[0], a["verts"][back])
    assert ctx.flat_classes() == c0
    restored = dict(tilted); restored["verts"] = a["verts"]
    _same(_render(ctx), refs.image("restored", 8, arrays=restored), "moved back")
    ctx.update_geometry(back[0], a["verts"][back], a["normals"][back], a["tbn"][back])
    assert ctx.flat_classes() == c0
    _same(_render(ctx), first, "the first frame again")
    # the option off across an update: the pass's word stays general, the classification follows the records
    ctx.set_option("flat_zero_classes", 0)
    ctx.update_geometry(back[0], tilted["verts"][back], tilted["normals"][back], tilted["tbn"][back])
    assert ctx.flat_classes() == c1
    _same(_render(ctx), want, "option off")
    ctx.set_option("flat_zero_classes", 1)
    _same(_render(ctx), want, "option on again")


def test_scenes_without_a_flat_list_have_no_class_table(ctx):
    from pbrpathtracer_amd import ptk
    from test_gpu_random_scenes import random_scene
    arrays, cam = random_scene(14, 300, True)
    ctx.upload_scene(arrays)
    with pytest.raises(ptk.PtkError):
        ctx.flat_classes()
