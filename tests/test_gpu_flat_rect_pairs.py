"""The pair pass of the exact PLAIN trace kernels (csrc/ptk_kernels_rect.hip; csrc/ptk_flat_mt.h flat_rect_pair, mt_rect_pair,
mt_rect_accept; csrc/ptk_frame.hip classify_flat_kernel; include/ptk.h "flat_rect_pairs", ptk_flat_rect_pairs).

The prefix of the flat list that consists of fan-split axis-aligned rectangles is tested one pair of records at a time.  Nothing a
path computes may change: every comparison is np.array_equal on the float accumulator - pairs on against pairs off
("flat_rect_pairs" 0: the kernels without the pair loop), against the generic FLAT kernel ("plain_kernel" 0) and against the CPU
oracle.  The device's pair word is read back and held to the host rule.

Frames of 64 x 48, 4 spp, depths 1, 3 and 8; every oracle image is computed once per module and shared."""
import numpy as np
import pytest

import flat_rect_scenes as R
import flat_zero_scenes as Z

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 64, 48, 4, 31
DEPTHS = (1, 3, 8)


class _Refs:
    def __init__(self, OB):
        from pbrpathtracer_amd import ptk
        self.OB = OB; self.images = {}
        self.lists = R.all_lists(ptk.flat_rect_pair)
        _, self.cam = Z.cornell()

    def image(self, name, D, arrays=None, spp=SPP):
        key = (name, D, spp)
        if key not in self.images:
            c = self.cam
            o = self.OB.Oracle(self.lists[name][0] if arrays is None else arrays)
            tot, _ = o.render(self.OB.make_camera(c["pos"], c["dir"], c["up"], c["focal"], c["fovy"], c["focal_dist"], c["aperture"]),
                              W, H, D, 0, spp, SEED)
            o.close()
            tot.setflags(write=False)
            self.images[key] = tot
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
    for name, v in (("flat_rect_pairs", 1), ("flat_zero_classes", 1), ("plain_kernel", 1), ("lambert_kernel", 1), ("persistent", -1)):
        ctx.set_option(name, v)
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(0, 1)


def _render(ctx, spp=SPP):
    ctx.reset(); ctx.render(0, spp, SEED)
    return ctx.read_accum()


def _three_ways(ctx, want, label, lambert=True):
    """pairs on, pairs off, the generic FLAT kernel: each the oracle's accumulator, bit for bit"""
    from pbrpathtracer_amd import ptk
    try:
        ctx.set_option("flat_rect_pairs", 1)
        on = _render(ctx)
        assert ctx.trace_variant() == ptk.TRACE_FLAT_PLAIN and ctx.trace_is_lambert() == lambert, label
        ctx.set_option("flat_rect_pairs", 0)
        off = _render(ctx)
        assert ctx.trace_variant() == ptk.TRACE_FLAT_PLAIN and ctx.trace_is_lambert() == lambert, label
        ctx.set_option("plain_kernel", 0)
        generic = _render(ctx)
        assert ctx.trace_variant() == ptk.TRACE_FLAT, label
    finally:
        ctx.set_option("plain_kernel", 1); ctx.set_option("flat_rect_pairs", 1)
    assert np.array_equal(on, off), (label, "against flat_rect_pairs = 0", int((on != off).sum()))
    assert np.array_equal(on, generic), (label, "against plain_kernel = 0", int((on != generic).sum()))
    assert np.array_equal(on, want), (label, "against the oracle", int((on != want).sum()))
    return on


def _list(ctx, refs, name, depths=DEPTHS, lambert=True):
    from pbrpathtracer_amd import ptk
    arrays, n_pairs = refs.lists[name]
    _setup(ctx, arrays, refs.cam)
    pairs = ctx.flat_rect_pairs()
    assert pairs == ptk.flat_rect_prefix(arrays["verts"]) and len(pairs) == n_pairs, (name, pairs)
    lit = False
    for D in depths:
        ctx.set_frame(W, H, D)
        lit |= bool((_three_ways(ctx, refs.image(name, D), (name, D), lambert) != 0).any())
        assert ctx.flat_rect_pairs() == pairs                        # the option does not touch the classification
    assert lit, name
    return pairs


LISTS = ["box", "golden-order", "light-alone", "light-then-singles", "sixteen", "prefix+1", "prefix+3", "signed-zeros", "triangle-first"]


@pytest.mark.parametrize("name", LISTS)
def test_pairs_on_equal_off_equal_generic_equal_oracle(ctx, refs, name):
    """the box; one rectangle alone, which is the light; the light quad as the only pair; eight rectangles in 16 records; a prefix
    followed by one and by three single records of different classes; stored zeros of unlike sign; no prefix at all"""
    _list(ctx, refs, name)


def test_every_kind_first_and_last(ctx, refs):
    first, last = set(), set()
    for k in range(1, 7):
        pairs = _list(ctx, refs, f"kind{k}-first")
        assert len(pairs) == 6 and pairs[0] == k, (k, pairs)
        first.add(pairs[0]); last.add(pairs[-1])
    assert first == last == set(range(1, 7)), (first, last)


def test_a_mirror_material_runs_the_generic_level(ctx, refs):
    from pbrpathtracer_amd import ptk
    for name in ("box", "prefix+3"):
        arrays = Z.mirror(refs.lists[name][0])
        assert ptk.scene_is_plain(arrays) and not ptk.scene_is_lambert(arrays)
        _setup(ctx, arrays, refs.cam)
        assert len(ctx.flat_rect_pairs()) == refs.lists[name][1]
        for D in DEPTHS:
            ctx.set_frame(W, H, D)
            _three_ways(ctx, refs.image(name + "/mirror", D, arrays), (name, "mirror", D), lambert=False)
    # ... and a Lambert list through that level as well
    _setup(ctx, refs.lists["box"][0], refs.cam)
    ctx.set_option("lambert_kernel", 0)
    try:
        _three_ways(ctx, refs.image("box", 8), ("box", "lambert_kernel 0"), lambert=False)
    finally:
        ctx.set_option("lambert_kernel", 1)


@pytest.mark.parametrize("name", ["box", "prefix+3"])
def test_one_item_per_wave_and_a_three_way_tile_split(ctx, refs, name):
    _setup(ctx, refs.lists[name][0], refs.cam)
    want = refs.image(name, 8)
    ctx.set_option("persistent", 0)
    try:
        _three_ways(ctx, want, (name, "one item per wave"))
    finally:
        ctx.set_option("persistent", -1)
    for use in (1, 0):
        ctx.set_option("flat_rect_pairs", use)
        total = np.zeros_like(want)
        for r in range(3):
            ctx.set_tile(r, 3)
            part = _render(ctx)
            assert not np.any((part != 0) & (total != 0))
            total += part
        ctx.set_tile(0, 1)
        assert np.array_equal(total, want), (name, use, "tiles")
    ctx.set_option("flat_rect_pairs", 1)


def test_a_geometry_update_breaks_a_pair_by_one_ulp_and_another_restores_it(ctx, refs):
    """one ulp on one coordinate of the second pair's far corner, in its second record only: the prefix ends in front of that pair,
    the frame is the oracle's for the moved geometry; the old vertices back: six pairs and the first frame again"""
    from pbrpathtracer_amd import ptk
    a = refs.lists["box"][0]
    _setup(ctx, a, refs.cam)
    p0 = ctx.flat_rect_pairs()
    assert len(p0) == 6
    first = _three_ways(ctx, refs.image("box", 8), "before")
    moved = dict(a); moved["verts"] = a["verts"].copy()
    v = moved["verts"][3].reshape(3, 3)                              # record 3 = (p0, p2, p3) of the second quad: p2 along an in-plane axis
    axis = [k for k in range(3) if v[1, k] != v[0, k]][0]
    # (the stored word is the float32 difference p2 - p0: step the coordinate until that difference moves, and it moves by one ulp)
    edge = np.float32(v[1, axis] - v[0, axis])
    for _ in range(4):
        v[1, axis] = np.nextafter(v[1, axis], np.float32(np.inf))
        if np.float32(v[1, axis] - v[0, axis]) != edge: break
    assert np.float32(v[1, axis] - v[0, axis]) == np.nextafter(edge, np.float32(np.inf))
    assert ptk.flat_rect_prefix(moved["verts"]) == p0[:1]
    ctx.update_geometry(3, moved["verts"][3:4])
    assert ctx.flat_rect_pairs() == p0[:1]
    _three_ways(ctx, refs.image("box/one ulp", 8, moved), "one ulp")
    # with the option off across an update the pass's word stays empty and the classification follows the records
    ctx.set_option("flat_rect_pairs", 0)
    ctx.update_geometry(3, a["verts"][3:4])
    assert ctx.flat_rect_pairs() == p0
    ctx.set_option("flat_rect_pairs", 1)
    again = _three_ways(ctx, refs.image("box", 8), "restored")
    assert np.array_equal(again, first)


def test_scenes_without_a_flat_list_have_no_pair_word(ctx):
    from pbrpathtracer_amd import ptk
    from test_gpu_random_scenes import random_scene
    arrays, cam = random_scene(14, 300, True)
    ctx.upload_scene(arrays)
    with pytest.raises(ptk.PtkError):
        ctx.flat_rect_pairs()
