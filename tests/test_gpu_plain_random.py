"""The PLAIN trace kernels (csrc/ptk_kernels_plain.hip, ptk_kernels_rect.hip, ptk_kernels_cycle.hip; both levels; the sixteen class bodies
and the six pair kinds of csrc/ptk_flat_mt.h; the frame table; the cycle unit's deal and its 32-bit table offsets) on the seeded random
scenes of tests/plain_random_scenes.py instead of edits of the one golden box.  tests/test_plain_random_cpu.py says what the family
reaches: every class, kind and prefix length 0..8, every arm of Trace a PLAIN kernel can take, tiles from empty to full.

Every comparison is np.array_equal on the float accumulator, and on the RGB8 image where one is read, against the CPU oracle: no
tolerance anywhere.  Every row of the family is rendered by the cycle unit and then under each option that takes a layer of the PLAIN
code away (the pair unit, the plain unit, no zero classes, the generic level, the generic FLAT kernel, the tree); one row in four also
resumed, split three ways and under the other work distributions; six pairs of rows across a partial ptk_update_geometry; six rows under
the contracted build, where PLAIN has to reproduce generic FLAT.  One context, and every oracle image once, per module."""
import numpy as np
import pytest

import plain_random_scenes as P

pytestmark = pytest.mark.gpu

DEFAULTS = (("flat", 1), ("flat_cycle", 1), ("flat_rect_pairs", 1), ("flat_zero_classes", 1), ("plain_kernel", 1), ("lambert_kernel", 1),
            ("persistent", -1), ("chunk", 0), ("contract", 0))
GROUPS = [list(range(k, len(P.FAMILY), 6)) for k in range(6)]          # six tests of eight or nine rows, every size of scene in each
SPLIT_ROWS = list(range(0, len(P.FAMILY), 4))
CONTRACT_ROWS = (5, 10, 18, 31, 47, 49)                                # 11 to 16 records, both levels, prefixes 0 to 8


class _Refs:
    """the family's scenes and the oracle's images of them, each made once and read-only"""
    def __init__(self, OB):
        self.OB = OB
        self.scenes = {}; self.images = {}

    def scene(self, k):
        if k not in self.scenes:
            self.scenes[k] = P.row_scene(P.FAMILY[k])
        return self.scenes[k]

    def image(self, k, rank=0, world=1, arrays=None, tag=None):
        key = (k, rank, world, tag)
        if key not in self.images:
            a, cam = self.scene(k)
            self.images[key] = P.oracle_image(self.OB, a if arrays is None else arrays, cam, P.FAMILY[k], rank, world)
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


def _setup(ctx, arrays, cam, row):
    for name, v in DEFAULTS:
        ctx.set_option(name, v)
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(row[4], row[5], row[6]); ctx.set_tile(0, 1)


def _render(ctx, row, rgb8=True):
    ctx.reset(); ctx.render(0, row[7], row[0])
    return ctx.read_accum(), (ctx.resolve_rgb8() if rgb8 else None)


def _kernel(ctx):
    return ctx.trace_variant(), ctx.trace_unit(), ctx.trace_is_lambert()


def _differs(got, want):
    """None when the accumulators (and the RGB8 images, where read) are equal, else how many words are not"""
    acc, rgb = got
    bad = int((acc.view(np.uint32) != want[0].view(np.uint32)).sum()) if acc.shape == want[0].shape else -1
    if bad == 0 and rgb is not None and not np.array_equal(rgb, want[1]):
        bad = -2
    return bad or None


def _row_under_every_option_set(ctx, refs, k):
    """-> the list of what went wrong for row k: [] when all seven renders are the oracle's image and ran the kernel they should"""
    from pbrpathtracer_amd import ptk
    row = P.FAMILY[k]; lam = row[3]
    a, cam = refs.scene(k)
    want = refs.image(k)
    wrong = []
    _setup(ctx, a, cam, row)
    classes, prefix = P.classify(a)
    if ctx.flat_classes() != classes: wrong.append(("classes", ctx.flat_classes(), classes))
    if ctx.flat_rect_pairs() != prefix: wrong.append(("pair prefix", ctx.flat_rect_pairs(), prefix))
    PLAIN = ptk.TRACE_FLAT_PLAIN
    expect = {"default": (PLAIN, ptk.UNIT_CYCLE, lam), "flat_cycle": (PLAIN, ptk.UNIT_RECT, lam), "flat_rect_pairs": (PLAIN, ptk.UNIT_PLAIN, lam),
              "flat_zero_classes": (PLAIN, ptk.UNIT_CYCLE, lam), "lambert_kernel": (PLAIN, ptk.UNIT_CYCLE, False),
              "plain_kernel": (ptk.TRACE_FLAT, ptk.UNIT_NONE, False), "flat": (ptk.TRACE_BVH, ptk.UNIT_NONE, False)}
    d = _differs(_render(ctx, row), want)
    if d: wrong.append(("default", "words that differ from the oracle's", d))
    if _kernel(ctx) != expect["default"]: wrong.append(("default", "kernel", _kernel(ctx)))
    for name, value, back in P.OPTION_SETS:
        if name == "lambert_kernel" and not lam:
            continue
        ctx.set_option(name, value)
        try:
            d = _differs(_render(ctx, row), want)
            if d: wrong.append((name, "words that differ from the oracle's", d))
            if _kernel(ctx) != expect[name]: wrong.append((name, "kernel", _kernel(ctx)))
        finally:
            ctx.set_option(name, back)
    return wrong


@pytest.mark.parametrize("group", range(len(GROUPS)))
def test_every_row_under_every_option_set_is_the_oracles_image(ctx, refs, group):
    """the cycle unit, then "flat_cycle" 0 (the pair unit), "flat_rect_pairs" 0 (the plain unit), "flat_zero_classes" 0, "lambert_kernel" 0
    (Lambert rows), "plain_kernel" 0 (generic FLAT) and "flat" 0 (the tree): accumulator and RGB8 of each equal the oracle's, each ran
    the kernel it names, and the device's classes and pair prefix after the upload are the host's"""
    wrong = {}
    for k in GROUPS[group]:
        w = _row_under_every_option_set(ctx, refs, k)
        if w: wrong[P.ROW_IDS[k]] = w
    assert not wrong, wrong


# ---- resumed and split renders ---------------------------------------------------------------------------------------------------------
def test_resumed_split_and_redistributed_renders_are_the_oracles_image(ctx, refs):
    """one row in four: two calls that share the samples; rank 1 of a three-way tile split against the oracle's own rank 1 of 3; one
    item per wave, the persistent loop, chunks of three"""
    from pbrpathtracer_amd import ptk
    wrong = {}
    for k in SPLIT_ROWS:
        row = P.FAMILY[k]; seed, spp = row[0], row[7]
        a, cam = refs.scene(k)
        want = refs.image(k)
        _setup(ctx, a, cam, row)
        w = []
        first = 1 + (seed % (spp - 1))
        ctx.reset(); ctx.render(0, first, seed); ctx.render(first, spp - first, seed)
        if _differs((ctx.read_accum(), ctx.resolve_rgb8()), want): w.append(("resumed at", first))
        try:
            ctx.set_tile(1, 3)
            if _differs(_render(ctx, row, rgb8=False), refs.image(k, 1, 3)): w.append("rank 1 of 3")
        finally:
            ctx.set_tile(0, 1)
        for name, value, back in (("persistent", 0, -1), ("persistent", 1, -1), ("chunk", 3, 0)):
            ctx.set_option(name, value)
            try:
                if _differs(_render(ctx, row), want): w.append((name, value))
                if _kernel(ctx) != (ptk.TRACE_FLAT_PLAIN, ptk.UNIT_CYCLE, row[3]): w.append((name, value, "kernel", _kernel(ctx)))
            finally:
                ctx.set_option(name, back)
        if w: wrong[P.ROW_IDS[k]] = w
    assert not wrong, wrong


# ---- geometry updates between family members ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", range(len(P.UPDATE_PAIRS)), ids=["%s<-%s" % (P.ROW_IDS[a], P.ROW_IDS[b]) for a, b in P.UPDATE_PAIRS])
def test_a_partial_update_from_another_row_is_the_oracles_image_of_the_mixed_scene(ctx, refs, pair):
    """A uploaded, a random proper sub-range of its triangles moved to B's by ptk_update_geometry: class table, pair prefix (longer for
    the first pair, shorter for the second) and frame table have to follow; the cycle unit and the pair unit against the oracle's image
    of the mixed arrays"""
    from pbrpathtracer_amd import ptk
    ia, ib = P.UPDATE_PAIRS[pair]
    row = P.FAMILY[ia]
    a, cam, first, v, nn, tb, mixed = P.mixed_scene(ia, ib)
    want = refs.image(ia, arrays=mixed, tag=("mixed", ib))
    assert not np.array_equal(want[0], refs.image(ia)[0])
    _setup(ctx, a, cam, row)
    assert not _differs(_render(ctx, row), refs.image(ia))
    ctx.update_geometry(first, v, nn, tb)
    classes, prefix = P.classify(mixed)
    assert ctx.flat_classes() == classes and ctx.flat_rect_pairs() == prefix
    try:
        for cycle, unit in ((1, ptk.UNIT_CYCLE), (0, ptk.UNIT_RECT)):
            ctx.set_option("flat_cycle", cycle)
            got = _render(ctx, row)
            assert _kernel(ctx) == (ptk.TRACE_FLAT_PLAIN, unit, row[3])
            assert not _differs(got, want), ("flat_cycle", cycle, _differs(got, want))
    finally:
        ctx.set_option("flat_cycle", 1)


# ---- contracted builds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", CONTRACT_ROWS, ids=[P.ROW_IDS[k] for k in CONTRACT_ROWS])
def test_contracted_plain_reproduces_contracted_generic(ctx, refs, k):
    """under "contract" 2 the images are not the oracle's; PLAIN is held to generic FLAT ("plain_kernel" 0) bit for bit, and to itself"""
    from pbrpathtracer_amd import ptk
    row = P.FAMILY[k]
    a, cam = refs.scene(k)
    _setup(ctx, a, cam, row)
    try:
        ctx.set_option("contract", 2)
        ctx.upload_scene(a)
        plain = _render(ctx, row); var_p = ctx.trace_variant()
        again = _render(ctx, row)
        ctx.set_option("plain_kernel", 0)
        generic = _render(ctx, row); var_g = ctx.trace_variant()
    finally:
        ctx.set_option("plain_kernel", 1); ctx.set_option("contract", 0)
    assert (var_p, var_g) == (ptk.TRACE_FLAT_PLAIN, ptk.TRACE_FLAT)
    assert (plain[0] != 0).any()
    assert not _differs(again, plain), "a second PLAIN render"
    assert not _differs(generic, plain), ("against plain_kernel = 0", _differs(generic, plain))
