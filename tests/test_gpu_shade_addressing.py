"""The cycle unit's shade block as it is compiled since its table reads go by 32-bit byte offsets, its hemisphere angle is computed in
float and two of its square roots lost their range test (csrc/ptk_device_fn.h ldg_at / sqrt_ieee_pos, csrc/ptk_angle_f32.h,
csrc/ptk_trace_shade.h; DESIGN 4.1 "The shade block's addressing").

None of that may change a sample: every comparison is np.array_equal on the float accumulator - against the CPU oracle and against
the same render under "flat_cycle" 0, the pair unit's kernel, which compiles the same shade block with 64-bit addressing, the double
angle and the guarded roots.  ptk_trace_unit reports the cycle unit in every case.

  * the golden Cornell box at 96 x 64, depth 8, 16 spp (LAMBERT level);
  * a 16-triangle PLAIN scene at 40 x 24, depth 4, 32 spp: seven materials, the last of them with reflectiveness > 0 and a
    roughness strictly inside (0, 1) on the LAST triangle - the generic level, the last rows of the shading, frame and material
    tables, the lobe sampler - and three light triangles, the third of them the scene's thirteenth: lightId takes its last value;
  * the Cornell box again as rank 1 of a 3-way tile split of a 100 x 52 frame (not a multiple of the 16 x 16 tile in either
    direction): the path start's pixel offsets are no dense prefix of its three tables, and the last tile row and column are cut.
Every oracle image is computed once per module."""
import numpy as np
import pytest

import flat_zero_scenes as Z
from feature_truth import owned_mask

pytestmark = pytest.mark.gpu

SEED = 53
DEFAULTS = (("flat_cycle", 1), ("flat_rect_pairs", 1), ("flat_zero_classes", 1), ("plain_kernel", 1), ("lambert_kernel", 1), ("persistent", -1),
            ("chunk", 0), ("contract", 0))


def sixteen_with_every_last_row(a):
    """Z.sixteen's box with two panels; panel triangle 12 becomes a third light (the light material), the last triangle gets a new
    LAST material: reflectiveness 0.7, roughness 0.4"""
    b = Z.sixteen(a)
    b["material"] = b["material"].copy()
    light_mat = int(a["material"][int(a["lights"][0])])
    mats = np.concatenate([a["materials"], a["materials"][:1]])
    mats["reflectiveness"][-1] = np.float32(0.7)
    mats["roughness"][-1] = np.float32(0.4)
    mats["diffuse"][-1] = np.array([0.25, 0.25, 0.75], np.float32)
    b["materials"] = mats
    b["material"][12] = light_mat
    b["material"][15] = len(mats) - 1
    b["lights"] = np.array([int(l) for l in a["lights"]] + [12], np.int32)
    return b


class _Refs:
    def __init__(self, OB):
        self.OB = OB
        self.box, self.cam = Z.cornell()
        self.sixteen = sixteen_with_every_last_row(self.box)
        self.images = {}

    def image(self, name, arrays, w, h, D, spp, rank=0, world=1):
        key = (name, w, h, D, spp, rank, world)
        if key not in self.images:
            c = self.cam
            o = self.OB.Oracle(arrays)
            tot, _ = o.render(self.OB.make_camera(c["pos"], c["dir"], c["up"], c["focal"], c["fovy"], c["focal_dist"], c["aperture"]),
                              w, h, D, 0, spp, SEED, rank=rank, world=world)
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


def _setup(ctx, arrays, cam, w, h, D):
    for name, v in DEFAULTS:
        ctx.set_option(name, v)
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(w, h, D); ctx.set_tile(0, 1)


def _both_units(ctx, spp, lambert, label):
    """the render by the cycle unit and by the pair unit ("flat_cycle" 0): the two accumulators"""
    from pbrpathtracer_amd import ptk
    try:
        ctx.set_option("flat_cycle", 1)
        ctx.reset(); ctx.render(0, spp, SEED)
        on = ctx.read_accum()
        assert (ctx.trace_variant(), ctx.trace_unit(), ctx.trace_is_lambert()) == (ptk.TRACE_FLAT_PLAIN, ptk.UNIT_CYCLE, lambert), label
        ctx.set_option("flat_cycle", 0)
        ctx.reset(); ctx.render(0, spp, SEED)
        off = ctx.read_accum()
        assert (ctx.trace_variant(), ctx.trace_unit(), ctx.trace_is_lambert()) == (ptk.TRACE_FLAT_PLAIN, ptk.UNIT_RECT, lambert), label
    finally:
        ctx.set_option("flat_cycle", 1)
    return on, off


def test_the_golden_cornell_box(ctx, refs):
    from pbrpathtracer_amd import ptk
    assert ptk.scene_is_plain(refs.box) and ptk.scene_is_lambert(refs.box)
    _setup(ctx, refs.box, refs.cam, 96, 64, 8)
    want = refs.image("box", refs.box, 96, 64, 8, 16)
    on, off = _both_units(ctx, 16, True, "box")
    assert (want != 0).any()
    assert np.array_equal(on, want), ("against the oracle", int((on != want).sum()))
    assert np.array_equal(on, off), ("against flat_cycle = 0", int((on != off).sum()))


def test_sixteen_triangles_seven_materials_three_lights(ctx, refs):
    from pbrpathtracer_amd import ptk
    a = refs.sixteen
    assert len(a["verts"]) == 16 and len(a["materials"]) >= 4 and len(a["lights"]) == 3
    assert int(a["material"][15]) == len(a["materials"]) - 1 and float(a["materials"]["reflectiveness"][-1]) > 0
    assert ptk.scene_is_plain(a) and not ptk.scene_is_lambert(a)
    _setup(ctx, a, refs.cam, 40, 24, 4)
    want = refs.image("sixteen", a, 40, 24, 4, 32)
    on, off = _both_units(ctx, 32, False, "sixteen")
    assert (want != 0).any()
    assert np.array_equal(on, want), ("against the oracle", int((on != want).sum()))
    assert np.array_equal(on, off), ("against flat_cycle = 0", int((on != off).sum()))
    # the last triangle is seen (its material tints what it reflects: the frame differs from the one without it) ...
    plain_last = dict(a); plain_last["material"] = a["material"].copy(); plain_last["material"][15] = int(a["material"][14])
    other = refs.image("sixteen, last triangle like its neighbour", plain_last, 40, 24, 4, 32)
    assert not np.array_equal(other, want)
    # ... and so is the third light (without it in the light list the frame is another)
    two = dict(a); two["lights"] = a["lights"][:2]
    assert not np.array_equal(refs.image("sixteen, two lights", two, 40, 24, 4, 32), want)


def test_rank_one_of_three_in_a_frame_that_is_no_multiple_of_the_tile(ctx, refs):
    from pbrpathtracer_amd import ptk
    w, h = 100, 52
    _setup(ctx, refs.box, refs.cam, w, h, 8)
    want = refs.image("box", refs.box, w, h, 8, 16, rank=1, world=3)       # (the oracle's own split: rank 1's pixels, zeros elsewhere)
    mine = owned_mask(w, h, 1, 3)
    assert mine.any() and not mine.all() and not mine[0, 0]           # (the frame's first pixels are another rank's: no dense prefix)
    assert (want != 0).any(axis=2).sum() <= mine.sum() < w * h
    try:
        ctx.set_tile(1, 3)
        on, off = _both_units(ctx, 16, True, "rank 1 of 3")
    finally:
        ctx.set_tile(0, 1)
    assert (want != 0).any()
    assert np.array_equal(on, want), ("against the oracle", int((on != want).sum()))
    assert np.array_equal(on, off), ("against flat_cycle = 0", int((on != off).sum()))
