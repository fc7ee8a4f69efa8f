"""The cycle unit's square roots from v_rsq_f32 (csrc/ptk_device_fn.h sqrt_ieee_rsq; DESIGN 4.1 "The cycle unit's roots") in whole renders,
against the pair unit ("flat_cycle" 0), which keeps the neighbour-test root, and against the CPU oracle.

Scenes: the 12-triangle Cornell golden at 64 x 48, 16 spp, depth 8, and six rows of tests/plain_random_scenes.py picked for what the
roots and the pass can meet - vertices snapped to a grid (rays through exact edges), bitwise twins (equal t), stored edge words of
-0.0, an empty light list, the camera in a rectangle's plane (zero determinants, NaN barycentrics, zero-length vectors), an oblique
record in front of rectangles only.  Each is rendered by both units at every PLAIN level the scene can run (the Lambert level where
no material reflects, the generic level - whose specular routes have two more roots - always), and once by the cycle unit resumed in
two halves.  Float accumulator and RGB8 must be np.array_equal between the units and with the oracle: no tolerance anywhere."""
import numpy as np
import pytest

import plain_random_scenes as P
from conftest import load_golden, scene_from_golden

pytestmark = pytest.mark.gpu

ROWS = {"grid-snapped": 31, "bitwise-twins": 7, "signed-zeros": 11, "no-lights": 6, "camera-in-plane": 10, "oblique-in-front": 50}
ROW_VARIANT = {"grid-snapped": 1, "bitwise-twins": 4, "signed-zeros": 5, "no-lights": 6, "camera-in-plane": 7, "oblique-in-front": 10}
CORNELL = (41, 12, 0, True, 64, 48, 8, 16)             # a row in the family's layout: (seed, n, variant, lambert, W, H, D, spp)
SCENES = ("cornell",) + tuple(ROWS)


def _cornell():
    z = load_golden("tier_s_cornell.npz")
    a = {k: np.array(v) for k, v in scene_from_golden(z).items()}
    cam = z["cam"]; proj = z["proj"]
    return a, dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]), focal_dist=float(z["focal_dist"]), aperture=0.0)


class _Refs:
    """scene, camera, row and the oracle's image of each, made once and read-only"""
    def __init__(self, OB):
        self.OB = OB; self.made = {}

    def get(self, name):
        if name not in self.made:
            row = CORNELL if name == "cornell" else P.FAMILY[ROWS[name]]
            a, cam = _cornell() if name == "cornell" else P.row_scene(row)
            self.made[name] = (a, cam, row, P.oracle_image(self.OB, a, cam, row))
        return self.made[name]


@pytest.fixture(scope="module")
def refs(oracle_mod):
    return _Refs(oracle_mod)


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def test_the_rows_are_the_compositions_they_are_named_for():
    assert all(P.FAMILY[k][2] == ROW_VARIANT[name] for name, k in ROWS.items())
    # both levels among them: three rows no material of which reflects, three with the lobe sampler's material
    assert sorted(P.FAMILY[k][3] for k in ROWS.values()) == [False] * 3 + [True] * 3


@pytest.mark.parametrize("name", SCENES)
def test_cycle_unit_pair_unit_and_oracle_agree_bit_for_bit(ctx, refs, name):
    from pbrpathtracer_amd import ptk
    a, cam, row, want = refs.get(name)
    seed, lam, spp = row[0], row[3], row[7]
    for opt in ("flat", "flat_rect_pairs", "flat_zero_classes", "plain_kernel", "lambert_kernel", "flat_cycle"):
        ctx.set_option(opt, 1)
    ctx.set_option("contract", 0)
    ctx.upload_scene(a); ctx.set_camera(**cam); ctx.set_frame(row[4], row[5], row[6]); ctx.set_tile(0, 1)
    got = {}
    try:
        for level in ((1, 0) if lam else (0,)):
            ctx.set_option("lambert_kernel", level)
            for cycle, unit in ((1, ptk.UNIT_CYCLE), (0, ptk.UNIT_RECT)):
                ctx.set_option("flat_cycle", cycle)
                ctx.reset(); ctx.render(0, spp, seed)
                got[(level, cycle)] = (ctx.read_accum(), ctx.resolve_rgb8())
                assert (ctx.trace_variant(), ctx.trace_unit(), ctx.trace_is_lambert()) == (ptk.TRACE_FLAT_PLAIN, unit, bool(lam and level)), (level, cycle)
        # the cycle unit resumed in two halves, at the level the scene runs by default
        ctx.set_option("lambert_kernel", 1); ctx.set_option("flat_cycle", 1)
        ctx.reset(); ctx.render(0, spp // 2, seed); ctx.render(spp // 2, spp - spp // 2, seed)
        got["resumed"] = (ctx.read_accum(), ctx.resolve_rgb8())
        assert ctx.trace_unit() == ptk.UNIT_CYCLE
    finally:
        ctx.set_option("lambert_kernel", 1); ctx.set_option("flat_cycle", 1)
    assert (want[0] != 0).any() or name == "no-lights"
    for key, (acc, rgb) in got.items():
        assert np.array_equal(acc.view(np.uint32), want[0].view(np.uint32)), (key, "accumulator words that differ from the oracle's", int((acc.view(np.uint32) != want[0].view(np.uint32)).sum()))
        assert np.array_equal(rgb, want[1]), (key, "RGB8")
    for level in ((1, 0) if lam else (0,)):
        assert np.array_equal(got[(level, 1)][0].view(np.uint32), got[(level, 0)][0].view(np.uint32)) and np.array_equal(got[(level, 1)][1], got[(level, 0)][1]), level
