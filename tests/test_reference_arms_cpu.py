"""The census of Trace's arms over the reference's TAPES (tests/reference_arms.py): every GPU test ends in "bit for bit against the
oracle", which is worth as much as the oracle's agreement with the reference - and that agreement is pinned, inside the suite, by the
tape replays of tests/test_oracle_golden.py alone.  Here: every arm of the oracle's Trace is taken at least FLOOR times by some
committed tape (tier_t_*: paths, tier_f_*: whole frames, both found by glob), or the reference gives no answer there that a tape
could pin - and then no tape takes it.  Needs neither a device nor the reference: the fixtures carry its answers."""
import numpy as np
import pytest

import reference_arms as RA
import trace_arms as TA
from conftest import load_golden, scene_from_golden

_UPPER = ("difference 5: where a wrapped coordinate rounds up to 1.0 the reference reads one texel past the row or the image "
          "(image.cpp:76-77) - another texel, or memory that is not the image's; the oracle clamps")
_OPACITY = ("difference 4: the reference draws once per leaf it visits, in the order of its per-run random tree (pathtracer.cpp:469-476, "
            "mesh.cpp:171-172): no tape holds those draws in an order the oracle's walk could take them; tests/test_opacity_expectations_cpu.py "
            "pins the opacity test to exact expectations instead")
_TIE = ("difference 3: at equal t the reference keeps the hit of whichever child its per-run random tree visits last "
        "(pathtracer.cpp:429-440, mesh.cpp:171-172): the winner changes from run to run")

# arm -> why no tape of the reference can pin it.  (NOT here: the lower clamps.  (int)NaN is INT_MIN, and in the reference as
# compiled 4 * (INT_MIN * width + INT_MIN) wraps to 0: a non-finite coordinate reads texel 0 of its row (column; of the image), the
# texel the oracle clamps to - tier_f_edges replays it bit for bit.)
NOT_REPLAYABLE = {
    "direct.light_id_clamped": "pathtracer.cpp:509-511: Rand() is std::uniform_real_distribution<float>(0, 1), at most 1 - 2^-24 (libstdc++ returns the "
                               "float below 1 where its quotient rounds to 1), and nl * (1 - 2^-24) rounds to the float below nl: no draw the reference "
                               "can put on a tape takes its own clamp",
    "closest_hit.stack_guard": TA.NOWHERE["closest_hit.stack_guard"] + " - and the guard is the oracle's own: the reference's Hit recurses",
}
assert set(NOT_REPLAYABLE) == set(TA.NOWHERE)
NOT_REPLAYABLE.update({f"tex2d.{slot}.upper_clamp_{ax}": _UPPER for slot in ("diffuse", "normal", "emissive", "roughness", "metallic", "opacity")
                       for ax in "xy"})
NOT_REPLAYABLE.update({f"tex2d.opacity.{arm}": _OPACITY for arm in ("missing_texture", "lower_clamp_x", "lower_clamp_y", "plain_fetch")})
NOT_REPLAYABLE.update({"test_triangle.opacity_draw_kept": _OPACITY, "test_triangle.opacity_draw_dropped": _OPACITY,
                       "test_triangle.tie_accepted_smaller_index": _TIE, "test_triangle.tie_rejected_larger_index": _TIE})

# the second batch of tapes (oracle/gen_golden.py tier_f2 / tier_t2) and an arm each of them alone carries over the floor
SECOND_BATCH = {
    "tier_f_bright": "shade.rr_killed_between_cap_and_max", "tier_f_nolights": "direct.no_lights",
    "tier_f_open": "direct.shadow_ray_missed_everything", "tier_f_edges": "tex2d.emissive.missing_texture",
    "tier_t_band_opaque": "sample_about.opaque_lobe.in_the_band", "tier_t_band_glass": "sample_about.glass_lobe.in_the_band",
}


@pytest.fixture(scope="module")
def counted(oracle_mod):
    return RA.census(oracle_mod)


def test_census_replay_is_the_replay(oracle_mod):
    """the counting entries return the very image (radiance) and draw count of the plain ones, on a frame and on paths"""
    z = load_golden("tier_f_edges.npz")
    o = oracle_mod.Oracle(scene_from_golden(z))
    cam = RA.golden_camera(oracle_mod, z)
    args = (cam, int(z["width"]), int(z["height"]), int(z["depth"]), z["tape"])
    ref, n = o.render_tape(*args)
    tot, nc, c = o.render_tape_census(*args)
    o.close()
    assert nc == n == int(z["ndraws"]) and np.array_equal(tot.view(np.uint32), ref.view(np.uint32)) and ref.any()
    assert sum(c.values()) > 0 and all(isinstance(k, str) and k for k in c) and len(set(c)) == len(c)
    z = load_golden("tier_t_glass.npz")
    o = oracle_mod.Oracle(scene_from_golden(z))
    D = int(z["depth"]); lit = 0; hits = 0
    for i in range(len(z["ro"])):
        tape = z["tape"][z["tape_off"][i]:z["tape_off"][i + 1]]
        for mode in (0, 1, 2):
            ref, n = o.trace_tape(z["ro"][i], z["rd"][i], D, tape, mode=mode)
            got, nc, c = o.trace_tape_census(z["ro"][i], z["rd"][i], D, tape, mode=mode)
            assert nc == n and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (i, mode)
            hits += c["test_triangle.accepted_nearer"]
        lit += bool(ref.any())
    o.close()
    assert lit > 100 and hits > 3 * lit


def test_every_arm_is_replayed_or_argued(counted):
    total, rows = counted
    print("\n" + RA.format_table(total, NOT_REPLAYABLE))
    names = list(total["F"])
    assert names == list(total["T"]) and set(NOT_REPLAYABLE) <= set(names), set(NOT_REPLAYABLE) - set(names)
    assert all(len(why) > 40 and ("difference" in why or name in TA.NOWHERE) for name, why in NOT_REPLAYABLE.items())
    assert len(RA.tape_fixtures("t")) >= 6 and len(RA.tape_fixtures("f")) >= 8
    short = []
    for n in names:
        count = total["T"][n] + total["F"][n]
        if n in NOT_REPLAYABLE:
            assert count == 0, f"{n}: listed as not replayable ({NOT_REPLAYABLE[n]}) and replayed {count} times"
        elif count < TA.FLOOR:
            short.append((n, count))
    assert not short, short


def test_every_tape_of_the_second_batch_is_needed(counted):
    """without any one of them a named arm falls under the floor"""
    total, rows = counted
    by_name = dict(rows)
    assert set(SECOND_BATCH) <= set(by_name), set(SECOND_BATCH) - set(by_name)
    for fixture, arm in SECOND_BATCH.items():
        all_ = total["T"][arm] + total["F"][arm]
        assert all_ >= TA.FLOOR and all_ - by_name[fixture][arm] < TA.FLOOR, (fixture, arm, all_, by_name[fixture][arm])


def test_fixtures_stay_small():
    """data only, and none larger than the largest tape of the first batch (tier_t_glass.npz)"""
    import os
    from conftest import GOLDEN
    limit = os.path.getsize(os.path.join(GOLDEN, "tier_t_glass.npz"))
    for name in RA.tape_fixtures("t") + RA.tape_fixtures("f"):
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= limit, name
        z = load_golden(name + ".npz")
        assert all(z[k].dtype.kind in "fiuV" for k in z.files), name
