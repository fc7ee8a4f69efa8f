"""Helper of tests/test_reference_arms_cpu.py - no tests of its own: the census of Trace's arms over the reference's TAPES, the
fixtures tests/golden/tier_t_*.npz (paths) and tier_f_*.npz (whole frames) that tests/test_oracle_golden.py replays against the
reference's recorded answers.  The oracle is held to the reference only on the arms some tape drives it through; on an arm no tape
takes it could misstate the reference, and every GPU test would hold the kernels bit for bit to the misstatement."""
import glob
import os

from conftest import GOLDEN, load_golden, scene_from_golden


def tape_fixtures(tier):
    """names (without .npz) of the committed tier "t" or "f" fixtures, found by glob"""
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, f"tier_{tier}_*.npz")))


def golden_camera(oracle_mod, z):
    return oracle_mod.make_camera(z["cam"][0:3], z["cam"][3:6], z["cam"][6:9], float(z["proj"][0]), float(z["proj"][1]),
                                  float(z["focal_dist"]), float(z["aperture"]))


def _add(total, c):
    for k, v in c.items():
        total[k] = total.get(k, 0) + v


def census_of_paths(oracle_mod, name):
    """{arm: count} over every path of one tier-T fixture, replayed as test_t_tape_paths replays it (mode 2)"""
    z = load_golden(name + ".npz")
    o = oracle_mod.Oracle(scene_from_golden(z))
    D = int(z["depth"])
    total = {}
    for i in range(len(z["ro"])):
        tape = z["tape"][z["tape_off"][i]:z["tape_off"][i + 1]]
        _, n, c = o.trace_tape_census(z["ro"][i], z["rd"][i], D, tape, mode=2)
        assert n == z["ndraws"][i], (name, i)
        _add(total, c)
    o.close()
    return total


def census_of_frame(oracle_mod, name):
    """{arm: count} over one tier-F fixture, replayed as test_f_whole_frames_replay_the_reference_bit_for_bit replays it"""
    z = load_golden(name + ".npz")
    o = oracle_mod.Oracle(scene_from_golden(z))
    _, n, c = o.render_tape_census(golden_camera(oracle_mod, z), int(z["width"]), int(z["height"]), int(z["depth"]), z["tape"])
    o.close()
    assert n == int(z["ndraws"]), name
    return c


def census(oracle_mod, skip=()):
    """({"T": {arm: count}, "F": {arm: count}}, rows [(fixture, {arm: count})]) over every committed tape fixture but `skip`"""
    total = {"T": {}, "F": {}}; rows = []
    for tier, fn in (("T", census_of_paths), ("F", census_of_frame)):
        for name in tape_fixtures(tier.lower()):
            if name in skip:
                continue
            c = fn(oracle_mod, name)
            rows.append((name, c))
            _add(total[tier], c)
    return total, rows


def format_table(total, not_replayable=()):
    names = list(total["F"])
    w = max(len(n) for n in names)
    lines = [f"{'arm':<{w}} {'tier T':>8} {'tier F':>8} {'total':>8}"]
    for n in names:
        t, f = total["T"].get(n, 0), total["F"].get(n, 0)
        lines.append(f"{n:<{w}} {t:>8} {f:>8} " + (f"{'-':>8}" if n in not_replayable and t + f == 0 else f"{t + f:>8}"))
    return "\n".join(lines)
