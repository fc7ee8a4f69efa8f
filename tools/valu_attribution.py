#!/usr/bin/env python3
"""Dynamic VALU budget of a FLAT trace kernel on a config, block by block: static VALU counts of the kernel's basic blocks
(tools/isa_blocks.py's parser on `hipcc -S` output) times how often the STATS kernel says each block ran.

    python3 tools/valu_attribution.py kernel.s generic|plain|lambert stats.json [measured SQ_INSTS_VALU of one full launch]

  kernel.s    hipcc -O3 ... --offload-arch=gfx950 --offload-device-only -S ptk_kernels.hip (the Makefile's flags)
  stats.json  ptk_collect_stats of one full launch (Context.collect_stats(0, spp, seed) as JSON)

The unit is the wave-instruction, what SQ_INSTS_VALU counts.  A FLAT wave runs ONE block per iteration of its main loop - the
triangle pass (walk_wave_iters) or the shade block (shade_wave_execs) - so the counts of the STATS kernel multiply the static
figures directly.  What they do not resolve is the inside of the shade block (which sampler route, whether any lane starts a
path, the square roots' fall-backs): every sub-block behind an execz branch runs when ANY lane of the wave takes it.  The shade
block is therefore given twice: as the static sum of its blocks that a config can reach (an upper bound per execution), and,
when a measured SQ_INSTS_VALU is passed, as what is left of the measurement once the exactly known groups are subtracted.

The block labels belong to ONE build of the kernel: each group below names its labels and the VALU count they must add up to,
and the script stops when the assembly no longer matches (re-derive the groups from tools/isa_blocks.py's table then).  The label
prefix (.LBB<n>_, n = the kernel's position in its file) is read from the assembly.  STALE for "plain" and "lambert" since the exact PLAIN
pass switches per triangle to a zero-class body: their groups name the single pass block of the kernels before that, so
the script stops on today's assembly; the per-class figures of DESIGN 5 come from tools/isa_blocks.py directly.  "lambert" is the LAMBERT level of the PLAIN
kernel; its stats come from the same STATS kernel (the counters-enabled kernels have neither variant)."""
import json
import re
import sys


def blocks_of(path, want):
    """label -> static VALU count, for the kernel whose symbol contains `want`"""
    out, cur, active = {}, None, False
    for line in open(path):
        s = line.strip()
        if re.match(r"^[A-Za-z_.$][\w.$]*:", s) and not s.startswith(".L"):
            active = want in s
        if not active:
            continue
        m = re.match(r"^(\.LBB[\w]+|[A-Za-z_][\w.$]*):", s)
        if m:
            cur = m.group(1); out[cur] = 0
            continue
        if cur is not None and s.startswith("v_"):
            out[cur] += 1
    return out


# group: (name, block numbers, expected static VALU, multiplier), multiplier in terms of
#   W = triangle passes (walk_wave_iters), S = shade executions (shade_wave_execs), T = W + S main-loop iterations,
#   N = triangles per pass, I = work items taken (paths_started / 512: 64 pixels x 8 samples, an estimate)
SPECS = {
    "generic": dict(symbol="trace_kernelILb0ELb1ELb0ELb0E", groups=[
        ("need ballot, votes, block choice", [2, 12, 66], 14, "T"),
        ("state copies at the loop's back edges", [9], 12, "T"),          # (one of the five copy blocks 9 / 10 / 11 / 91 / 229 per iteration)
        ("dealing units to lanes", [14, 16, 18, 58, 63], 87, "D"),
        ("taking a work item", [7, 21, 22, 27, 28, 30, 33, 36, 39, 41, 50, 55, 57], 311, "I"),
        ("pass prologue (ray pair, opacity keys)", [71], 49, "W"),
        ("triangle loop", [75], 63, "W*N"),
        ("triangle loop: hit updates", [83, 84], 6, "W*N*U"),
        ("triangle loop: opacity branch", [78, 80], 119, "0"),
        ("pass epilogue", [85, 87], 21, "W"),
        ("camera-ray block", [92, 99, 100, 104], 212, "0"),
        ("shade block: texture lookups", [135, 230, 231, 232], 153, "0"),
    ], shade=(106, 227)),
    "plain": dict(symbol="trace_kernelILb0ELb1ELb1ELb0E", groups=[
        ("need ballot, votes, block choice", [2, 10, 12, 67], 18, "T"),
        ("dealing units to lanes", [15, 17, 19, 59, 64], 87, "D"),
        ("taking a work item", [7, 22, 23, 28, 29, 31, 34, 37, 40, 42, 51, 56, 58], 306, "I"),
        ("triangle loop", [73, 75], 67, "W*N", 63),                        # (63 always + 2 + 2 hit-update moves behind execz)
        ("triangle loop: hit updates", [], 4, "W*N*U"),
        ("pass epilogue", [78, 80, 82], 15, "W"),
    ], shade=(86, 134)),
    # the same blocks up to the shade block, which is shorter: no specular-draw output, no reflect(), no mirror / lobe routes
    "lambert": dict(symbol="trace_kernelILb0ELb1ELb1ELb1E", groups=[
        ("need ballot, votes, block choice", [2, 10, 12, 67], 18, "T"),
        ("dealing units to lanes", [15, 17, 19, 59, 64], 87, "D"),
        ("taking a work item", [7, 22, 23, 28, 29, 31, 34, 37, 40, 42, 51, 56, 58], 305, "I"),
        ("triangle loop", [73, 75], 67, "W*N", 63),
        ("triangle loop: hit updates", [], 4, "W*N*U"),
        ("pass epilogue", [78, 80, 82], 15, "W"),
    ], shade=(86, 116)),
}


def main():
    path, which, stats_path = sys.argv[1], sys.argv[2], sys.argv[3]
    measured = float(sys.argv[4]) if len(sys.argv) > 4 else None
    spec = SPECS[which]
    st = json.load(open(stats_path))
    blk = blocks_of(path, spec["symbol"])
    prefixes = {m.group(0) for k in blk for m in [re.match(r"\.LBB\d+_", k)] if m}
    if len(prefixes) != 1:
        sys.exit(f"{spec['symbol']}: expected the blocks of one kernel, found label prefixes {sorted(prefixes)}")
    spec["prefix"] = prefixes.pop()
    num = lambda label: int(label[len(spec["prefix"]):]) if label.startswith(spec["prefix"]) and label[len(spec["prefix"]):].isdigit() else None
    W, S = st["walk_wave_iters"], st["shade_wave_execs"]
    N = st["tri_tests"] / max(1, st["rays"])                               # every ray of a pass meets every triangle
    env = dict(W=W, S=S, T=W + S, N=round(N), I=st["paths_started"] / 512.0)
    rows, claimed = [], set()
    for g in spec["groups"]:
        name, nums, expect, mult = g[:4]
        static = sum(blk[spec["prefix"] + str(n)] for n in nums) if nums else expect
        if static != expect:
            sys.exit(f"{name}: blocks {nums} hold {static} VALU, the group was derived for {expect}: the kernel was rebuilt, re-derive the groups")
        claimed.update(nums)
        if len(g) > 4:
            static = g[4]
        rows.append((name, static, mult))
    lo, hi = spec["shade"]
    shade_static = sum(v for k, v in blk.items() if num(k) is not None and lo <= num(k) <= hi and num(k) not in claimed)
    total_static = sum(blk.values())
    print(f"{which}: {spec['symbol']}  static VALU {total_static}   W {W}  S {S}  N {env['N']}  paths {st['paths_started']}")
    print(f"{'group':46s} {'static':>7s} {'x':>10s} {'dynamic lo':>12s} {'dynamic hi':>12s}")
    known_lo = known_hi = 0.0
    for name, static, mult in rows:
        # D (deal events): at least one per 64 paths started, at most one per main-loop iteration; U (share of loop iterations in
        # which some lane accepts a hit): 0 .. 1
        v_lo = static * eval(mult, dict(env, D=st["paths_started"] / 64.0, U=0.0))
        v_hi = static * eval(mult, dict(env, D=env["T"], U=1.0))
        known_lo += v_lo; known_hi += v_hi
        print(f"{name:46s} {static:7d} {mult:>10s} {v_lo / 1e9:12.4f} {v_hi / 1e9:12.4f}")
    print(f"{'shade block (static sum of reachable blocks)':46s} {shade_static:7d} {'S':>10s} {'':12s} {shade_static * S / 1e9:12.4f}")
    print(f"{'sum, G wave-instructions':46s} {'':7s} {'':10s} {known_lo / 1e9:12.4f} {(known_hi + shade_static * S) / 1e9:12.4f}")
    if measured:
        mid = 0.5 * (known_lo + known_hi)
        print(f"measured SQ_INSTS_VALU {measured / 1e9:.4f} G: triangle loops {63 * W * env['N'] / measured:.3f} of it; everything else "
              f"{(measured - 63 * W * env['N']) / 1e9:.4f} G; shade block inferred {(measured - known_hi) / S:.0f} .. {(measured - known_lo) / S:.0f} "
              f"VALU per execution (static bound {shade_static}); per traced path {measured * 64 / st['paths_started']:.0f} thread-instructions at full waves")
        print(json.dumps({"kernel": which, "measured": measured, "triangle_loops": 63 * W * env["N"], "known_mid": mid, "shade_inferred_per_exec": (measured - mid) / S}))


main()
