"""GPU box, one-off: many seeds of tests/plain_random_scenes.py's generator through the PLAIN trace kernels (not part of the suite).
python tools/soak_plain_scenes.py [first_seed] [count]
Sizes cycle through 1..16 triangles, the variant (0..10) and the level (generic / LAMBERT) go by the seed.  Every scene is rendered by
the cycle unit and under the six options that take a layer of the PLAIN code away (tests/plain_random_scenes.py OPTION_SETS), each
against the CPU oracle, accumulator and RGB8 bit for bit.  Prints a MISMATCH line per render that differs; exit status 1 if any did."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401  (first copy of the HIP runtime, as tests/conftest.py does)
from pbrpathtracer_amd import ptk
from oracle import oracle_binding as OB
import plain_random_scenes as P

first = int(sys.argv[1]) if len(sys.argv) > 1 else 100
count = int(sys.argv[2]) if len(sys.argv) > 2 else 200
OB.build()
ctx = ptk.Context(0)
bad = scenes = renders = 0
t0 = time.time()
for k in range(count):
    seed = first + k
    n = 1 + k % 16
    variant = seed % len(P.VARIANTS)
    lambert = bool((seed // 3) & 1)
    row = (seed, n, variant, lambert, 33 + (seed * 7) % 32, 17 + (seed * 5) % 32, 1 + seed % 8, 3 + seed % 9)
    arrays, cam = P.plain_scene(seed, n, variant, lambert)
    ref, ref8 = P.oracle_image(OB, arrays, cam, row)
    if not np.isfinite(ref).all():
        print(f"seed {seed}: oracle image not finite (n {n} variant {variant}): skipped", flush=True)
        continue
    scenes += 1
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_frame(row[4], row[5], row[6]); ctx.set_tile(0, 1)
    classes, prefix = P.classify(arrays)
    if ctx.flat_classes() != classes or ctx.flat_rect_pairs() != prefix:
        bad += 1
        print(f"MISMATCH seed {seed} n {n} variant {variant} lambert {int(lambert)} classification", flush=True)
    for name, value, back in (("default", 0, 0),) + P.OPTION_SETS:
        if name == "lambert_kernel" and not lambert:
            continue
        if name != "default": ctx.set_option(name, value)
        ctx.reset(); ctx.render(0, row[7], seed)
        ok = np.array_equal(ref.view(np.uint32), ctx.read_accum().view(np.uint32)) and np.array_equal(ref8, ctx.resolve_rgb8())
        if name != "default": ctx.set_option(name, back)
        renders += 1
        if not ok:
            bad += 1
            print(f"MISMATCH seed {seed} n {n} variant {variant} lambert {int(lambert)} {row[4]}x{row[5]} depth {row[6]} spp {row[7]} {name}", flush=True)
    if k % 25 == 24:
        print(f"seed {seed}: {scenes} scenes, {renders} renders, {bad} mismatches  [{time.time() - t0:.0f} s]", flush=True)
print(f"seeds {first}..{first + count - 1}: {scenes} scenes, {renders} renders, mismatches: {bad}")
ctx.close()
sys.exit(1 if bad else 0)
