#!/usr/bin/env python3
"""CPU only, not a test: the cross-check of the named census (Oracle.render_census, tests/trace_arms.py) by the compiler's own
branch coverage.  Builds oracle/pt_oracle.c with `gcc -O0 --coverage` into a temporary directory, renders every scene of the
registry through it (the census render, index order and tree walk as the registry says, so that every function of the counted
path runs), and and through the plain render, and prints the branches `gcov -b` reports as taken 0 times in tex2d ... trace.  What it prints beyond
the arms argued unreachable in tests/trace_arms.py is an arm the census has no name for, or one no scene drives.

    python tools/oracle_gcov.py            # from the repository root
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

FUNCTIONS = ("tex2d_impl", "test_triangle_impl", "closest_hit_impl", "closest_hit_census", "sample_about_impl", "direct_illumination_impl",
             "shade_impl", "trace_census")


def render_with(lib):
    import conftest  # noqa: F401  (torch first, as the tests load it)
    from oracle import oracle_binding as OB
    import trace_arms as TA
    OB.LIB_PATH = lib
    OB.build = lambda force=False: lib
    total, _ = TA.census(OB)
    # ... and through the plain render: the always-inlined bodies exist once per caller, and gcov lists each copy's branches
    for name, arrays, cam, W, H, D, spp, seed, _ in TA.registry():
        o = OB.Oracle(arrays)
        o.render(OB.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"]),
                 W, H, D, 0, spp, seed, threads=1)
        o.close()
    print("census arms at zero under every kernel:", sorted(k for k in total["BVH"] if not any(total[v][k] for v in TA.VARIANTS)))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--render-with":
        return render_with(sys.argv[2])
    tmp = tempfile.mkdtemp(prefix="oracle_gcov_")
    try:
        for f in ("pt_oracle.c", "pt_oracle.h"):
            shutil.copy(os.path.join(ROOT, "oracle", f), tmp)
        lib = os.path.join(tmp, "libptoracle_cov.so")
        # always_inline bodies are attributed to their own lines; one thread, so that the counters are not raced
        subprocess.check_call(["gcc", "-std=c99", "-O0", "--coverage", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-c", "pt_oracle.c"],
                              cwd=tmp)
        subprocess.check_call(["gcc", "--coverage", "-shared", "-o", lib, "pt_oracle.o", "-lm"], cwd=tmp)
        # the renders run in a child: its exit writes the counters
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--render-with", lib], cwd=ROOT)
        out = subprocess.run(["gcov", "-b", "-c", "pt_oracle.c"], cwd=tmp, check=True, capture_output=True, text=True).stdout
        text = open(os.path.join(tmp, "pt_oracle.c.gcov")).read().splitlines()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    # walk the annotated source: remember the enclosing function and the last source line, report `branch N never executed` / `taken 0`
    func = None; src = ""; lineno = 0; n = 0
    for line in text:
        m = re.match(r"\s*[-#=\d*]+:\s*(\d+):(.*)", line)
        if m:
            lineno, raw = int(m.group(1)), m.group(2)
            src = raw.strip()
            d = re.match(r"(?:ORC_INLINE|static|int|void|float|const)\b[^;=]*?\b(\w+)\(", raw)      # a definition starts in column 0
            if d:
                func = d.group(1)
            continue
        # `never executed` is a copy no render goes through (closest_hit_brute's, the probes'); a block no scene enters shows as
        # `taken 0` on the branch that leads to it
        m = re.match(r"branch\s+(\d+) (taken 0)", line)
        if m and func in FUNCTIONS:
            if re.search(r"\bif \(cz\b|ARM\(|cz\[|cz \?", src):
                continue                                   # the census' own plumbing
            print(f"{func}:{lineno}: branch {m.group(1)} {m.group(2)}: {src[:110]}"); n += 1
    print(f"{n} untaken branches in {', '.join(FUNCTIONS)}")
    print(out.splitlines()[1] if len(out.splitlines()) > 1 else out)


if __name__ == "__main__":
    main()
