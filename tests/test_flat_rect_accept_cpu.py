"""The pair pass's accept as one update per ray, without a device (tests/cpp/flat_rect_accept_fuzz.cpp on the kernels' own header,
csrc/ptk_flat_mt.h): mt_rect_accept_once - hit = X & (inA | inB), first = inA, the form tri_accept_rect runs as wave masks - against
mt_rect_accept, the sequential rule that tests/cpp/flat_rect_fuzz.cpp holds to the pass.

The program takes the full cross product of fifteen directed values over the nine float inputs (+-0, +-the smallest denormal, +-eps
and eps's neighbours, 1 and its neighbours, +-infinity, NaNs of either sign: t == best_t, t == eps, |a| == eps, uv == 1, a point
inside both records, u = -0, a NaN anywhere) and four million random draws; the two functions must agree on every one, and the
program fails by itself when the named cases are not met."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "flat_rect_accept_fuzz.cpp")


def _build_and_run(tmp_path, name, flags, values, draws):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-pthread", "-I" + CSRC, SRC, "-o", exe] + flags)
    out = subprocess.run([exe, str(values), str(draws)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok") and out.stdout.count("mismatches 0\n") == 3, out.stdout[-3000:]
    m = re.search(r"directed: (\d+) values per input, (\d+) cases", out.stdout)
    assert m and int(m.group(1)) == values and int(m.group(2)) == values ** 9, out.stdout[-3000:]
    assert re.search(r"random: %d draws" % draws, out.stdout), out.stdout[-3000:]
    return out.stdout


def test_one_update_per_ray_decides_as_the_sequential_rule(tmp_path):
    print(_build_and_run(tmp_path, "flat_rect_accept_fuzz", ["-O2"], 15, 4000000))


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone host program: the sanitizers' runtime is linked into it, nothing is preloaded; a smaller product (nine values:
    both signs of zero, eps with a neighbour, 1 with both, a negative, a NaN)"""
    _build_and_run(tmp_path, "flat_rect_accept_fuzz_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], 9, 400000)
