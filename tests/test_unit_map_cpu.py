"""The cycle unit's work-unit mapping without a device (tests/cpp/unit_map_fuzz.cpp on the kernel's own header, csrc/ptk_unit_map.h):
unit_place / unit_pixel, the functions the deal of csrc/ptk_trace_cycle.h calls, over every item shape a launch can produce.

The program sweeps every live-pixel count 1 .. 64 with random live masks (the lowest and the highest bits first), chunk sizes 4 and 8
with a full and a short last chunk, and every split of an item's deal into rounds of 1 .. 64 needy lanes.  Every unit is dealt
exactly once and never to a dead pixel, its slot is base + s * 64 + q, s and q are the true quotient and the pixel of the true
remainder's rank, and pixel, sample and slot are what the voted kernels' deal computes; the program fails by itself when no item
with one live pixel or no partial last round was met."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "unit_map_fuzz.cpp")


def _build_and_run(tmp_path, name, flags, masks):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-I" + CSRC, SRC, "-o", exe] + flags)
    out = subprocess.run([exe, str(masks)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok") and "mismatches 0\n" in out.stdout, out.stdout[-3000:]
    m = re.search(r"items (\d+) \(with one live pixel: (\d+)\), units placed (\d+), partial last rounds (\d+)", out.stdout)
    # 64 live counts x masks x (chunk 4, chunk 8) x (full, short); each item dealt at 64 widths
    assert m and int(m.group(1)) == 64 * masks * 4 and int(m.group(2)) == masks * 4 and int(m.group(4)) > 0, out.stdout[-3000:]
    assert int(m.group(3)) >= 64 * int(m.group(1)), out.stdout[-3000:]
    return out.stdout


def test_every_unit_of_every_item_is_dealt_once_to_the_kernels_pixel_sample_and_slot(tmp_path):
    print(_build_and_run(tmp_path, "unit_map_fuzz", ["-O2"], 12))


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone host program: the sanitizers' runtime is linked into it, nothing is preloaded; fewer masks per live count"""
    _build_and_run(tmp_path, "unit_map_fuzz_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], 3)
