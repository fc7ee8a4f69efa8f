"""The hemisphere sampler's angle in float (csrc/ptk_angle_f32.h: what the cycle unit's shade block compiles instead of the double
form of csrc/ptk_device_fn.h) without a device: tests/cpp/angle_f32_sweep.cpp over ALL 2^24 u01 draws, built with -ffp-contract=off.

ang = fma(theta, c_hi, theta * c_lo) and r = fma(-k, p3, fma(-k, p2, fma(-k, p1, ang))) must give the bits of the double form's
ang, its quadrant k, the bits of its reduced argument r and the bits of the sine and cosine that leave sincos_2pi - zero mismatches
of each, stage by stage from the double form's own input and as one chain from the draw.  The five constants are the header's,
derived there from 2 pi and pi / 2 in double; the program prints them."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "angle_f32_sweep.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, SRC, "-o", exe] + flags)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok"), out.stdout[-3000:]
    assert "mismatches: ang 0, k 0, r 0, sin 0, cos 0, whole chain 0\n" in out.stdout, out.stdout[-3000:]
    m = re.search(r"draws (\d+), largest quadrant (\d+)", out.stdout)
    assert m and int(m.group(1)) == 1 << 24 and int(m.group(2)) == 4, out.stdout[-3000:]
    return out.stdout


def test_all_draws_give_the_double_forms_bits(tmp_path):
    out = _build_and_run(tmp_path, "angle_f32_sweep", ["-O2"])
    # the constants as derived: the float nearest 2 pi and pi / 2, and what is left of the doubles
    assert "c_hi 0x1.921fb6p+2 c_lo -0x1.777a5cp-23 p1 0x1.921fb6p+0 p2 -0x1.777a5cp-25 p3 " in out, out


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone host program: the sanitizers' runtime is linked into it, nothing is preloaded"""
    _build_and_run(tmp_path, "angle_f32_sweep_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
