"""The surface-sampling unit as the compiler lowers it (csrc/ptk_surface.hip, csrc/Makefile): no device, one
`hipcc -S` of the unit with the Makefile's own command line (taken from `make -n`).

The rule of include/ptk.h is stated without contraction, so the unit must be built with -ffp-contract=off; and every kernel of it -
the weights, the quantiser, the two kernels of the prefix sum, the coarse table, the sampler with and without it - is held to no scratch
and no spills.  Metadata only (tools/isa_blocks.py Kernel.meta): no instruction is looked for."""
import importlib.util
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
KERNELS = ("surface_weights_kernel", "surface_check_weights_kernel", "surface_quantise_kernel", "surface_coarse_kernel",
           "scan_reduce_kernel", "scan_apply_kernel", "surface_sample_kernelILb0EEE", "surface_sample_kernelILb1EEE")


def _isa():
    spec = importlib.util.spec_from_file_location("isa_blocks", os.path.join(ROOT, "tools", "isa_blocks.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the unit's device assembly by the Makefile's command line for build/ptk_surface.o: -c -> --offload-device-only -S"""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "build/ptk_surface.o"], capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.split("\n") if "ptk_surface.hip" in l and " -c " in l]
    assert len(lines) == 1, out
    cmd = shlex.split(lines[0])
    dst = str(tmp_path_factory.mktemp("surface_unit") / "surface.s")
    cmd[cmd.index("-o") + 1] = dst
    cmd[cmd.index("-c")] = "-S"
    cmd.insert(1, "--offload-device-only")
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return dst, cmd


def test_the_unit_is_built_exact_and_holds_its_kernels(built):
    path, cmd = built
    assert "-ffp-contract=off" in cmd and "--offload-arch=gfx950" in cmd and not any(c.startswith("-DPTK_CONTRACT") for c in cmd)
    assert not any(c.startswith("-ffp-contract=") and c != "-ffp-contract=off" for c in cmd), cmd
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), re.M)
    assert len(names) == len(KERNELS), names
    for k in KERNELS:
        assert sum(k in n for n in names) == 1, (k, names)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spills(built, kernel):
    K = _isa().Kernel(built[0], kernel)
    m = K.meta
    print(f"{kernel}: {m}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_count"] + m.get("agpr_count", 0) <= 64, m               # (eight waves per SIMD: the sampler hides its probes' latency by occupancy)
