"""The surface-attribute unit as the compiler lowers it (csrc/ptk_attributes.hip, csrc/Makefile): no device, one
`hipcc -S` of the unit with the Makefile's own command line (taken from `make -n`).

The rule of include/ptk.h is stated without contraction, so the unit must be built with -ffp-contract=off, as ptk_features.hip is;
and attributes_kernel is held to no scratch and no spills.  Metadata only (tools/isa_blocks.py Kernel.meta): no
instruction is looked for."""
import importlib.util
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
KERNELS = ("attributes_kernel",)


def _isa():
    spec = importlib.util.spec_from_file_location("isa_blocks", os.path.join(ROOT, "tools", "isa_blocks.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _command(unit):
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, f"build/{unit}.o"], capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.split("\n") if f"{unit}.hip" in l and " -c " in l]
    assert len(lines) == 1, out
    return shlex.split(lines[0])


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the unit's device assembly by the Makefile's command line for build/ptk_attributes.o: -c -> --offload-device-only -S"""
    cmd = _command("ptk_attributes")
    dst = str(tmp_path_factory.mktemp("attributes_unit") / "attributes.s")
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


def test_the_unit_is_on_the_feature_units_command_line(built):
    """one rule, one arithmetic: but for the file names the two units that call surface_attrs are compiled by the same command"""
    strip = lambda cmd, unit: [c.replace(unit, "UNIT") for c in cmd]
    assert strip(_command("ptk_attributes"), "ptk_attributes") == strip(_command("ptk_features"), "ptk_features")


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spills(built, kernel):
    K = _isa().Kernel(built[0], kernel)
    m = K.meta
    print(f"{kernel}: {m}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
