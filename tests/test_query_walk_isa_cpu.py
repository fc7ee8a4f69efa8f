"""The one-wave ray queries on the shared prologue and walk (csrc/ptk_query_walk.h) as the compiler lowers them: the kernels of
csrc/ptk_crossings.hip and csrc/ptk_hits.hip (csrc/Makefile), and closest_kernel's two instantiations
(csrc/ptk_closest.hip), which have the prologue from there and their node arm from csrc/ptk_point_walk.h.  No device: one
`hipcc -S` per unit with the Makefile's own command line (taken from `make -n`), as tests/test_multihit_isa_cpu.py does for the
multi-hit unit.

The prologue borrows rows of the traversal stack for staging and the walk's callable triangle arm must fold into the kernel: a
lambda capture the compiler could not resolve, or staging memory of the prologue's own, would still give a correct library.  So every
kernel's metadata is held to no scratch, no spills and a group segment that is the stack alone.  Metadata only (tools/isa_blocks.py
Kernel.meta): no instruction is looked for."""
import importlib.util
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
# (closest_kernel<STATS> by its mangled names: one template's two instantiations)
UNITS = {"ptk_crossings": ("crossings_kernel", "contains_kernel"), "ptk_hits": ("hits_kernel", "occluded_kernel"),
         "ptk_closest": ("closest_kernelILb0EEE", "closest_kernelILb1EEE")}
KERNELS = [(u, k) for u, ks in UNITS.items() for k in ks]


def _isa():
    spec = importlib.util.spec_from_file_location("isa_blocks", os.path.join(ROOT, "tools", "isa_blocks.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """unit -> (its device assembly, the command): the Makefile's command line for build/<unit>.o with -c -> --offload-device-only -S"""
    got = {}
    for unit in UNITS:
        out = subprocess.run(["make", "-n", "-B", "-C", CSRC, f"build/{unit}.o"], capture_output=True, text=True, check=True).stdout
        lines = [l for l in out.split("\n") if unit + ".hip" in l and " -c " in l]
        assert len(lines) == 1, out
        cmd = shlex.split(lines[0])
        dst = str(tmp_path_factory.mktemp(unit) / (unit + ".s"))
        cmd[cmd.index("-o") + 1] = dst
        cmd[cmd.index("-c")] = "-S"
        cmd.insert(1, "--offload-device-only")
        r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        got[unit] = (dst, cmd)
    return got


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_the_unit_is_built_exact_and_holds_its_two_kernels(built, unit):
    path, cmd = built[unit]
    assert "-ffp-contract=off" in cmd and "--offload-arch=gfx950" in cmd and not any(c.startswith("-DPTK_CONTRACT") for c in cmd)
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), re.M)
    assert len(names) == len(UNITS[unit]), names
    for k in UNITS[unit]:
        assert sum(k in n for n in names) == 1, (k, names)


@pytest.mark.parametrize("unit,kernel", KERNELS)
def test_no_scratch_no_spills_and_the_stack_alone_in_lds(built, unit, kernel):
    path = built[unit][0]
    K = _isa().Kernel(path, kernel)
    m = K.meta
    print(f"{kernel}: {m}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    # the group segment is the stack alone, (PTK_MAX_BVH_DEPTH + 1) rows of 64 links: the prologue stages through its rows
    txt = open(path).read()
    lds = re.search(r"\.amdhsa_kernel\s+" + re.escape(K.name) + r"\s.*?\.amdhsa_group_segment_fixed_size\s+(\d+)", txt, re.S)
    depth = int(re.search(r"#define PTK_MAX_BVH_DEPTH (\d+)", open(os.path.join(ROOT, "include", "ptk.h")).read()).group(1))
    assert int(lds.group(1)) == (depth + 1) * 64 * 4, (lds.group(1), depth)
