"""The K-nearest kernel as the compiler lowers it (csrc/ptk_knearest.hip, csrc/Makefile): no device, one `hipcc -S` of
the unit with the Makefile's own command line (taken from `make -n`).

The list of a lane is a pair of arrays indexed by unrolled loops only.  An index the compiler could not resolve would move the list
to scratch memory and still give a correct library, many times slower, so every instantiation's metadata is held to no scratch and
no spills.  Metadata only (tools/isa_blocks.py Kernel.meta): no instruction is looked for."""
import importlib.util
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
LISTS = (1, 4, 16)
KINDS = [(kt, stats) for kt in LISTS for stats in (0, 1)]          # nearest_kernel<KT, STATS>


def _isa():
    spec = importlib.util.spec_from_file_location("isa_blocks", os.path.join(ROOT, "tools", "isa_blocks.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the unit's device assembly by the Makefile's command line for build/ptk_knearest.o: -c -> --offload-device-only -S"""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "build/ptk_knearest.o"], capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.split("\n") if "ptk_knearest.hip" in l and " -c " in l]
    assert len(lines) == 1, out
    cmd = shlex.split(lines[0])
    dst = str(tmp_path_factory.mktemp("knearest_unit") / "knearest.s")
    cmd[cmd.index("-o") + 1] = dst
    cmd[cmd.index("-c")] = "-S"
    cmd.insert(1, "--offload-device-only")
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return dst, cmd


def _name(kt, stats):
    return f"nearest_kernelILi{kt}ELb{stats}EEE"


def test_the_unit_is_built_exact_and_holds_the_six_instantiations(built):
    path, cmd = built
    assert "-ffp-contract=off" in cmd and "--offload-arch=gfx950" in cmd and not any(c.startswith("-DPTK_CONTRACT") for c in cmd)
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), re.M)
    assert len(names) == len(KINDS) and all("nearest_kernel" in n for n in names), names
    for kt, stats in KINDS:
        assert sum(_name(kt, stats) in n for n in names) == 1, (kt, stats, names)


@pytest.mark.parametrize("kt,stats", KINDS)
def test_no_scratch_and_no_spills(built, kt, stats):
    K = _isa().Kernel(built[0], _name(kt, stats))
    m = K.meta
    print(f"nearest_kernel<{kt}, {bool(stats)}>: {m}")
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_count"] + m.get("agpr_count", 0) <= 512, m
    # the group segment is the stack alone: (PTK_MAX_BVH_DEPTH + 1) rows of 64 links
    txt = open(built[0]).read()
    lds = re.search(r"\.amdhsa_kernel\s+" + re.escape(K.name) + r"\s.*?\.amdhsa_group_segment_fixed_size\s+(\d+)", txt, re.S)
    depth = int(re.search(r"#define PTK_MAX_BVH_DEPTH (\d+)", open(os.path.join(ROOT, "include", "ptk.h")).read()).group(1))
    assert int(lds.group(1)) == (depth + 1) * 64 * 4, (lds.group(1), depth)
