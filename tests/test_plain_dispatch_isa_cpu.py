"""The class switch of the exact PLAIN pass as the compiler lowers it (csrc/ptk_kernels_plain.hip, csrc/Makefile PLAIN_UNIT_FLAGS;
DESIGN 4.1 "The pass"): no device, one `hipcc -S` of the unit with the Makefile's own command line (taken from `make -n`).

The unit is built with -mllvm -structurizecfg-skip-uniform-regions=1 so that the pass's wave-uniform 16-way switch stays a tree of
s_cmp / s_cbranch_scc pairs whose bodies branch straight to the accept chain.  Without it the backend structurizes the tree: every
subtree sets a 64-bit flag and every level is left through `s_andn2_b64 vcc, exec, flag` + `s_cbranch_vccnz`, four such hops per
triangle of a Cornell box.  The option is a hidden one: a compiler that silently ignores it would still build a correct library, so
the assembly is held to what the option is there for, and the same checks must fail on the unit as the common command line builds it
(the second test).  tools/isa_blocks.py follows each class's route from the loop header to the join by interpreting the scalar
compares, flag moves and flag tests along it."""
import importlib.util
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
KERNELS = ("trace_kernelILb0ELb1ELb1ELb1EEEv", "trace_kernelILb0ELb1ELb1ELb0EEEv")      # LAMBERT level, generic PLAIN level
C2_CLASSES = (13, 14, 9, 10, 8, 11, 9, 10, 5, 4, 7, 6)       # the Cornell box of bench config C2 (tests/test_flat_zero_classes_cpu.py holds the scene to them)


def _isa():
    spec = importlib.util.spec_from_file_location("isa_blocks", os.path.join(ROOT, "tools", "isa_blocks.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _assembly(tmp_path, name, make_vars=()):
    """the unit's device assembly by the Makefile's command line for build/ptk_kernels_plain.o: -c -> --offload-device-only -S"""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "build/ptk_kernels_plain.o"] + list(make_vars), capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.split("\n") if "ptk_kernels_plain.hip" in l and " -c " in l]
    assert len(lines) == 1, out
    cmd = shlex.split(lines[0])
    k = cmd.index("-o")
    dst = str(tmp_path / name)
    cmd[k + 1] = dst
    cmd[cmd.index("-c")] = "-S"
    cmd.insert(1, "--offload-device-only")
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return dst, cmd


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return _assembly(tmp_path_factory.mktemp("plain_unit"), "plain.s")


def test_the_unit_is_built_with_the_option_and_holds_the_two_kernels_only(built):
    path, cmd = built
    assert "-structurizecfg-skip-uniform-regions=1" in cmd and cmd[cmd.index("-structurizecfg-skip-uniform-regions=1") - 1] == "-mllvm"
    assert "-ffp-contract=off" in cmd and "-fno-slp-vectorize" in cmd and not any(c.startswith("-DPTK_CONTRACT") for c in cmd)
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), re.M)
    assert len(names) == 2 and all(any(k in n for n in names) for k in KERNELS), names
    # ... and the common unit no longer emits them (one definition of each in the library)
    src = open(os.path.join(CSRC, "ptk_kernels.hip")).read()
    assert "#define PTK_PLAIN_UNIT" not in src and "PTK_PLAIN_UNIT" in src


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_body_branches_straight_to_the_accept_chain(built, kernel):
    isa = _isa()
    K = isa.Kernel(built[0], kernel)
    table, _ = isa.route_table(K)
    for c in range(16):
        t = table[c]
        assert t["end"] == "latch", (c, t["end"])
        assert t["flag_hops"] == 0, (c, t)                       # no s_cbranch_vcc* fed by s_andn2_b64 vcc, exec, flag on the way
        assert t["branches_body_to_join"] <= 1, (c, t)           # at most one unconditional branch between the body and the chain
        assert t["cbranch"] == 4, (c, t)                         # the four compare pairs, nothing else conditional
    # the bodies are the zero classes': three-zero 28, plane-only 37, general 49 VALU up to the join
    assert [table[c]["valu"] for c in range(16)] == [49, 37, 37, 37] + [28] * 12
    # one pass over the box of C2: the counts DESIGN 5 predicts the scalar counters from
    assert sum(table[c]["flag_hops"] for c in C2_CLASSES) == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_registers_scratch_and_control_flow(built, kernel):
    isa = _isa()
    K = isa.Kernel(built[0], kernel)
    m = K.meta
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    # five waves per SIMD (PTK_TRACE_WAVES_PLAIN): 512 registers per lane, allocated in eights
    assert (m["vgpr_count"] + m.get("agpr_count", 0) + 7) // 8 * 8 * 5 <= 512, m
    # every divergent region is closed on every route, whatever uniform branches it crosses
    bad, n, _ = isa.check_exec_regions(K)
    assert n > 20 and bad == [], bad
    # main loop, deal loop and its inner loops, pass loop: one back edge and one exit each; the pass sits directly in the main loop
    L = isa.loops(K)
    assert len(L) == 5 and all(len(l["back_edges"]) == 1 and l["exits"] == 1 for l in L), L
    ph = isa.pass_header(K)[0]
    assert [l["depth"] for l in L if l["header_index"] == ph] == [2] and [l["depth"] for l in L] == [1, 2, 2, 3, 4]


def test_the_checks_fail_on_the_common_command_line(tmp_path):
    """the same unit without PLAIN_UNIT_FLAGS is the parent's build of the two kernels: flag hops on every route"""
    path, cmd = _assembly(tmp_path, "plain_common.s", ["PLAIN_UNIT_FLAGS="])
    assert not any("structurizecfg" in c for c in cmd)
    isa = _isa()
    for kernel in KERNELS:
        table, _ = isa.route_table(isa.Kernel(path, kernel))
        assert all(table[c]["flag_hops"] >= 2 for c in range(16)), [table[c]["flag_hops"] for c in range(16)]
        assert sum(table[c]["flag_hops"] for c in C2_CLASSES) == 48           # four hops per triangle of the box
