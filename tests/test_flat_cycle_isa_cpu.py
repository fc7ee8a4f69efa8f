"""The cycle unit as the compiler lowers it (csrc/ptk_kernels_cycle.hip, csrc/ptk_trace_cycle.h, csrc/Makefile; DESIGN 4.1 "The
cycle unit"): no device, one `hipcc -S` of the unit with the Makefile's own command line (taken from `make -n`), and one of the pair
unit (csrc/ptk_kernels_rect.hip) by its own, to set the two kernels' deals side by side.

What the unit is there for is control, so the assembly is held to that: the pass and the shade block keep their counts (a turn of the
pair loop at most 68 VALU with a body of at most 41 - the unit is built without the module inliner, kinds 1, 3 and 5 keep one
product twice - and the record loop's bodies 49 / 37 / 28), nothing spills, every masked region closes, and on the static route from
the pass's latch through one deal of one round to the first instruction of the shade block (tools/isa_blocks.py deal_route) the new
kernel executes fewer VALU instructions and waits for LDS / scalar memory fewer times than the pair unit's kernel does on its route.
The two counts are printed; nothing is asserted against a number chosen in advance."""
import importlib.util
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
LEVELS = ("ILb0ELb1ELb1ELb1EEEv", "ILb0ELb1ELb1ELb0EEEv")              # LAMBERT level, generic PLAIN level
TURN_VALU, BODY_VALU = 68, 41


def _isa():
    spec = importlib.util.spec_from_file_location("isa_blocks", os.path.join(ROOT, "tools", "isa_blocks.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _assembly(tmp, unit):
    """the unit's device assembly by the Makefile's command line for build/<unit>.o: -c -> --offload-device-only -S"""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "build/%s.o" % unit], capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.split("\n") if unit + ".hip" in l and " -c " in l]
    assert len(lines) == 1, out
    cmd = shlex.split(lines[0])
    dst = str(tmp / (unit + ".s"))
    cmd[cmd.index("-o") + 1] = dst
    cmd[cmd.index("-c")] = "-S"
    cmd.insert(1, "--offload-device-only")
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return dst, cmd


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cycle_unit")
    return _assembly(tmp, "ptk_kernels_cycle"), _assembly(tmp, "ptk_kernels_rect")


def test_the_unit_has_the_plain_units_flags_alone_and_holds_the_two_kernels_only(built):
    (path, cmd), _ = built
    assert "-structurizecfg-skip-uniform-regions=1" in cmd and "-enable-tail-merge=0" in cmd and "-enable-module-inliner=1" not in cmd
    assert "-ffp-contract=off" in cmd and "-fno-slp-vectorize" in cmd and not any(c.startswith("-DPTK_CONTRACT") for c in cmd)
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), re.M)
    assert len(names) == 2 and all(any("trace_kernel_cycle" + k in n for n in names) for k in LEVELS), names
    # ... and CYCLE_UNIT_FLAGS reaches its command line (the A/B arm with the module inliner)
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "build/ptk_kernels_cycle.o", "CYCLE_UNIT_FLAGS=-mllvm -enable-module-inliner=1"],
                         capture_output=True, text=True, check=True).stdout
    assert [l for l in out.split("\n") if "ptk_kernels_cycle.hip" in l and "-enable-module-inliner=1" in l], out


@pytest.mark.parametrize("level", LEVELS)
def test_registers_scratch_and_masked_regions(built, level):
    isa = _isa()
    K = isa.Kernel(built[0][0], "trace_kernel_cycle" + level)
    m = K.meta
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    # five waves per SIMD (PTK_TRACE_WAVES_PLAIN): 512 registers per lane, allocated in eights; 102 scalar registers
    assert (m["vgpr_count"] + m.get("agpr_count", 0) + 7) // 8 * 8 * 5 <= 512 and m["sgpr_count"] <= 102, m
    bad, n, _ = isa.check_exec_regions(K)
    assert n > 20 and bad == [], bad
    # the pair loop stands directly in the main loop, in front of the record loop
    L = isa.loops(K)
    pp, ph = isa.pair_header(K)[0], isa.pass_header(K)[0]
    assert [l["depth"] for l in L if l["header_index"] in (pp, ph)] == [2, 2] and pp < ph, L
    assert all(len(l["back_edges"]) == 1 for l in L), L


@pytest.mark.parametrize("level", LEVELS)
def test_the_pass_keeps_its_counts(built, level):
    isa = _isa()
    K = isa.Kernel(built[0][0], "trace_kernel_cycle" + level)
    header = isa.pair_header(K)
    table, _ = isa.route_table(K, header, range(1, 7))
    turn = {kind: table[kind]["whole_iteration"]["valu"] for kind in range(1, 7)}
    body = {kind: table[kind]["valu"] for kind in range(1, 7)}
    print(level, "pair loop, VALU of a whole turn by kind:", turn, "header to accept:", body)
    assert all(table[k]["end"] == "latch" and table[k]["flag_hops"] == 0 for k in range(1, 7)), table
    assert all(v <= TURN_VALU for v in turn.values()) and all(v <= BODY_VALU for v in body.values()), (turn, body)
    rec, _ = isa.route_table(K)
    assert [rec[c]["valu"] for c in range(16)] == [49, 37, 37, 37] + [28] * 12


@pytest.mark.parametrize("level", LEVELS)
def test_one_deal_costs_fewer_vector_instructions_and_fewer_waits_than_the_pair_units(built, level):
    isa = _isa()
    new = isa.Kernel(built[0][0], "trace_kernel_cycle" + level)
    old = isa.Kernel(built[1][0], "trace_kernel_rect" + level)
    _, cn = isa.deal_route(new)
    _, co = isa.deal_route(old)
    print(level, "pass latch -> one deal of one round -> shade block, pair unit:", co)
    print(level, "pass latch -> one deal of one round -> shade block, cycle unit:", cn)
    assert cn["valu"] < co["valu"] and cn["lgkm_waits"] < co["lgkm_waits"], (cn, co)
    # the deal's control is scalar: no divergent loop on the route (no s_andn2_b64 exec, exec, <mask> bookkeeping), one table read
    route, _ = isa.deal_route(new)
    assert not [new.ins[i] for i in route if new.ins[i][1] == "s_andn2_b64" and new.ins[i][2][0] == "exec"]
    assert cn["lds"] == 1, cn
