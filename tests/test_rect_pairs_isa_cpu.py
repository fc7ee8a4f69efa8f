"""The pair pass as the compiler lowers it (csrc/ptk_kernels_rect.hip, csrc/Makefile; DESIGN 4.1 "Fan-split rectangles"): no device,
one `hipcc -S` of the unit with the Makefile's own command line (taken from `make -n`).

ptk_flat_mt.h mt_rect_pair shares nothing by hand: it calls the triangle test's arithmetic twice, the second record's words named as
the first's, and leaves the sharing to common-subexpression elimination.  A compiler that did not share would still build a correct
library, so the assembly is held to what the unit is there for.  tools/isa_blocks.py walks the pair loop's route for each of the six
kinds from the loop header to the shared accept chain.

Operation counts: record A alone is 29 VALU instructions, B inside the pair 11 more (3 for u, 3 for q, 5 for v; nothing
for s, h, a, the reciprocal, t): 40 from the loop header to the accept for every kind.  The unit is built with the module inliner
(csrc/Makefile RECT_UNIT_FLAGS) for that: by the default inliner mt_pair<ZM> is simplified by itself before it is inlined, record
A's -(s_m * alpha) becomes s_m * (-alpha) there and no longer meets record B's s_m * alpha - kinds 1, 3, 5 then take 41, and
test_every_kinds_second_record_costs_at_most_the_predicted_count fails, as it does for a compiler that ignores the hidden option."""
import importlib.util
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
KERNELS = ("trace_kernel_rectILb0ELb1ELb1ELb1EEEv", "trace_kernel_rectILb0ELb1ELb1ELb0EEEv")      # LAMBERT level, generic PLAIN level
A_ALONE, B_IN_PAIR = 29, 11          # VALU instructions by operation count


def _isa():
    spec = importlib.util.spec_from_file_location("isa_blocks", os.path.join(ROOT, "tools", "isa_blocks.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the unit's device assembly by the Makefile's command line for build/ptk_kernels_rect.o: -c -> --offload-device-only -S"""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "build/ptk_kernels_rect.o"], capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.split("\n") if "ptk_kernels_rect.hip" in l and " -c " in l]
    assert len(lines) == 1, out
    cmd = shlex.split(lines[0])
    dst = str(tmp_path_factory.mktemp("rect_unit") / "rect.s")
    cmd[cmd.index("-o") + 1] = dst
    cmd[cmd.index("-c")] = "-S"
    cmd.insert(1, "--offload-device-only")
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return dst, cmd


def _pair_table(built, kernel):
    isa = _isa()
    K = isa.Kernel(built[0], kernel)
    table, _ = isa.route_table(K, isa.pair_header(K), range(1, 7))
    return isa, K, table


def test_the_unit_has_the_plain_units_flags_and_holds_the_two_kernels_only(built):
    path, cmd = built
    assert "-structurizecfg-skip-uniform-regions=1" in cmd and "-enable-tail-merge=0" in cmd and "-enable-module-inliner=1" in cmd
    assert "-ffp-contract=off" in cmd and "-fno-slp-vectorize" in cmd and not any(c.startswith("-DPTK_CONTRACT") for c in cmd)
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), re.M)
    assert len(names) == 2 and all(any(k in n for n in names) for k in KERNELS), names


@pytest.mark.parametrize("kernel", KERNELS)
def test_one_reciprocal_pair_per_rectangle_and_bodies_that_branch_straight_to_the_accept(built, kernel):
    isa, K, table = _pair_table(built, kernel)
    for kind in range(1, 7):
        t = table[kind]
        assert t["end"] == "latch" and t["flag_hops"] == 0 and t["branches_body_to_join"] <= 1, (kind, t)
        seq, _, _ = isa.route(K, kind, isa.pair_header(K))
        rcp = [i for i, _ in seq if K.ins[i][1].startswith("v_rcp_f32")]
        assert len(rcp) == 2, (kind, len(rcp))                      # one per ray: both records divide by the same determinant
    # the record loop behind it is the plain unit's: the zero classes' bodies
    rec, _ = isa.route_table(K)
    assert [rec[c]["valu"] for c in range(16)] == [49, 37, 37, 37] + [28] * 12
    # a turn of the pair loop, accept chain included, against the two turns of the record loop it replaces (three-zero records)
    two = 2 * rec[4]["whole_iteration"]["valu"]
    for kind in range(1, 7):
        w = table[kind]["whole_iteration"]
        assert w["valu"] < two, (kind, w, two)                      # (how much fewer: the next test)
        assert w["smem"] == 2                                      # v0 | e1yz e2xy and e2z | index: record A's words only


def test_every_kinds_second_record_costs_at_most_the_predicted_count(built):
    cost = {}
    for kernel in KERNELS:
        _, _, table = _pair_table(built, kernel)
        cost[kernel] = {kind: table[kind]["valu"] - A_ALONE for kind in range(1, 7)}
    print("VALU instructions of B inside a pair, by kind:", cost)
    assert all(c <= B_IN_PAIR for k in KERNELS for c in cost[k].values()), cost


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
    # the plain unit's five loops and the pair loop, which sits directly in the main loop in front of the record loop
    L = isa.loops(K)
    assert len(L) == 6 and all(len(l["back_edges"]) == 1 and l["exits"] == 1 for l in L), L
    assert [l["depth"] for l in L] == [1, 2, 2, 2, 3, 4]
    pp, ph = isa.pair_header(K)[0], isa.pass_header(K)[0]
    assert [l["depth"] for l in L if l["header_index"] in (pp, ph)] == [2, 2] and pp < ph
