"""The cycle unit's shade block as the compiler lowers it (csrc/ptk_kernels_cycle.hip; csrc/ptk_device_fn.h ldg_at, sqrt_ieee_pos;
csrc/ptk_angle_f32.h; DESIGN 4.1 "The shade block's addressing"): no device, one `hipcc -S` of the unit with the Makefile's own
command line, as tests/test_flat_cycle_isa_cpu.py takes it.

For trace_kernel_cycle at both levels: no double-precision instruction and no v_mad_i64_i32 anywhere; the 64-bit shifts and
shift-adds that remain are pinned to their count and their places - the item acquisition and the deal in front of the shade block,
and the two sample stores, which keep 64-bit addressing on purpose (the C2 sample buffer is 3.77 GB); every load of the shade block
takes its base from an SGPR pair; nothing spills and the register budgets hold.

And the host rule that goes with the 32-bit offsets (csrc/ptk_table_offset.h) at its edge: tests/cpp/table_offset_edge.cpp."""
import importlib.util
import os
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
LEVELS = {"lambert": "ILb0ELb1ELb1ELb1EEEv", "generic": "ILb0ELb1ELb1ELb0EEEv"}
VGPRS = {"lambert": 72, "generic": 78}
SGPRS = 102
# what the built kernels have, each level alike:
#   v_lshlrev_b64   2: both in the kernel's prologue, the lane's bit and the mask of the lanes below it (1 << lane, -1 << lane)
#   v_lshl_add_u64 14: 12 in acquire_work_item (the queue counters' and the live list's addresses, the 64-bit item arithmetic), all
#                      in front of the shade block; 2 are the address of samples_u[out_idx] for the sample stores of
#                      PTK_FINISH_PATH, one in the shade block (a path that ends there) and one behind the pass (a miss)
LSHLREV_B64, LSHL_ADD_U64, LSHL_ADD_U64_STORES = 2, 14, 2


def _isa():
    spec = importlib.util.spec_from_file_location("isa_blocks", os.path.join(ROOT, "tools", "isa_blocks.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the unit's device assembly by the Makefile's command line for build/ptk_kernels_cycle.o: -c -> --offload-device-only -S"""
    tmp = tmp_path_factory.mktemp("shade_addressing")
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "build/ptk_kernels_cycle.o"], capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.split("\n") if "ptk_kernels_cycle.hip" in l and " -c " in l]
    assert len(lines) == 1, out
    cmd = shlex.split(lines[0])
    dst = str(tmp / "ptk_kernels_cycle.s")
    cmd[cmd.index("-o") + 1] = dst
    cmd[cmd.index("-c")] = "-S"
    cmd.insert(1, "--offload-device-only")
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert not any(c.startswith("-DPTK_SHADE32") for c in cmd), cmd         # (no switch: the forms are the unit's)
    return dst


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_no_double_and_no_64_bit_multiply_add_and_the_remaining_64_bit_shifts_are_where_they_belong(built, level):
    isa = _isa()
    K = isa.Kernel(built, "trace_kernel_cycle" + LEVELS[level])
    ops = [op for _, op, _ in K.ins]
    base = lambda op: op[:-4] if op.endswith(("_e32", "_e64")) else op
    assert not [op for op in ops if base(op).endswith("_f64")], sorted(set(op for op in ops if base(op).endswith("_f64")))
    assert "v_mad_i64_i32" not in ops
    shade = isa.shade_start(K)
    shifts = [i for i, op in enumerate(ops) if op == "v_lshlrev_b64"]
    adds = [i for i, op in enumerate(ops) if op == "v_lshl_add_u64"]
    print(level, "v_lshlrev_b64 at lines", [K.ins[i][0] for i in shifts], "v_lshl_add_u64 at lines", [K.ins[i][0] for i in adds],
          "shade block from line", K.ins[shade][0])
    assert len(shifts) == LSHLREV_B64 and len(adds) == LSHL_ADD_U64, (len(shifts), len(adds))
    # the prologue's lane masks: in front of the main loop's first LDS read of the deal, far in front of the shade block
    assert all(i < 100 and i < shade for i in shifts), shifts
    behind = [i for i in adds if i >= shade]
    assert len(behind) == LSHL_ADD_U64_STORES and all(i < shade for i in adds if i not in behind)
    for i in behind:
        # the sample store's address: samples_u + out_idx * 16, consumed by the next memory instruction, a 16-byte store
        dst = K.ins[i][2][0]
        assert K.ins[i][2][2] == "4", K.ins[i]
        nxt = [K.ins[j] for j in range(i + 1, min(i + 8, len(K.ins))) if K.ins[j][1].startswith(("global_", "flat_", "buffer_"))][0]
        assert nxt[1] == "global_store_dwordx4" and nxt[2][0] == dst and nxt[2][-1] == "off", (K.ins[i], nxt)
    # every load from the shade block on (the shade block's tables, the pass's records) has a scalar base and a 32-bit offset
    loads = [K.ins[i] for i in range(shade, len(K.ins)) if K.ins[i][1].startswith("global_load")]
    assert len(loads) >= 15 and all(l[2][-1].split()[0].startswith("s[") and not l[2][1].startswith("v[") for l in loads), loads
    assert not [op for op in ops if op.startswith(("flat_", "scratch_"))]


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_no_scratch_no_spills_and_the_register_budgets(built, level):
    isa = _isa()
    m = isa.Kernel(built, "trace_kernel_cycle" + LEVELS[level]).meta
    print(level, m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["vgpr_count"] + m.get("agpr_count", 0) <= VGPRS[level] and m["sgpr_count"] <= SGPRS, m


def test_the_hosts_rule_for_tables_of_four_gib_at_its_edge(tmp_path):
    exe = str(tmp_path / "table_offset_edge")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "table_offset_edge.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
