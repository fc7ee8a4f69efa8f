"""The cycle unit's square roots as the compiler lowers them (csrc/ptk_device_fn.h sqrt_ieee_rsq; DESIGN 4.1 "The cycle unit's roots"): no
device, one `hipcc -S` of the unit with the Makefile's own command line as tests/test_flat_cycle_isa_cpu.py takes it.  Every hot sqrt_ieee
site of the shade block - from its range test's compare to the end of the block that test guards - holds one v_rsq_f32, no v_sqrt_f32,
no v_cndmask and that one compare, an unsigned integer one; the v_sqrt_f32 left in the kernel stand in the never-taken expansions."""
import importlib.util
import os
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
LEVELS = ("ILb0ELb1ELb1ELb1EEEv", "ILb0ELb1ELb1ELb0EEEv")              # LAMBERT level, generic PLAIN level


# ---- the unit's assembly ---------------------------------------------------------------------------------------------------------------
def _isa():
    spec = importlib.util.spec_from_file_location("isa_blocks", os.path.join(ROOT, "tools", "isa_blocks.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the unit's device assembly by the Makefile's command line for build/ptk_kernels_cycle.o: -c -> --offload-device-only -S"""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "build/ptk_kernels_cycle.o"], capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.split("\n") if "ptk_kernels_cycle.hip" in l and " -c " in l]
    assert len(lines) == 1, out
    cmd = shlex.split(lines[0])
    dst = str(tmp_path_factory.mktemp("cycle_sqrt") / "cycle.s")
    cmd[cmd.index("-o") + 1] = dst
    cmd[cmd.index("-c")] = "-S"
    cmd.insert(1, "--offload-device-only")
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return dst


def _base(op):
    return op.replace("_e64", "").replace("_e32", "")


def _sqrt_sites(K):
    """every v_rsq_f32 of the kernel with its site: from the compare that writes the mask of the s_and_saveexec_b64 in front of it to the
    instruction that ends the block the mask guards (the next write of exec or branch)"""
    sites = []
    for i, (_, op, _) in enumerate(K.ins):
        if _base(op) != "v_rsq_f32":
            continue
        g = max(j for j in range(i) if K.ins[j][1] == "s_and_saveexec_b64")
        mask = K.ins[g][2][1]
        c = max(j for j in range(g) if K.ins[j][1].startswith("v_cmp") and K.ins[j][2][0] == mask)
        e = min(j for j in range(i, len(K.ins)) if K.ins[j][1].startswith("s_cbranch") or K.ins[j][1] == "s_branch"
                or (K.ins[j][1].startswith("s_") and "exec" in K.ins[j][1]) or (K.ins[j][2] and K.ins[j][2][0] == "exec"))
        sites.append([_base(K.ins[j][1]) for j in range(c, e)])
    return sites


@pytest.mark.parametrize("level", LEVELS)
def test_a_hot_square_root_is_one_rsq_behind_one_integer_compare(built, level):
    isa = _isa()
    K = isa.Kernel(built, "trace_kernel_cycle" + level)
    sites = _sqrt_sites(K)
    print(level, len(sites), "sites:", [len([o for o in s if o.startswith("v_")]) for s in sites], "VALU each")
    # 1 - w * w, u_su and the two normalisations of a diffuse bounce; the generic level has its specular routes' beside them
    assert len(sites) >= 4, sites
    for s in sites:
        assert s.count("v_rsq_f32") == 1 and "v_sqrt_f32" not in s and not [o for o in s if o.startswith("v_cndmask")], s
        cmps = [o for o in s if o.startswith("v_cmp")]
        assert len(cmps) == 1 and cmps[0].endswith("_u32"), s
        assert len([o for o in s if o in ("v_fma_f32", "v_fmac_f32")]) == 2 and s.count("v_mul_f32") == 2, s      # g = x * y, h = y / 2; the residual and its correction
    # ... and every v_sqrt_f32 left in the kernel stands in a never-taken expansion: as many as there are sites, none inside one
    assert len([1 for _, op, _ in K.ins if _base(op) == "v_sqrt_f32"]) == len(sites)
