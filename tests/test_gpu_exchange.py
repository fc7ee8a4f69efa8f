"""The multi-GPU exchange step on the one GPU a test box has.  The product path is native (ptk_gather_accum: pack kernel
-> grouped ncclSend / ncclRecv on the library's own RCCL communicator -> unpack kernel on the root); here
  * a one-rank communicator runs that whole path end to end (RCCL refuses two ranks on one device),
  * the pack / unpack kernels are checked against the library's host-side packing order (ptk_packed_layout) with this
    one GPU playing every rank of 1-, 2-, 3- and 8-way splits of a ragged frame,
  * the overlap contract (the exchange snapshots the accumulator; the next render may be queued at once) is checked,
  * bench.py's N > 1 control flow is rehearsed with two gloo ranks, started by bench.py itself (no torchrun).
The N = 2 / 3 arithmetic of the same packing order runs on CPU in tests/test_distributed_cpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, scene_from_golden

pytestmark = pytest.mark.gpu

W, H = 70, 50          # ragged: 5 x 4 tiles, last column / row partial


def _ctx(width=W, height=H):
    from pbrpathtracer_amd import ptk
    z = load_golden("tier_s_cornell.npz")
    c = ptk.Context(0)
    c.upload_scene(scene_from_golden(z))
    cam, proj = z["cam"], z["proj"]
    c.set_camera(cam[0:3], cam[3:6], cam[6:9], float(proj[0]), float(proj[1]), float(z["focal_dist"]), float(z["aperture"]))
    c.set_frame(width, height, 4)
    return c


def test_pack_and_unpack_kernels_follow_the_library_layout():
    from pbrpathtracer_amd import ptk
    c = _ctx()
    c.reset(); c.render(0, 6, 3)
    accum = c.read_accum()
    flat = accum.reshape(-1)
    assert flat.any()
    for world in (1, 2, 3, 8):
        packed = []
        for r in range(world):
            lay = ptk.packed_layout(W, H, r, world)
            got = c.probe_pack(r, world)
            exp = np.where(lay >= 0, flat[np.maximum(lay, 0)], np.float32(0.0))
            assert np.array_equal(got, exp), (world, r)
            packed.append(got)
        image = c.probe_unpack(world, np.concatenate(packed))
        assert np.array_equal(image, accum), world           # every pixel written, bit for bit (the probe pre-fills NaNs)
    c.close()


def test_native_gather_one_rank_communicator_and_overlap():
    """ptk_comm_init + ptk_gather_accum + ptk_read_gathered through a one-rank RCCL communicator; the gathered image is
    the accumulator AS IT WAS when the exchange was issued, while rendering carries on."""
    from pbrpathtracer_amd import ptk
    c = _ctx()
    assert c.L.ptk_gather_accum(c.h, None, 0) != 0          # no communicator yet: an error, not a crash
    assert b"communicator" in c.L.ptk_last_error(c.h)
    c.comm_init(ptk.comm_unique_id(), 0, 1)
    c.reset(); c.render(0, 5, 11)
    c.gather_accum(0)
    c.render(5, 3, 11)                                      # queued at once: overlaps the exchange
    first = c.read_gathered()
    ref5 = _ctx(); ref5.reset(); ref5.render(0, 5, 11)
    assert np.array_equal(first, ref5.read_accum())
    ref8 = _ctx(); ref8.reset(); ref8.render(0, 8, 11)
    assert np.array_equal(c.read_accum(), ref8.read_accum())    # the local accumulator kept accumulating
    c.gather_accum(0); c.gather_wait()
    assert np.array_equal(c.read_gathered(), ref8.read_accum())
    with pytest.raises(ptk.PtkError):
        c.gather_accum(1)                                   # root outside the group
    # the gathered image belongs to the frame it was combined for: after a resolution change it is refused, not mis-read
    c.set_frame(W + 32, H + 16, 4)
    with pytest.raises(ptk.PtkError, match="another resolution"):
        c.read_gathered()
    c.set_frame(W, H, 4)
    assert np.array_equal(c.read_gathered(), ref8.read_accum())
    c.comm_destroy()
    c.close(); ref5.close(); ref8.close()


def test_bench_exchange_on_one_gpu():
    """bench.py --force-exchange --full: the N > 1 code path (communicator, exchange every K steps and after the last,
    checksum) with one rank."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C1", "--steps", "5", "--warmup", "1",
                        "--full", "--force-exchange", "--exchange-every", "2", "--no-cpu-baseline", "--no-other-configs"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["config"]["exchange_every"] == 2 and d["config"]["exchanges_in_timed_region"] == 3      # steps 2, 4 and the last
    assert "native packed RCCL gather" in d["config"]["exchange"]
    assert d["roofline"]["bound"] in ("valu", "l2_miss_fabric") and 0 < d["roofline"]["frac"] < 1
    assert 0 < d["traced_samples_per_s"] <= d["value"]
    assert d["config"]["rccl_ranks"] == 1 and d["config"]["devices"] == [0]      # ncclCommCount of the library's own communicator
    assert d["parity"]["ok"] is True and d["parity"]["exact_fraction"] == 1.0


def test_bench_two_ranks_rehearsal_self_launched():
    """`python bench.py --gpus 2 --full` as the driver runs it - NOT under torchrun: bench.py starts its two ranks itself (child
    process, before it touches the GPU) and relays rank 0's line.  Two ranks must share this box's one GPU, which RCCL
    refuses, so the rehearsal backend (gloo, exchange through host copies in the library's packing order) stands in; the
    gathered image must hold exactly what the two ranks hold together."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--config", "C1", "--backend", "gloo", "--exchange-every", "2", "--full", "--no-cpu-baseline", "--with-c5"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "C1 gathered-image checksum OK" in r.stderr and "C5 gathered-image checksum OK" in r.stderr, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines                                            # ONE line: rank 0's result
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["parallelism"] == "tile-split x2" and d["config"]["exchanges_in_timed_region"] == 2
    # the self-proving fields: what the library's own communicator reports (none in the gloo rehearsal), the distinct HIP
    # ordinals the ranks rendered on (both ranks share this box's one GPU), the exchange's checksum
    assert "rccl_ranks" in d["config"] and d["config"]["rccl_ranks"] is None and d["config"]["devices"] == [0]
    assert d["config"]["gathered_checksum"]["ok"] is True
    # image parity beside the number, and the contracted build next to the exact one
    assert d["parity"]["ok"] is True and d["parity"]["exact_fraction"] == 1.0 and d["parity"]["pixels"] > 0
    assert d["value_contracted"]["value"] > 0 and d["value_contracted"]["parity"]["ok"] is True
    # BASELINE config 5 as stated - the 1 M-triangle frame tile-split over the ranks with the exchange in the timed region
    c5 = d["other_configs"]["C5"]
    assert c5["n_gpus"] == 2 and c5["value"] > 0 and c5["triangles"] >= 1000000 and c5["config"]["gathered_checksum"]["ok"] is True
    assert c5["config"]["exchanges_in_timed_region"] == 1 and c5["parity"]["ok"] is True


def test_bench_rank_absent_at_the_exchange_ends_the_run_within_the_bound():
    """a rank that renders but never enters the exchange step (PTK_BENCH_FAULT: it stops right before its first
    gather) must end `bench.py --gpus 2` with a non-zero exit inside the bound - rank 0's wait on the gather times out
    (--rank-timeout), torch.distributed.run ends the other rank, the parent names the failure and prints no result line."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["PTK_BENCH_FAULT"] = "absent:1:exchange"
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--config", "C1",
                        "--backend", "gloo", "--exchange-every", "1", "--no-cpu-baseline", "--rank-timeout", "10", "--wall-limit", "300"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    took = time.time() - t0
    assert r.returncode != 0 and took < 280, (r.returncode, took, r.stderr[-3000:])
    assert '"metric"' not in r.stdout
    assert "FAULT INJECTED: absent at exchange" in r.stderr and "a rank failed or timed out" in r.stderr, r.stderr[-3000:]


def test_native_gather_wait_is_bounded():
    """ptk_gather_wait / ptk_comm_init never wait for ever: with comm_timeout_s set to a fraction of a second a communicator whose
    second rank never joins is refused with PTK_ERR_RCCL naming rank, world and device (the helper thread that sits in
    ncclCommInitRank is abandoned; this test runs it in a child process that is ended afterwards)."""
    code = (
        "import sys, time; sys.path.insert(0, %r)\n"
        "from pbrpathtracer_amd import ptk\n"
        "ctx = ptk.Context(0)\n"
        "ctx.set_option('comm_timeout_s', 0.5)\n"
        "uid = ptk.comm_unique_id()\n"
        "t0 = time.time()\n"
        "try:\n"
        "    ctx.comm_init(uid, 0, 2)\n"
        "    print('JOINED')\n"
        "except ptk.PtkError as e:\n"
        "    print('REFUSED in %%.1f s: %%s' %% (time.time() - t0, e))\n"
        "sys.stdout.flush()\n"
        "import os; os._exit(0)\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert "REFUSED" in r.stdout and "rank 0 of 2" in r.stdout and "waited" in r.stdout, (r.stdout, r.stderr[-2000:])


def test_native_gather_wait_times_out_on_a_step_that_does_not_complete():
    """The bound INSIDE ptk_gather_wait, on one GPU: the exchange stream is kept busy for 3 s (ptk_debug_stall_exchange) ahead of an
    exchange step, and comm_timeout_s is 0.3 s - the wait must come back with PTK_ERR_RCCL naming step, rank, root and the bytes
    outstanding well before the stream drains, the communicator is gone afterwards (aborted), no gathered image is left to read
    (ptk_read_gathered and ptk_gathered_device_ptr refuse rather than hand out a partial or stale one), and a fresh one gathers the
    right image again.  In a child process under a time limit: a wait that is not bounded would otherwise hang the suite."""
    code = (
        "import sys, time; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from pbrpathtracer_amd import ptk\n"
        "from test_gpu_exchange import _ctx\n"
        "c = _ctx(); c.comm_init(ptk.comm_unique_id(), 0, 1)\n"
        "c.reset(); c.render(0, 4, 11)\n"
        "c.gather_accum(0); c.gather_wait(); c.synchronize()\n"        # step 1: allocates the exchange buffers (which synchronises)
        "c.set_option('comm_timeout_s', 0.3)\n"
        "c.debug_stall_exchange(3000)\n"
        "c.gather_accum(0)\n"
        "t0 = time.time()\n"
        "try:\n"
        "    c.gather_wait(); print('WAITED %%.2f s' %% (time.time() - t0))\n"
        "except ptk.PtkError as e:\n"
        "    print('REFUSED in %%.2f s: %%s' %% (time.time() - t0, e))\n"
        "for name in ('read_gathered', 'gathered_device_ptr'):\n"      # a failed exchange leaves no gathered image to read
        "    try:\n"
        "        getattr(c, name)(); print('STALE IMAGE FROM %%s' %% name)\n"
        "    except ptk.PtkError as e:\n"
        "        print('NO IMAGE FROM %%s: %%s' %% (name, e))\n"
        "try:\n"
        "    c.gather_accum(0); print('GATHERED WITHOUT A COMMUNICATOR')\n"
        "except ptk.PtkError as e:\n"
        "    print('AFTERWARDS: %%s' %% e)\n"
        "c.synchronize()\n"
        "c.set_option('comm_timeout_s', 60)\n"
        "c.comm_init(ptk.comm_unique_id(), 0, 1)\n"
        "c.gather_accum(0); g = c.read_gathered()\n"
        "print('RECOVERED' if np.array_equal(g, c.read_accum()) else 'WRONG IMAGE AFTER RECOVERY')\n"
        "print('DEVICE VIEW %%d bytes' %% c.gathered_device_ptr()[1])\n"
        "sys.stdout.flush()\n"
        "import os; os._exit(0)\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    out = r.stdout
    assert "REFUSED in" in out and "timed out" in out and "step 2 on rank 0 of 1 (root 0)" in out and "still expecting" in out, (out, r.stderr[-2000:])
    waited = float(out.split("REFUSED in ")[1].split(" s")[0])
    assert 0.3 <= waited < 1.5, out
    assert "AFTERWARDS:" in out and "communicator" in out.split("AFTERWARDS:")[1].splitlines()[0], out
    for name in ("read_gathered", "gathered_device_ptr"):
        assert f"NO IMAGE FROM {name}:" in out and "no gathered image" in out.split(f"NO IMAGE FROM {name}:")[1].splitlines()[0], (out, r.stderr[-2000:])
    assert "RECOVERED" in out, (out, r.stderr[-2000:])
    assert f"DEVICE VIEW {W * H * 12} bytes" in out, out


def test_native_gather_between_two_gpus(tmp_path):
    """The N > 1 branch of ptk_gather_accum (grouped ncclSend / ncclRecv on the library's own communicator, exchange
    stream next to persistent trace waves) with two real ranks: two fresh child processes, one GPU each, render their
    tiles of a frame and gather; the root's gathered image must equal a single-GPU render bit for bit.  Skipped on boxes
    with one GPU (the driver's test box): until it has run somewhere, DESIGN.md keeps saying "unmeasured on hardware"."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    out = str(tmp_path)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "two_gpu_rank.py"), str(r), "2", out], cwd=ROOT, env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill(); o, _ = p.communicate()
        logs.append(o)
    assert all(p.returncode == 0 for p in procs), "\n".join(x[-2000:] for x in logs)
    gathered = np.load(os.path.join(out, "gathered.npy"))
    c = _ctx(200, 136)
    c.reset(); c.render(0, 6, 17); c.render(6, 4, 17)
    assert np.array_equal(gathered, c.read_accum())
    c.close()
