"""bench.py on the GPU: the multi-process entry point (launcher -> rank process -> TCP side channel -> RCCL communicator)
with ONE rank, which is all a one-GPU box can run (RCCL refuses two ranks on a device), and the plain single-process
line next to it.  Config 3 keeps it short.  The tests that read the natural solve or the measured ceilings run the benchmark
with --full (without the CPU baseline); the others run it plain."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(env_extra, *args, full=True):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                                            "TSCM_RDZV_PORT", "TSCM_BENCH_FORCE_DIST", "TSCM_BENCH_STUB")}
    env.update(env_extra)
    more = ("--full", "--no-cpu-baseline") if full else ()
    out = subprocess.run([sys.executable, BENCH, "--config", "3", "--steps", "20", "--warmup", "10", *more, *args],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_spawned_single_rank_matches_the_plain_run(hip_device):
    plain = _run({})
    dist = _run({"TSCM_BENCH_FORCE_DIST": "1"}, "--gpus", "1")
    assert plain["n_gpus"] == 1 and dist["n_gpus"] == 1
    assert dist["rccl_ranks"] == 1 and dist["exchange_ranks"] == 1      # ncclCommCount of the communicator the rank created
    assert plain["rccl_ranks"] == 0 and plain["exchange"] is None      # no communicator, no RCCL in the exchange
    assert 0 < plain["roofline"]["iteration_frac"] < plain["roofline"]["frac"]
    for d in (plain, dist):
        r = d["roofline"]
        assert r["launches"] > 0 and r["avg_launch_ms"] > 0
        assert r["peak_measured_mfma_f64"] > 5 and r["peak_measured_valu_f64"] > 5      # TFLOP/s, measured in the same process
        assert 0 < r["frac"] < 1 and 0 < r["frac_of_measured_ceiling"] < 1.5
        assert d["natural_solve"]["termination"] in ("Function tolerance reached.", "Parameter tolerance reached.", "Gradient tolerance reached.")
    # same solve, same decisions
    assert plain["natural_solve"]["iterations"] == dist["natural_solve"]["iterations"]
    assert abs(plain["natural_solve"]["rmse_px"] - dist["natural_solve"]["rmse_px"]) < 1e-12
    # the communicator path (separate control kernel + all-reduce of one rank) costs a few microseconds per iteration
    assert dist["value"] > 0.6 * plain["value"]


def test_more_ranks_than_gpus_fails_loudly(hip_device):
    from tscm_calib_amd import lib
    n = lib.lib().tscm_device_count()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, BENCH, "--config", "3", "--gpus", str(n + 1), "--steps", "5"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    assert "needs" in out.stderr and "GPUs" in out.stderr
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_two_rank_processes_on_one_device_over_the_ipc_exchange(hip_device):
    """`bench.py --gpus 2` end to end -- launcher, side channel, communicator, barriers, max over ranks, rank 0's JSON line -- with
    both rank processes on THIS device: TSCM_BENCH_EXCHANGE=ipc selects the library's IPC exchange back-end (RCCL refuses two
    ranks on one device).  Same natural solve as the plain run; the line says what it is."""
    plain = _run({})
    two = _run({"TSCM_BENCH_EXCHANGE": "ipc"}, "--gpus", "2")
    assert two["n_gpus"] == 2 and two["exchange"] == "ipc" and two["exchange_ranks"] == 2
    assert two["rccl_ranks"] == 0                                   # RCCL carried nothing in this run: the line must not say it saw 2 ranks
    assert "rank processes on" in two["config"]["parallelism"]
    assert len(two["per_rank"]) == 2 and len(two["corners_per_rank"]) == 2
    assert two["natural_solve"]["iterations"] == plain["natural_solve"]["iterations"]
    assert abs(two["natural_solve"]["rmse_px"] - plain["natural_solve"]["rmse_px"]) < 1e-9
    assert two["value"] > 0


def test_ipc_rank_processes_reproduce_the_local_group_bit_for_bit(hip_device):
    """tools/ipc_check.py: 2 and 4 rank PROCESSES on this device (rendezvous, handle exchange, hipIpcOpenMemHandle, arrival
    flags between kernels of different processes, the board gather through the communicator) against the same shards in one
    process through the LOCAL group: iteration log and final parameters, bit for bit."""
    tool = os.path.join(os.path.dirname(BENCH), "tools", "ipc_check.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, tool, "--world", "2,4", "--config", "3", "--iterations", "10"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert [l["world"] for l in lines] == [2, 4]
    for l in lines:
        assert l["identical"] and l["iterations"] == 10
        assert set(l["fingerprint_ipc_ranks"]) == {l["fingerprint_local_group"]}


def test_the_drivers_torchrun_command_with_two_ranks_on_this_device(hip_device):
    """`python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P bench.py --gpus 2 ...`
    -- the command the driver uses for N > 1 -- with both ranks on this device over the IPC exchange: one JSON line, from rank 0."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["TSCM_BENCH_EXCHANGE"] = "ipc"
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), BENCH, "--gpus", "2", "--config", "3", "--steps", "20", "--warmup", "5"],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["n_gpus"] == 2 and d["steps"] == 20 and d["warmup"] == 5 and d["exchange"] == "ipc" and len(d["per_rank"]) == 2
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6


def test_a_rank_that_is_gone_is_reported_not_waited_for(hip_device):
    """Failure detection of the IPC exchange: one of two rank processes leaves before the solve; the other's exchange kernel gives
    up after its bound (10 s) and the solve returns TSCM_E_PEER (ABI 6: its own code, RCCL had no part in it) -- the exchanges enqueued
    behind the failed one return at once, and the communicator is unusable afterwards."""
    tool = os.path.join(os.path.dirname(BENCH), "tools", "ipc_check.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, tool, "--world", "2", "--config", "1", "--iterations", "10", "--die-rank", "1"], env=env, capture_output=True, text=True, timeout=300)
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.stdout + out.stderr)[-3000:]
    assert lines[0]["peer_failure_detected"] and lines[0]["code"] == -7 and 5 < lines[0]["seconds"] < 60
    assert lines[0]["again_code"] == -7 and lines[0]["again_seconds"] < 2.0


def test_dump_outputs_are_what_the_timed_solve_computes(hip_device, tmp_path):
    """--dump-outputs: the arrays of the last timed solve (config 3, --steps 20: one solve of 20 forced iterations) against the
    same solve run here through the API from the same start -- what a caller of the timed path receives.  A plain run (no
    --full): its line has the headline fields and the dominant kernel's HIP-event figures, and none of what --full adds."""
    import numpy as np
    import bench
    from tscm_calib_amd import api, synth
    d = _run({}, "--dump-outputs", str(tmp_path), full=False)
    assert d["steps"] == 20
    assert d["unit"] == "LM iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6
    assert d["roofline"]["launches"] > 0 and d["roofline"]["avg_launch_ms"] > 0 and d["roofline"]["traffic"] is None
    assert not {"natural_solve", "cpu_baseline"} & set(d)
    assert not [k for k in d["roofline"] if k.startswith("peak_measured") or "measured_ceiling" in k or "measured_floor" in k]
    got = {n[:-4]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert all(a.dtype == np.float64 for a in got.values())
    with api.Solver(synth.make_config(3), device=hip_device) as s:
        s.upload_params()
        want = s.solve_resident(reset=True, max_num_iterations=20, **bench.BENCH_OPTS)
        cam_rt, intr, board_rt = s.download_params()
    assert want["lm_iterations"] == 20 and len(got["iteration_cost"]) == want["num_iterations"]
    assert np.array_equal(got["iteration_step_is_successful"], [it["step_is_successful"] for it in want["iterations"]])
    assert np.allclose(got["iteration_cost"], [it["cost"] for it in want["iterations"]], rtol=1e-9, atol=0)
    assert abs(got["final_cost"][0] - want["final_cost"]) <= 1e-9 * want["final_cost"]
    assert np.allclose(got["cam_rt"], cam_rt, rtol=0, atol=1e-8 * max(np.max(np.abs(cam_rt)), 1.0))
    assert np.allclose(got["board_rt"], board_rt, rtol=0, atol=1e-8 * np.max(np.abs(board_rt)))
    assert np.max(np.abs(got["intr"][:, :7] - intr[:, :7]) / np.abs(intr[:, :7])) < 1e-4
