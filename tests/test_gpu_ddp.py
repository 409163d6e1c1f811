"""Two ranks through FusedTrainStep on ONE GPU (both on cuda:0, gloo process group): the multi-rank control flow
(bucketed all-reduce on the side stream, global-count loss normalisation, a rank with an empty batch still joining
the exchange) must reproduce the single-rank step on the concatenated batch.  RCCL itself is exercised by the
driver's multi-GPU bench; here the point is the arithmetic and that no rank deadlocks."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_two_rank_fused_step_equals_one_rank_step(tmp_path, wire):
    """Both wire formats of the gradient exchange: fp32 (exact: == the one-rank step to 1e-5) and bf16 (BASELINE config 4's
    "bf16" all-reduce, half the bytes: within 1e-2 per tensor, both ranks bit-identical)."""
    ok = tmp_path / "ok"
    port = 29500 + os.getpid() % 2000
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(HERE, "ddp_worker.py"), str(ok), wire]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert ok.read_text() == "ok"


# A shared card admits CARD_PROCESS_LIMIT processes with it open at once.  The pytest process and the torch.distributed launcher
# (its torch.cuda.is_available() opens the device) are two of them, so at most RANKS_PER_CARD ranks share one card.
CARD_PROCESS_LIMIT = 6
RANKS_PER_CARD = CARD_PROCESS_LIMIT - 2


def _bf16_wire_trajectory(tmp_path, ranks, port_salt):
    """`ranks` ranks of ddp_worker.py's trajectory mode (rank r on cuda:r % visible GPUs, gloo), 12 optimizer steps: the full-batch
    loss after every step stays within 5e-3 of the one-rank run on the concatenated batch with the bf16 wire (fp32 wire: 1e-4), the
    ranks end bit-identical.  Bounds the growth of the wire rounding with ring length."""
    ok = tmp_path / "ok"
    port = 29500 + (os.getpid() + port_salt) % 2000
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(HERE, "ddp_worker.py"), str(ok), "trajectory"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert ok.read_text() == "ok"


def test_four_rank_bf16_wire_follows_the_one_rank_trajectory(tmp_path):
    """The opt-in bf16 wire format over a ring of 4 ranks sharing ONE GPU (the most one card takes): three partial sums per
    element on the wire where the two-rank tests have one."""
    _bf16_wire_trajectory(tmp_path, RANKS_PER_CARD, 1301)


def test_eight_rank_bf16_wire_follows_the_one_rank_trajectory(tmp_path):
    """The opt-in bf16 wire format at the largest world size of one node: 8 ranks dealt over the visible GPUs (rank r on
    cuda:r % n), at most RANKS_PER_CARD per card -- two cards or more."""
    import torch
    have = torch.cuda.device_count()
    if -(-8 // max(have, 1)) > RANKS_PER_CARD:
        pytest.skip(f"needs 2 GPUs (8 ranks, at most {RANKS_PER_CARD} per card), found {have}")
    _bf16_wire_trajectory(tmp_path, 8, 977)


def test_more_ranks_than_gpus_is_refused_not_hung():
    """bench.py --gpus 2 on a box with one GPU (and without the shared-GPU debugging switch): a clear refusal within seconds,
    not two ranks fighting over cuda:0 or a hang in the RCCL rendezvous."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has two GPUs: the refusal path is for 1-GPU boxes")
    env = {k: v for k, v in os.environ.items() if k != "SQ_BENCH_SHARE_GPU"}
    cmd = [sys.executable, os.path.join(os.path.dirname(HERE), "bench.py"), "--gpus", "2", "--workload", "vis_fwd", "--steps", "1", "--warmup", "0",
           "--no-cpu-baseline", "--no-secondary"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "needs 2 visible GPUs" in (r.stderr + r.stdout), (r.stdout[-500:], r.stderr[-1500:])


def _bench_kfold(tmp_path, gpus, batch, tag):
    import json
    dump = tmp_path / f"params_{tag}.pt"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SQ_BENCH_SHARE_GPU="1", SQ_BENCH_DUMP_PARAMS=str(dump))
    cmd = [sys.executable, os.path.join(os.path.dirname(HERE), "bench.py"), "--gpus", str(gpus), "--workload", "train_kfold", "--batch", str(batch),
           "--epochs", "1", "--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline", "--no-secondary"]      # --full: the `check` block
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1200)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, (r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(lines[-1]), dump


def test_config4_train_kfold_two_ranks_equal_one_rank_at_the_same_global_batch(tmp_path):
    """BASELINE config 4 (src/main.py:101-135,180-187 semantics) through bench.py itself at the model's real size
    (ViS D = 1024, depth 6, G = 20 820, bf16): two ranks of 16 slides (shared GPU, gloo -- the multi-process control flow and
    the bucketed exchange; RCCL is the driver's run) against ONE rank at the same global batch of 32.  Five folds run, both
    ranks end with identical parameters, and the parameters of the last fold agree with the one-rank run."""
    import torch
    two, p2 = _bench_kfold(tmp_path, 2, 16, "two")
    one, p1 = _bench_kfold(tmp_path, 1, 32, "one")
    assert two["ranks"] == 2 and two["backend"] == "gloo" and two["n_gpus"] == 2 and one["ranks"] == 1
    assert two["check"]["folds_run"] == 5 and one["check"]["folds_run"] == 5
    assert two["check"]["ranks_hold_identical_parameters"] is True
    ex = two["check"]["gradient_exchange_ms_per_step"]           # what a first multi-GPU run needs to explain its scaling
    assert ex is not None and ex["backward_ms"] > 0 and ex["allreduce_span_ms"] > 0 and one["check"]["gradient_exchange_ms_per_step"] is None
    # config 4 says bf16: a bf16 model exchanges bf16 buckets -- 2 bytes per parameter per step (107.5 MB at this size), not 4
    assert ex["wire_format"] == "bf16" and 100e6 < ex["bytes_exchanged_per_step"] < 115e6, ex
    assert two["config"]["slides"] == 32 and one["config"]["slides"] == 32
    a, b = torch.load(p2), torch.load(p1)
    d = (a - b).abs()
    rel_sum = abs(two["check"]["param_abs_sum"] - one["check"]["param_abs_sum"]) / one["check"]["param_abs_sum"]
    print(f"config 4, 2 ranks x 16 vs 1 rank x 32: param max diff {float(d.max()):.2e} mean {float(d.mean()):.2e}, abs-sum rel diff {rel_sum:.2e}; "
          f"{two['value']:.0f} vs {one['value']:.0f} slides/s")
    # AdamW at lr = 1e-3: a gradient whose sign differs between the two summation orders moves a parameter by up to 2 lr per step
    assert float(d.max()) < 5e-3 and float(d.mean()) < 2e-5 and rel_sum < 1e-4
