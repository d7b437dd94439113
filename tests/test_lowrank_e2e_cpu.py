"""Low-rank outer transport (``Diloco(lowrank=R)``, ``--comm-rank R``) over gloo with 2 and 3 workers: replica
equality, a falling loss on a fixed repeated batch, checkpoints (bit-exact resume, another R, a dense resume)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch


from . import _lowrank_checks as chk
from . import _outer_chains as oc
from ._mp import child_env, free_port, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ = 64


_two_steps = oc.lowrank_two_steps  # shared with tests/test_transports_multiworker_gpu.py


@pytest.mark.parametrize("world", [2, 3])
def test_replicas_equal_and_mean_residual_is_what_was_not_delivered(world):
    assert all(run_ranks(_two_steps, world, 128.0))


def test_several_buckets_per_round():
    assert all(run_ranks(_two_steps, 2, 0.01))


# ------------------------------------------------------------------------------------------ torchrun
def _dataset(tmp_path):
    """A fixed repeated batch: every window of the shard is the same 64 tokens."""
    from nanodiloco_amd.data.memmap import write_token_shard
    d = tmp_path / "data"
    d.mkdir()
    window = np.random.default_rng(0).integers(0, 256, SEQ)
    write_token_shard(str(d / "train.bin"), np.tile(window, 96), vocab_size=256)
    cfg = tmp_path / "tiny_gqa.json"
    cfg.write_text(json.dumps(dict(chk.TINY, architectures=["LlamaForCausalLM"], rms_norm_eps=1e-5)))
    return ["--llama-config-file", str(cfg), "--data", "memmap", "--dataset-path", str(d), "--batch-size", "8",
            "--per-device-batch-size", "4", "--seq-length", str(SEQ), "--warmup-steps", "2", "--wandb", "off",
            "--device", "cpu", "--debug-checks", "--total-steps", "8", "--inner-steps", "2", "--lr", "3e-3"]


def _torchrun(nproc, args, timeout=600):
    env = child_env(OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m", "nanodiloco_amd"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _losses(path):
    return [x["loss"] for x in map(json.loads, open(path)) if "loss" in x]


def _tensors(path):
    from safetensors.torch import load_file
    return load_file(str(path))


@pytest.mark.slow
def test_cli_two_workers_stop_resume_bitwise_and_resume_rules(tmp_path):
    """torchrun, 2 gloo workers, --comm-rank 4 --debug-checks on the tiny GQA Llama: the loss falls on the repeated
    batch, the run stopped after outer step 1 and resumed ends bit for bit where the uninterrupted one does (weights,
    residual, Q), a resume with another R re-seeds Q and keeps the residual, a dense resume ignores both."""
    base = _dataset(tmp_path)
    a, b, mid = tmp_path / "a", tmp_path / "b", tmp_path / "mid"
    la = tmp_path / "a.jsonl"
    r = _torchrun(2, base + ["--comm-rank", "4", "--checkpoint-dir", str(a), "--log-file", str(la)])
    assert "Training completed!" in r.stdout
    loss = _losses(la)
    assert len(loss) == 8 and all(np.isfinite(loss)) and loss[-1] < loss[0], loss
    _torchrun(2, base + ["--comm-rank", "4", "--stop-at-step", "2", "--checkpoint-dir", str(b), "--checkpoint-every", "1"])
    subprocess.run(["cp", "-r", str(b), str(mid)], check=True)
    _torchrun(2, base + ["--comm-rank", "4", "--resume", str(b), "--checkpoint-dir", str(b)])
    for f in ("model.safetensors", "diloco_state.safetensors", "rank0.safetensors", "rank1.safetensors"):
        ta, tb = _tensors(a / f), _tensors(b / f)
        assert ta.keys() == tb.keys()
        for key in ta:
            if not key.startswith("data."):
                assert torch.equal(ta[key], tb[key]), (f, key)
    state = json.load(open(a / "trainer_state.json"))
    assert state["comm_lowrank"]["rank"] == 4
    q = _tensors(mid / "diloco_state.safetensors")["lowrank.q"]
    saved = [_tensors(mid / f"rank{rk}.safetensors")["lowrank.residual"] for rk in (0, 1)]
    assert q.numel() > 0 and bool(torch.isfinite(q).all())
    # (every worker sees the same repeated batch, so the two residuals are the same here; different ones: above)
    assert all(t.numel() == state["flat_numel"] and bool((t != 0).any()) for t in saved)
    # another R: Q starts from Q0 again, the residual stays, and both are said
    c = tmp_path / "c"
    r = _torchrun(2, base + ["--comm-rank", "8", "--resume", str(mid), "--checkpoint-dir", str(c)])
    assert "re-seeded from the constant seed" in r.stdout and "kept, it is an amount still owed" in r.stdout
    assert json.load(open(c / "trainer_state.json"))["comm_lowrank"]["rank"] == 8
    # without the flag: the dense run of that state, the low-rank state is dropped with a line in the log
    r = _torchrun(2, base + ["--resume", str(mid)])
    assert "checkpoint holds low-rank transport state" in r.stdout and "ignored" in r.stdout


@pytest.mark.slow
def test_cli_three_workers_loss_falls(tmp_path):
    base = _dataset(tmp_path)
    log = tmp_path / "log.jsonl"
    r = _torchrun(3, base + ["--comm-rank", "4", "--log-file", str(log)])
    assert "Training completed!" in r.stdout
    loss = _losses(log)
    assert len(loss) == 8 and all(np.isfinite(loss)) and loss[-1] < loss[0], loss
