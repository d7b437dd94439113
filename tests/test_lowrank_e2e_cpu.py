"""Low-rank outer transport (``Diloco(lowrank=R)``, ``--comm-rank R``) over gloo with 2 and 3 workers: replica
equality, a falling loss on a fixed repeated batch, checkpoints (bit-exact resume, another R, a dense resume)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
from nanodiloco_amd.parallel.diloco import Diloco
from nanodiloco_amd.parallel.dist import init_distributed
from nanodiloco_amd.parallel.transports import LowRankTransport

from . import _lowrank_checks as chk
from ._mp import child_env, free_port, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, MU = 0.7, 0.9
SEQ = 64


def _two_steps(rank, world, bucket_mb):
    """Every worker drifts on its own; after each outer step theta_sync and the master are the same bits everywhere,
    the residuals are each worker's own, and their mean is what the step did not deliver: with the first step's
    momentum (buf = d) theta moved by lr (1 + mu) d, so mean_w(acc_w) - mean_w(e_w) = d must reproduce it."""
    env = init_distributed("gloo")
    m = LlamaForCausalLM(LlamaConfig(**chk.TINY)).init_weights(7)
    dl = Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store, lr=LR, momentum=MU), 2, 8, 4, env=env,
                comm_dtype=torch.float32, lowrank=4, bucket_mb=bucket_mb)
    assert isinstance(dl.transport, LowRankTransport)
    st, plan = m.store, dl.transport.plan
    mask, comp = chk.covered(plan, st.numel)
    tmask = torch.from_numpy(mask)
    w1, w2 = dl.transport.wire1.numel(), dl.transport.wire2.numel()
    assert dl.bytes_per_outer_step == 4 * (w1 + w2)
    assert (dl.buckets_per_outer_step > 2) == (bucket_mb < 1)
    for s in range(2):
        drifts = [0.01 * torch.randn(st.numel, generator=torch.Generator().manual_seed(100 * s + j)) * tmask
                  for j in range(world)]
        theta = dl.sync.clone()
        st.master.add_(drifts[env.worker])
        dl.outer_step()
        dl.check_replicas(tol=0.0)
        assert torch.equal(st.master, dl.sync) and bool(torch.isfinite(st.master).all())
        e = dl.lowrank_residual
        assert bool(e[torch.from_numpy(comp)].any()) and not bool(e[~torch.from_numpy(comp)].any())
        if s == 0:
            es = [torch.zeros_like(e) for _ in range(world)]
            torch.distributed.all_gather(es, e)
            assert not torch.equal(es[0], es[1])
            acc = torch.stack([-d for d in drifts]).double().mean(0)  # sync - master of worker j is -drift_j
            d = acc - torch.stack(es).double().mean(0) * torch.from_numpy(comp)
            moved = (theta - dl.sync).double()
            # theta is rounded once where it is written (half an ulp of |theta|, taken as 2^-22 max|theta| with
            # room for the two fma), d and the residuals carry fp32 roundings relative to the step itself
            tol = 2.0 ** -22 * float(theta.abs().max()) + 1e-6 * float(moved.abs().max())
            assert float((moved - LR * (1 + MU) * d).abs().max()) <= tol
    assert dl.outer_comm.stats.calls == 2 * dl.buckets_per_outer_step
    return True


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
