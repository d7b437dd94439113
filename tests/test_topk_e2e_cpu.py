"""Top-k sparse outer transport (``Diloco(topk=K)``, ``--comm-topk K``) over gloo against the in-test oracle of
tests/_topk_oracle.py, its option rules, its checkpoints and the CLI."""
import json
import os
import subprocess
import sys

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.main import parse_args
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
from nanodiloco_amd.parallel.diloco import Diloco, _check_options
from nanodiloco_amd.parallel.dist import init_distributed
from nanodiloco_amd.parallel.transports import DenseTransport, TopKTransport

from . import _outer_chains as oc
from . import _topk_checks as chk
from ._mp import child_env, free_port, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(hidden_size=32, intermediate_size=64, num_attention_heads=2, num_hidden_layers=1, vocab_size=50,
            rms_norm_eps=1e-5)
LR, MU = 0.7, 0.9
SIGMA = 0.01


def _mk(comm=torch.float32, topk=7, inner_dp=1, seed=7, env=None, **kw):
    env = env or init_distributed("gloo", inner_dp=inner_dp)
    m = LlamaForCausalLM(LlamaConfig.from_dict(TINY)).init_weights(seed)
    dl = Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store, lr=LR, momentum=MU), 2, 8, 4, env=env,
                comm_dtype=comm, topk=topk, **kw)
    return env, m, dl


def _drift(n, step, worker):
    return SIGMA * torch.randn(n, generator=torch.Generator().manual_seed(100 * step + worker))


def _no_dist_env():
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)


# ------------------------------------------------------------------------------------- 1. the oracle's steps
_chain = oc.topk_chain  # shared with tests/test_transports_multiworker_gpu.py


@pytest.mark.parametrize("comm", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("world", [2, 3])
def test_two_steps_match_oracle_bitwise(world, comm):
    assert all(run_ranks(_chain, world, comm, 7, 1, 128.0))


def test_several_buckets_three_workers():
    # 3 slots of two chunks each: 2 * 64 * (2 + 2) bytes per slot
    assert all(run_ranks(_chain, 3, torch.bfloat16, 64, 1, (3 * 2 * 64 * 4 + 3 * 32) / (1 << 20)))


def test_two_level_shards_the_span():
    assert all(run_ranks(_chain, 4, torch.bfloat16, 7, 2, 128.0))


def _offloaded(rank, world):
    """The host-offloaded snapshot goes through ``_sync_on_device()``: the same bits as the device-resident one."""
    env, m, dl = _mk(torch.bfloat16, 64)
    _, m2, dl2 = _mk(torch.bfloat16, 64, env=env, offload_snapshot=True)
    for s in range(2):
        for mm, dd in ((m, dl), (m2, dl2)):
            mm.store.master.add_(_drift(mm.store.numel, s, env.worker))
            dd.outer_step()
        assert torch.equal(m.store.master, m2.store.master) and torch.equal(dl.sync, dl2.sync)
        assert torch.equal(dl.topk_residual, dl2.topk_residual) and dl2.sync.device.type == "cpu"
        dl2.check_replicas(tol=0.0)
    return True


def test_offloaded_snapshot_same_bits():
    assert all(run_ranks(_offloaded, 2))


# ------------------------------------------------------------------------------------- 2. degenerate equivalence
def test_k_4096_fp32_equals_dense_transport_one_worker():
    _no_dist_env()
    env, m, dl = _mk(torch.float32, 4096)
    _, m2, dl2 = _mk(torch.float32, 0, env=env)
    assert isinstance(dl.transport, TopKTransport) and isinstance(dl2.transport, DenseTransport)
    chk.check_degenerate(m, dl, m2, dl2)


# ------------------------------------------------------------------------------------- 3. rules
def test_rules_through_diloco():
    _no_dist_env()
    for k in (-1, 4097):
        with pytest.raises(ValueError, match="topk"):
            _mk(topk=k)
    for comm in ("int8", "int4", torch.int8):
        with pytest.raises(ValueError, match="int8 / int4"):
            _mk(comm)
    with pytest.raises(ValueError, match="error_feedback"):
        _mk(error_feedback=True)
    with pytest.raises(ValueError, match="overlap"):
        _mk(overlap=True)
    with pytest.raises(ValueError, match="fragments"):
        _mk(fragments=1, stream_overlap=0)
    net = torch.nn.Linear(4, 4)
    with pytest.raises(ValueError, match="ModuleDiloco"):
        Diloco(net, torch.optim.AdamW(net.parameters(), lr=1e-3), torch.optim.SGD(net.parameters(), lr=0.7), 0, 10,
               topk=4)
    assert _check_options(True, torch.bfloat16, topk=4096) == 0 and _check_options(True, torch.float32, topk=1) == 0
    # off by default: the dense transport, and no residual anywhere
    _, _, dl = _mk(topk=0)
    assert isinstance(dl.transport, DenseTransport) and not hasattr(dl, "topk_residual")
    _, _, dl = _mk(torch.bfloat16, 64)
    assert dl.transport.k == 64 and not bool(dl.topk_residual.any())
    assert dl.transport.shared_state()[0]["comm_topk"] == {"k": 64, "chunk": 4096, "value_dtype": "bf16"}


def test_rules_through_the_cli():
    from nanodiloco_amd.trainer import Trainer
    assert parse_args([]).comm_topk == 0
    assert parse_args(["--comm-topk", "64", "--comm-dtype", "bf16"]).comm_topk == 64
    base = ["--total-steps", "8", "--inner-steps", "4", "--device", "cpu", "--wandb", "off", "--comm-topk", "64"]
    for extra, word in ((["--comm-dtype", "int8"], "--comm-dtype int8"), (["--comm-dtype", "int4"], "--comm-dtype int4"),
                        (["--comm-error-feedback"], "--comm-error-feedback"), (["--overlap-outer"], "--overlap-outer"),
                        (["--streaming-fragments", "1"], "--streaming-fragments"), (["--comm-topk", "5000"], "4096")):
        with pytest.raises(ValueError, match="--comm-topk") as err:
            Trainer(parse_args(base + extra))
        assert word in str(err.value)


# ------------------------------------------------------------------------------------- 4. torchrun
BASE = ["--llama-config-file", "configs/llama_tiny.json", "--batch-size", "8", "--per-device-batch-size", "4",
        "--seq-length", "64", "--warmup-steps", "2", "--wandb", "off", "--device", "cpu", "--debug-checks",
        "--total-steps", "8", "--inner-steps", "4", "--data", "synthetic", "--eval-every", "4", "--eval-batches", "2"]
TOPK = ["--comm-topk", "64", "--comm-dtype", "bf16"]


def _torchrun(nproc, args, timeout=600):
    env = child_env(OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m", "nanodiloco_amd"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _log(path):
    return [json.loads(line) for line in open(path)]


def _tensors(path):
    from safetensors.torch import load_file
    return load_file(str(path))


@pytest.mark.slow
def test_cli_run_stop_resume_bitwise_and_resume_rules(tmp_path):
    """torchrun, 2 gloo workers on configs/llama_tiny.json with --comm-topk 64 --comm-dtype bf16 --eval-every:
    the interrupted and resumed run ends bit for bit where the uninterrupted one does, --debug-checks stays silent
    (the runs succeed), the logged bytes are the slot's, and a top-k checkpoint resumes without the flag (residual
    ignored, logged) and with another k (residual kept)."""
    a, b = tmp_path / "a", tmp_path / "b"
    la, lb = tmp_path / "a.jsonl", tmp_path / "b.jsonl"
    r = _torchrun(2, BASE + TOPK + ["--checkpoint-dir", str(a), "--log-file", str(la)])
    assert "Training completed!" in r.stdout
    _torchrun(2, BASE + TOPK + ["--stop-at-step", "4", "--checkpoint-dir", str(b), "--checkpoint-every", "1"])
    mid = tmp_path / "mid"
    subprocess.run(["cp", "-r", str(b), str(mid)], check=True)
    _torchrun(2, BASE + TOPK + ["--resume", str(b), "--checkpoint-dir", str(b), "--log-file", str(lb)])
    ra, rb = _log(la), _log(lb)
    train_a, train_b = [x for x in ra if "loss" in x], [x for x in rb if "loss" in x]
    assert [x["step"] for x in train_a] == list(range(1, 9)) and [x["step"] for x in train_b] == [5, 6, 7, 8]
    assert train_a[-1]["loss"] == train_b[-1]["loss"]
    eval_a, eval_b = [x for x in ra if "eval_loss" in x], [x for x in rb if "eval_loss" in x]
    assert [x["step"] for x in eval_a] == [4, 8] and eval_a[-1]["eval_loss"] == eval_b[-1]["eval_loss"]
    print(f"top-k 64 bf16, 2 workers: final eval_loss {eval_a[-1]['eval_loss']}")
    for f in ("model.safetensors", "diloco_state.safetensors", "rank0.safetensors", "rank1.safetensors"):
        ta, tb = _tensors(a / f), _tensors(b / f)
        assert ta.keys() == tb.keys()
        for key in ta:
            if not key.startswith("data."):  # the residual, the optimizer state, the weights
                assert torch.equal(ta[key], tb[key]), (f, key)
    n = json.load(open(a / "trainer_state.json"))["flat_numel"]
    assert train_a[3]["bytes_outer"] == ops.topk_slot_bytes(n, 64, torch.bfloat16) > 0
    assert json.load(open(a / "trainer_state.json"))["comm_topk"] == {"k": 64, "chunk": 4096, "value_dtype": "bf16"}
    saved = [_tensors(mid / f"rank{rk}.safetensors")["topk.residual"] for rk in (0, 1)]
    assert all(t.numel() == n and bool((t != 0).any()) for t in saved) and not torch.equal(saved[0], saved[1])
    # without the flag: the dense run of that state, the residual is dropped with a line in the log
    r = _torchrun(2, BASE + ["--resume", str(mid)])
    assert "checkpoint holds a top-k residual" in r.stdout and "ignored" in r.stdout
    # another k (and value dtype): the residual is an fp32 amount still owed and stays
    c = tmp_path / "c"
    r = _torchrun(2, BASE + ["--comm-topk", "7", "--comm-dtype", "fp32", "--resume", str(mid), "--checkpoint-dir", str(c)])
    assert "starting from zero" not in r.stdout and "top-k residual" not in r.stdout
    assert json.load(open(c / "trainer_state.json"))["comm_topk"] == {"k": 7, "chunk": 4096, "value_dtype": "fp32"}


def _resume_rules(rank, world, tmp):
    """load_state through save_checkpoint / load_checkpoint: another k keeps the residual, a changed length or a
    checkpoint without one starts from zero."""
    from nanodiloco_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    env, m, dl = _mk(torch.bfloat16, 64)
    m.store.master.add_(_drift(m.store.numel, 0, env.worker))
    dl.outer_step()
    res = dl.topk_residual.clone()
    assert bool((res != 0).any())
    save_checkpoint(os.path.join(tmp, "tk"), m, dl, env, 4)
    _, m2, dl2 = _mk(torch.float32, 7, env=env, seed=8)
    load_checkpoint(os.path.join(tmp, "tk"), m2, dl2, env)
    assert torch.equal(dl2.topk_residual, res)
    assert dl2.transport.load_state({"topk.residual": res[:-64]}, {}, {"comm_topk": {}})[-1].endswith("starting from zero")
    assert not bool(dl2.topk_residual.any())
    dl2.topk_residual.fill_(1.0)
    assert "starting from zero" in dl2.transport.load_state({}, {}, {"comm_topk": {}})[-1]
    assert not bool(dl2.topk_residual.any())
    # a dense checkpoint into a top-k run: zero residual, nothing to say
    _, m3, dl3 = _mk(torch.float32, 0, env=env)
    save_checkpoint(os.path.join(tmp, "dense"), m3, dl3, env, 4)
    dl2.topk_residual.fill_(1.0)
    load_checkpoint(os.path.join(tmp, "dense"), m2, dl2, env)
    assert not bool(dl2.topk_residual.any())
    # a top-k checkpoint into dense and quantised runs: ignored, and rank 0 says so
    for comm in (torch.float32, "int8"):
        _, m4, dl4 = _mk(comm, 0, env=env)
        per = {"topk.residual": res}
        lines = dl4.transport.load_state(per, {}, {"comm_topk": {}})
        assert (len(lines) == 1 and "ignored" in lines[0]) if rank == 0 else lines == []
    return True


def test_checkpoint_residual_rules(tmp_path):
    assert all(run_ranks(_resume_rules, 2, str(tmp_path)))
