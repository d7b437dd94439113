"""Error feedback of the int8 / int4 outer transport (``Diloco(error_feedback=True)``, ``--comm-error-feedback``)
over gloo, through checkpoints and through the CLI."""
import json
import os
import subprocess
import sys

import pytest
import torch

from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.main import parse_args
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
from nanodiloco_amd.parallel.diloco import Diloco
from nanodiloco_amd.parallel.dist import init_distributed

from . import _outer_chains as oc
from ._mp import child_env, free_port, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(hidden_size=32, intermediate_size=64, num_attention_heads=2, num_hidden_layers=1, vocab_size=50,
            rms_norm_eps=1e-5)
LR, MU = 0.7, 0.9
COMM = ["int8", "int4"]


def _mk(comm, inner_dp=1, seed=7, env=None, ef=True, **kw):
    env = env or init_distributed("gloo", inner_dp=inner_dp)
    m = LlamaForCausalLM(LlamaConfig.from_dict(TINY)).init_weights(seed)
    dl = Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store, lr=LR, momentum=MU), 2, 8, 4, env=env,
                comm_dtype=comm, error_feedback=ef, **kw)
    return env, m, dl


# ------------------------------------------------------------------------------------- 6. bitwise chain
# the chains are shared with tests/test_transports_multiworker_gpu.py
_chain, _several_buckets, _checkpoints = oc.qef_chain, oc.qef_several_buckets, oc.qef_checkpoints


@pytest.mark.parametrize("comm", COMM)
@pytest.mark.parametrize("world", [2, 4])
def test_three_steps_match_oracle_chain_bitwise(world, comm):
    assert all(run_ranks(_chain, world, comm, 1))


@pytest.mark.parametrize("comm", COMM)
def test_two_level_error_feedback(comm):
    assert all(run_ranks(_chain, 4, comm, 2))


# ------------------------------------------------------------------------------------- 7. many buckets
def test_three_workers_many_buckets_offloaded_snapshot():
    assert all(run_ranks(_several_buckets, 3))


# ------------------------------------------------------------------------------------- 8. checkpoint
def test_checkpoint_roundtrip_and_resume_rules(tmp_path):
    assert all(run_ranks(_checkpoints, 2, str(tmp_path)))


# ------------------------------------------------------------------------------------- 9. refusals, CLI
def test_error_feedback_needs_the_quantised_transport():
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    for comm in (torch.float32, torch.bfloat16):
        with pytest.raises(ValueError, match="error_feedback"):
            _mk(comm)
    net = torch.nn.Linear(4, 4)
    for comm in ("int8", None):
        with pytest.raises(ValueError):
            Diloco(net, torch.optim.AdamW(net.parameters(), lr=1e-3), torch.optim.SGD(net.parameters(), lr=0.7), 0, 10,
                   comm_dtype=comm, error_feedback=True)
    # off by default, and then there are no buffers
    _, _, dl = _mk("int4", ef=False)
    assert dl.error_feedback is False and dl.error_feedback_state() is None
    _, _, dl = _mk("int4")
    assert dl.error_feedback_state()["bits"] == 4 and not bool(dl.qef_send.any())


def test_cli_flag_parses_and_is_rejected_without_quantised_transport():
    from nanodiloco_amd.trainer import Trainer
    assert parse_args([]).comm_error_feedback is False
    assert parse_args(["--comm-dtype", "int4", "--comm-error-feedback"]).comm_error_feedback is True
    assert parse_args(["--comm-error-feedback", "false"]).comm_error_feedback is False
    for comm in ("fp32", "bf16"):
        with pytest.raises(ValueError, match="--comm-error-feedback"):
            Trainer(parse_args(["--comm-dtype", comm, "--comm-error-feedback", "--total-steps", "8", "--inner-steps", "4",
                                "--device", "cpu", "--wandb", "off"]))


# ------------------------------------------------------------------------------------- 10. torchrun
BASE = ["--llama-config-file", "configs/llama_tiny.json", "--batch-size", "8", "--per-device-batch-size", "4",
        "--seq-length", "64", "--warmup-steps", "2", "--wandb", "off", "--device", "cpu", "--debug-checks"]


def _torchrun(nproc, args, timeout=600):
    env = child_env(OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m", "nanodiloco_amd"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _log(path):
    return [json.loads(l) for l in open(path)]


@pytest.mark.slow
def test_cli_error_feedback_run_resume_and_elastic_resume(tmp_path):
    """torchrun, 2 ranks: an int4 run with --comm-error-feedback finishes with a finite loss and logs the bytes of
    the stateless int4 run; its checkpoint resumes to step 12, and onto 3 ranks with --elastic-resume."""
    run = BASE + ["--total-steps", "8", "--inner-steps", "4", "--data", "synthetic", "--comm-dtype", "int4"]
    rows = {}
    for name, extra in (("plain", []), ("ef", ["--comm-error-feedback"])):
        log = tmp_path / f"{name}.jsonl"
        r = _torchrun(2, run + extra + ["--log-file", str(log), "--checkpoint-dir", str(tmp_path / name)])
        assert "Training completed!" in r.stdout
        rows[name] = _log(log)
        assert [x["step"] for x in rows[name]] == list(range(1, 9))
        assert all(x["loss"] == x["loss"] and abs(x["loss"]) < 1e4 for x in rows[name])
    assert rows["ef"][3]["bytes_outer"] == rows["plain"][3]["bytes_outer"] > 0
    with open(tmp_path / "ef" / "trainer_state.json") as f:
        meta = json.load(f)["comm_error_feedback"]
    assert meta["bits"] == 4 and meta["num_workers"] == 2 and meta["plan"]
    resume = BASE + ["--total-steps", "12", "--inner-steps", "4", "--data", "synthetic", "--comm-dtype", "int4",
                     "--comm-error-feedback", "--resume", str(tmp_path / "ef")]
    for nproc, extra in ((2, []), (3, ["--elastic-resume"])):
        log = tmp_path / f"resume{nproc}.jsonl"
        r = _torchrun(nproc, resume + extra + ["--log-file", str(log)])
        got = _log(log)
        assert [x["step"] for x in got] == [9, 10, 11, 12] and all(x["loss"] == x["loss"] for x in got)
        if nproc == 3:
            assert "qef.reduce was saved for another bucket plan or worker count" in r.stdout
