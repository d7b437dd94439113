"""int8 / int4 block-quantised transport of the DiLoCo outer step over gloo, and through the CLI."""
import json
import os
import subprocess
import sys

import pytest
import torch

from nanodiloco_amd.config import LlamaConfig
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


def _mk(comm, inner_dp=1, seed=7, env=None, **kw):
    env = env or init_distributed("gloo", inner_dp=inner_dp)
    m = LlamaForCausalLM(LlamaConfig.from_dict(TINY)).init_weights(seed)
    dl = Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store, lr=LR, momentum=MU), 2, 8, 4, env=env,
                comm_dtype=comm, **kw)
    return env, m, dl


def _golden(rank, world, comm):
    """The golden values of test_diloco_cpu.py: constant blocks quantise to +-QMAX, so the error is a few ulp."""
    env, m, dl = _mk(comm, seed=100 + rank)
    st = m.store
    theta0 = st.master.clone()
    st.master.sub_(rank + 1.0)
    dl.outer_step()
    step1 = st.master - theta0
    assert torch.allclose(step1[: st.num_params], torch.full_like(step1[: st.num_params], -1.995), atol=1e-5), step1[:4]
    assert torch.equal(dl.sync, st.master)
    th1 = st.master.clone()
    dl.outer_step()
    step2 = st.master - th1
    assert torch.allclose(step2[: st.num_params], torch.full_like(step2[: st.num_params], -0.8505), atol=1e-5), step2[:4]
    dl.check_replicas()
    return True


@pytest.mark.parametrize("comm", COMM)
def test_golden_values_two_workers(comm):
    assert all(run_ranks(_golden, 2, comm))


# shared with tests/test_transports_multiworker_gpu.py
_random_drift, _several_buckets = oc.q_random_drift, oc.q_several_buckets


@pytest.mark.parametrize("comm", COMM)
def test_random_drift_four_workers_matches_oracle_bitwise(comm):
    assert all(run_ranks(_random_drift, 4, comm, 1))


@pytest.mark.parametrize("comm", COMM)
def test_two_level_quantised(comm):
    assert all(run_ranks(_random_drift, 4, comm, 2))


def test_three_workers_many_buckets_offloaded_snapshot():
    assert all(run_ranks(_several_buckets, 3))


def test_single_process_and_int8_dtype_alias():
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    for comm in ("int8", torch.int8, "int4"):
        env, m, dl = _mk(comm, seed=1)
        assert dl.qbits == (4 if comm == "int4" else 8)
        st = m.store
        base = st.master.clone()
        st.master.sub_(2.0)
        dl.outer_step()  # W=1: -0.7 * (2 + 1.8) = -2.66
        assert torch.allclose(st.master[: st.num_params], (base - 2.66)[: st.num_params], atol=1e-5)
        assert dl.bytes_per_outer_step == 0 and dl.buckets_per_outer_step == 0  # no collectives without a group


def test_quantised_transport_rejects_overlap_and_plain_modules():
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    for comm in ("int8", "int4", torch.int8):
        with pytest.raises(ValueError, match="overlap"):
            _mk(comm, overlap=True)
        net = torch.nn.Linear(4, 4)
        with pytest.raises(ValueError, match="quantised"):
            Diloco(net, torch.optim.AdamW(net.parameters(), lr=1e-3), torch.optim.SGD(net.parameters(), lr=0.7), 0, 10,
                   comm_dtype=comm)
    with pytest.raises(ValueError):
        _mk("int2")


# ---------------------------------------------------------------------------------------------- CLI
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
def test_cli_quantised_bytes_and_stateless_resume(tmp_path):
    """torchrun, 2 ranks: int8 and int4 runs finish with a finite loss and log about a quarter / an eighth
    of the fp32 run's bytes; a checkpoint written with int8 resumes with fp32 and the other way round."""
    run = BASE + ["--total-steps", "8", "--inner-steps", "4", "--data", "synthetic"]
    rows = {}
    for comm in ("fp32", "int8", "int4"):
        log = tmp_path / f"{comm}.jsonl"
        r = _torchrun(2, run + ["--comm-dtype", comm, "--log-file", str(log), "--checkpoint-dir", str(tmp_path / comm)])
        assert "Training completed!" in r.stdout
        rows[comm] = _log(log)
        assert [x["step"] for x in rows[comm]] == list(range(1, 9))
        assert all(x["loss"] == x["loss"] and abs(x["loss"]) < 1e4 for x in rows[comm])
    b32, b8, b4 = (rows[c][3]["bytes_outer"] for c in ("fp32", "int8", "int4"))
    # codes are 1/4 (1/8) of fp32; the scales add 4 bytes per 256 elements and the chunks are padded to blocks
    assert 0.25 <= b8 / b32 < 0.26 and 0.125 <= b4 / b32 < 0.135, (b32, b8, b4)
    for src, dst in (("int8", "fp32"), ("fp32", "int8")):
        log = tmp_path / f"resume_{dst}.jsonl"
        _torchrun(2, BASE + ["--total-steps", "12", "--inner-steps", "4", "--data", "synthetic", "--comm-dtype", dst,
                             "--resume", str(tmp_path / src), "--log-file", str(log)])
        got = _log(log)
        assert [x["step"] for x in got] == [9, 10, 11, 12] and all(x["loss"] == x["loss"] for x in got)
