"""z-loss (``--z-loss``, ``ops.lm_head_ce(..., z_loss=)``) without a GPU: the PyTorch twin branch of the op and the
float64 oracle of ``tests/_zloss.py`` against float64 autograd of ``CE + z`` on explicit logits, the model's loss
parts, and the CLI on two gloo workers (log records, refusals, resume)."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.main import parse_args
from nanodiloco_amd.models import LlamaForCausalLM

from . import _zloss as zl
from ._mp import child_env, free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = 1e-2
N, D, V, SCALE = 96, 32, 101, 0.25


def _inputs():
    torch.manual_seed(0)
    y = torch.randn(N, D)
    w = 0.5 * torch.randn(V, D)
    tgt = torch.randint(0, V, (N,))
    tgt[::7] = zl.IGN
    return y, w, tgt


def _op(y0, w, tgt, **kw):
    y = y0.clone().requires_grad_(True)
    gw = torch.zeros(V, D)
    parts = ops.lm_head_ce_parts(y, w, gw, tgt, loss_scale=SCALE, chunk_rows=64, **kw)
    parts.loss.backward()
    return parts, y.grad, gw


def test_oracle_matches_float64_autograd():
    """The oracle the GPU tests judge the kernels by is the gradient of the objective: 1e-12 from float64 autograd."""
    y, w, tgt = _inputs()
    for got, want in zip(zl.lm_head_ce_z(y, w, tgt, SCALE, Z), zl.autograd_ce_z(y, w, tgt, SCALE, Z)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # a negative lse (g < 1) and a missing factor are both visible to it
    lse, _, _, dl = zl.ce_z_rows(torch.randn(4, V) - 20.0, torch.tensor([0, 5, zl.IGN, 100]), 1.0, Z)
    assert bool((lse < 0).all()) and not bool(dl[2].any())
    _, _, _, dl0 = zl.ce_z_rows(torch.randn(4, V) - 20.0, torch.tensor([0, 5, zl.IGN, 100]), 1.0, 0.0)
    assert float((dl - dl0).abs().max()) > 1e-3


def test_lm_head_ce_twin_matches_float64_autograd():
    y, w, tgt = _inputs()
    parts, dy, gw = _op(y, w, tgt, z_loss=Z)
    ce64, z64, dy64, gw64 = zl.autograd_ce_z(y, w, tgt, SCALE, Z)
    close = dict(rtol=1e-5, atol=1e-6)
    assert float(z64) > 0.05  # the term is there to be seen
    torch.testing.assert_close(parts.ce_loss.double(), ce64, **close)
    torch.testing.assert_close(parts.z_loss.double(), z64, **close)
    torch.testing.assert_close(parts.loss.detach().double(), ce64 + z64, **close)
    torch.testing.assert_close(dy.double(), dy64, **close)
    torch.testing.assert_close(gw.double(), gw64, **close)
    assert not parts.ce_loss.requires_grad and not parts.z_loss.requires_grad
    # lm_head_ce returns the objective
    y2 = y.clone().requires_grad_(True)
    assert torch.equal(ops.lm_head_ce(y2, w, torch.zeros(V, D), tgt, loss_scale=SCALE, chunk_rows=64, z_loss=Z),
                       parts.loss)


def test_z_loss_zero_is_bitwise_the_call_without_it():
    y, w, tgt = _inputs()
    a, dya, gwa = _op(y, w, tgt)
    b, dyb, gwb = _op(y, w, tgt, z_loss=0.0)
    assert torch.equal(a.loss, b.loss) and torch.equal(dya, dyb) and torch.equal(gwa, gwb)
    assert torch.equal(a.ce_loss, a.loss.detach()) and a.z_loss is None and b.z_loss is None
    # and the gradient of a real z run differs from it
    _, dyz, _ = _op(y, w, tgt, z_loss=Z)
    assert not torch.equal(dyz, dya)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_bad_coefficients_are_refused(bad):
    y, w, tgt = _inputs()
    with pytest.raises(ValueError, match="z_loss"):
        ops.lm_head_ce(y, w, None, tgt, z_loss=bad)


def test_model_output_parts():
    cfg = LlamaConfig.from_dict(dict(hidden_size=32, intermediate_size=64, num_attention_heads=2, num_hidden_layers=1,
                                     vocab_size=50, rms_norm_eps=1e-5))
    m = LlamaForCausalLM(cfg).init_weights(3)
    ids = torch.randint(0, 50, (2, 16), generator=torch.Generator().manual_seed(1))
    assert m.z_loss == 0.0
    out0 = m(ids, labels=ids)
    out0.loss.backward()
    g0 = m.store.grad.clone()
    assert out0.z_loss is None and torch.equal(out0.ce_loss, out0.loss.detach()) and not out0.ce_loss.requires_grad
    m.store.zero_grad()
    m.z_loss = Z
    out = m(ids, labels=ids)
    out.loss.backward()
    assert torch.equal(out.ce_loss, out0.ce_loss)  # the same fp32 rows, summed the same way
    assert float(out.z_loss) > 0 and torch.equal(out.loss.detach(), out.ce_loss + out.z_loss)
    assert not torch.equal(m.store.grad, g0)
    # evaluation ignores it
    m.eval()
    s = m.loss_stats(ids, ids)
    assert abs(float(s[0] / s[1]) - float(out0.ce_loss)) < 1e-5


# ------------------------------------------------------------------------------------------ CLI
BASE = ["--llama-config-file", "configs/llama_tiny.json", "--batch-size", "8", "--per-device-batch-size", "4",
        "--seq-length", "64", "--warmup-steps", "2", "--wandb", "off", "--device", "cpu", "--debug-checks",
        "--data", "synthetic", "--inner-steps", "4", "--total-steps", "8"]


def _torchrun(nproc, args, timeout=600):
    env = child_env(OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m", "nanodiloco_amd"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _log(path):
    return [json.loads(l) for l in open(path)]


def _tensors(path):
    from safetensors.torch import load_file
    return load_file(str(path))


def test_cli_flag_parses_and_refuses_bad_values():
    from nanodiloco_amd.trainer import Trainer
    assert parse_args([]).z_loss == 0.0
    assert parse_args(["--z-loss", "1e-4"]).z_loss == 1e-4
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(ValueError, match="--z-loss"):
            Trainer(parse_args(BASE + ["--z-loss", bad]))


@pytest.mark.slow
def test_cli_two_workers_records_and_resume(tmp_path):
    """Two gloo workers, 8 steps, H = 4, --z-loss 1e-3: every record has a finite z_loss > 0 and `loss` stays the
    cross-entropy (step 1, from the initial weights on the same batch, against the run without the flag); the run
    without the flag has no new key; stopping at step 4 and resuming gives the uninterrupted run bit for bit."""
    a, b = tmp_path / "a", tmp_path / "b"
    la, lb, l0 = tmp_path / "a.jsonl", tmp_path / "b.jsonl", tmp_path / "0.jsonl"
    zrun = BASE + ["--z-loss", "1e-3"]
    _torchrun(2, zrun + ["--checkpoint-dir", str(a), "--log-file", str(la)])
    _torchrun(2, BASE + ["--log-file", str(l0)])
    ra, r0 = _log(la), _log(l0)
    assert [x["step"] for x in ra] == [x["step"] for x in r0] == list(range(1, 9))
    for x in ra:
        assert math.isfinite(x["z_loss"]) and x["z_loss"] > 0
        assert x["Perplexity"] == math.exp(min(x["loss"], 80.0))  # of the cross-entropy, as ever
    for x, z in zip(r0, ra):
        assert "z_loss" not in x and set(x) == set(z) - {"z_loss"}
    assert abs(ra[0]["loss"] - r0[0]["loss"]) <= 1e-6 * abs(r0[0]["loss"])
    # V = 32000 at initialisation: lse ~ ln V, so the weighted term is about 1e-3 * (ln 32000)^2 = 0.1076
    assert abs(ra[0]["z_loss"] - 1e-3 * math.log(32000) ** 2) < 5e-3
    assert any(x["loss"] != y["loss"] for x, y in zip(ra[2:], r0[2:]))  # the term does steer the run
    with open(a / "trainer_state.json") as f:
        assert "z_loss" not in f.read()  # a hyperparameter: nothing of it in a checkpoint
    _torchrun(2, zrun + ["--stop-at-step", "4", "--checkpoint-dir", str(b), "--checkpoint-every", "1"])
    _torchrun(2, zrun + ["--resume", str(b), "--checkpoint-dir", str(b), "--log-file", str(lb)])
    rb = _log(lb)
    assert [x["step"] for x in rb] == [5, 6, 7, 8]
    for x, y in zip(ra[4:], rb):
        assert x["loss"] == y["loss"] and x["z_loss"] == y["z_loss"]
    for f in ("model.safetensors", "diloco_state.safetensors"):
        ta, tb = _tensors(a / f), _tensors(b / f)
        assert ta.keys() == tb.keys()
        for k in ta:
            assert torch.equal(ta[k], tb[k]), (f, k)
