"""Logit soft-capping without a GPU: the float64 oracle against float64 autograd, the PyTorch path of
``ops.lm_head_ce`` / ``lm_head_loss`` against the oracle, ``softcap=0.0`` bitwise the cap-free call, the config key,
the CLI flag, the logits the model hands out, and one two-worker gloo run through the CLI."""
import dataclasses
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

from . import _softcap as sc
from ._mp import child_env, free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, Z = 5.0, 1e-2
N, D, V, SCALE = 96, 32, 101, 0.25


def _inputs():
    torch.manual_seed(0)
    y = torch.randn(N, D)
    w = 0.9 * torch.randn(V, D)  # logits of std 5: from the linear part of the cap well into its saturation
    tgt = torch.randint(0, V, (N,))
    tgt[::7] = sc.IGN
    return y, w, tgt


def _op(y0, w, tgt, **kw):
    y = y0.clone().requires_grad_(True)
    gw = torch.zeros(V, D)
    parts = ops.lm_head_ce_parts(y, w, gw, tgt, loss_scale=SCALE, chunk_rows=64, **kw)
    parts.loss.backward()
    return parts, y.grad, gw


@pytest.mark.parametrize("z", [0.0, Z], ids=["ce", "ce+z"])
def test_oracle_matches_float64_autograd(z):
    """The oracle the GPU tests judge the kernels by is the gradient of the objective: 1e-12 from float64 autograd,
    ignored rows and an all-ignored batch included."""
    y, w, tgt = _inputs()
    d = 1 - torch.tanh((y.double() @ w.double().t()) / CAP) ** 2
    assert float(d.min()) < 0.1 and float(d.max()) > 0.95  # the factor is there to be seen
    for t in (tgt, torch.full_like(tgt, sc.IGN)):
        for got, want in zip(sc.lm_head_ce_cap(y, w, t, SCALE, z, CAP), sc.autograd_ce_cap(y, w, t, SCALE, z, CAP)):
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    lse, ce, zz, dl = sc.ce_cap_rows(y @ w.t(), tgt, 1.0, z, CAP)
    assert not bool(dl[tgt == sc.IGN].any()) and not bool(ce[tgt == sc.IGN].any()) and not bool(zz[tgt == sc.IGN].any())
    assert float(lse.max()) <= CAP + math.log(V)  # |y| <= C


@pytest.mark.parametrize("z", [0.0, Z], ids=["ce", "ce+z"])
def test_lm_head_ce_cpu_path_matches_the_oracle(z):
    y, w, tgt = _inputs()
    parts, dy, gw = _op(y, w, tgt, z_loss=z, softcap=CAP)
    ce64, z64, dy64, gw64 = sc.lm_head_ce_cap(y, w, tgt, SCALE, z, CAP)
    close = dict(rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(parts.ce_loss.double(), ce64, **close)
    if z:
        torch.testing.assert_close(parts.z_loss.double(), z64, **close)
    else:
        assert parts.z_loss is None and torch.equal(parts.ce_loss, parts.loss.detach())
    torch.testing.assert_close(parts.loss.detach().double(), ce64 + z64, **close)
    torch.testing.assert_close(dy.double(), dy64, **close)
    torch.testing.assert_close(gw.double(), gw64, **close)
    y2 = y.clone().requires_grad_(True)
    assert torch.equal(ops.lm_head_ce(y2, w, torch.zeros(V, D), tgt, loss_scale=SCALE, chunk_rows=64, z_loss=z,
                                      softcap=CAP), parts.loss)
    # the cap is no rounding matter here
    p0, dy0, _ = _op(y, w, tgt, z_loss=z)
    assert abs(float(p0.ce_loss) - float(parts.ce_loss)) > 0.1 and not torch.equal(dy0, dy)


def test_lm_head_loss_cpu_path_matches_the_oracle():
    y, w, tgt = _inputs()
    row_loss, row_hit = ops.lm_head_loss(y, w, tgt, chunk_rows=64, softcap=CAP)
    _, ce64, _, _ = sc.ce_cap_rows(y @ w.t(), tgt, 1.0, 0.0, CAP)
    torch.testing.assert_close(row_loss.double(), ce64, rtol=1e-5, atol=1e-6)
    loss0, hit0 = ops.lm_head_loss(y, w, tgt, chunk_rows=64)
    assert torch.equal(row_hit, hit0) and not torch.equal(row_loss, loss0)  # top-1 stays on the stored logits


def test_softcap_zero_is_bitwise_the_call_without_it():
    y, w, tgt = _inputs()
    a, dya, gwa = _op(y, w, tgt)
    for off in (0.0, None):
        b, dyb, gwb = _op(y, w, tgt, softcap=off)
        assert torch.equal(a.loss, b.loss) and torch.equal(dya, dyb) and torch.equal(gwa, gwb) and b.z_loss is None
    a, dya, gwa = _op(y, w, tgt, z_loss=Z)
    b, dyb, gwb = _op(y, w, tgt, z_loss=Z, softcap=0.0)
    assert torch.equal(a.loss, b.loss) and torch.equal(a.z_loss, b.z_loss) and torch.equal(dya, dyb)
    assert torch.equal(gwa, gwb)
    la, ha = ops.lm_head_loss(y, w, tgt, chunk_rows=64)
    lb, hb = ops.lm_head_loss(y, w, tgt, chunk_rows=64, softcap=0.0)
    assert torch.equal(la, lb) and torch.equal(ha, hb)
    x = torch.randn(7, 5)
    assert ops.logit_softcap(x, 0.0) is x and torch.equal(ops.reference.softcap(x, 0.0), x)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), "30", True])
def test_bad_caps_are_refused(bad):
    y, w, tgt = _inputs()
    with pytest.raises(ValueError, match="softcap"):
        ops.lm_head_ce(y, w, None, tgt, softcap=bad)
    with pytest.raises(ValueError, match="softcap"):
        ops.lm_head_loss(y, w, tgt, softcap=bad)
    with pytest.raises(ValueError, match="softcap"):
        ops.logit_softcap(torch.zeros(4), bad)


def test_reference_softcap():
    x = torch.tensor([0.0, 1e-4, -1e-4, 8.0, -8.0, 300.0, -300.0, float("nan")])
    y = ops.reference.softcap(x, 8.0)
    want = sc.softcap64(x, 8.0)
    assert torch.allclose(y[:-1].double(), want[:-1], rtol=1e-6, atol=0) and bool(torch.isnan(y[-1]))
    assert y[5].item() == 8.0 and y[6].item() == -8.0
    z = x.clone()
    assert ops.logit_softcap(z, 8.0) is z and torch.equal(z[:-1], y[:-1])


# ------------------------------------------------------------------------------------------ config
TINY = dict(hidden_size=32, intermediate_size=64, num_attention_heads=2, num_hidden_layers=2, vocab_size=50,
            rms_norm_eps=1e-5, max_position_embeddings=64)


def test_config_key_round_trips_and_is_absent_when_off():
    off = LlamaConfig.from_dict(TINY)
    assert off.final_logit_softcapping is None
    assert "final_logit_softcapping" not in off.to_dict() and "final_logit_softcapping" not in off.to_hf_json()
    for zero in (0, 0.0, None):
        c = LlamaConfig.from_dict({**TINY, "final_logit_softcapping": zero})
        assert c.final_logit_softcapping is None and c.to_dict() == off.to_dict() and c.to_hf_json() == off.to_hf_json()
    on = LlamaConfig.from_dict({**TINY, "final_logit_softcapping": 30.0})
    assert on.final_logit_softcapping == 30.0 and "final_logit_softcapping" not in on.extra
    d = on.to_hf_json()
    assert d["final_logit_softcapping"] == 30.0 and d["architectures"] == ["LlamaForCausalLM"]
    back = LlamaConfig.from_dict(json.loads(json.dumps(d)))
    assert back.final_logit_softcapping == 30.0
    assert {k: v for k, v in d.items() if k != "final_logit_softcapping"} == off.to_hf_json()
    assert LlamaConfig.from_dict({**TINY, "final_logit_softcapping": 30}).final_logit_softcapping == 30
    assert LlamaForCausalLM(on).softcap == 30.0 and LlamaForCausalLM(off).softcap == 0.0


@pytest.mark.parametrize("bad", [-1, float("inf"), float("nan"), "30", True])
def test_config_refuses_bad_values(bad):
    with pytest.raises(ValueError, match="final_logit_softcapping"):
        LlamaConfig.from_dict({**TINY, "final_logit_softcapping": bad})


# ------------------------------------------------------------------------------------------ model
def _pair(cap):
    off = LlamaConfig.from_dict(TINY)
    on = dataclasses.replace(off, final_logit_softcapping=cap)
    m0, m1 = LlamaForCausalLM(off).init_weights(3), LlamaForCausalLM(on).init_weights(3)
    for m in (m0, m1):  # weights large enough for the logits to reach the cap
        m.store.master.mul_(6.0)
        m.store.sync_shadow()
    return m0, m1


def test_model_logits_are_the_cap_of_the_uncapped_models():
    """forward, prefill and decode_step of the capped model give reference.softcap of the cap-free model's logits
    (the same weights); the loss and loss_stats are those of the capped logits."""
    cap = 2.0
    m0, m1 = _pair(cap)
    ids = torch.randint(0, 50, (2, 16), generator=torch.Generator().manual_seed(1))
    l0, l1 = m0(ids).logits, m1(ids).logits
    assert float(l0.abs().max()) > 2 * cap and float(l1.abs().max()) <= cap
    assert torch.equal(l1, ops.reference.softcap(l0, cap))
    out = m1(ids, labels=ids, return_logits=True)
    assert torch.equal(out.logits, l1)
    want = ops.reference.cross_entropy_loss(l1, ops.reference.shift_labels(ids))
    assert abs(float(out.loss.detach()) - float(want)) <= 1e-5 * float(want)
    s = m1.loss_stats(ids, ids)
    assert abs(float(s[0] / s[1]) - float(want)) <= 1e-5 * float(want)
    assert torch.equal(s[2], m0.loss_stats(ids, ids)[2])  # top-1 hits: unaffected
    c0, c1 = m0.new_cache(2, 24), m1.new_cache(2, 24)
    p0, p1 = m0.prefill(ids, None, c0), m1.prefill(ids, None, c1)
    assert torch.equal(p1, ops.reference.softcap(p0, cap)) and torch.equal(p1, l1[:, -1])
    tok = p0.argmax(-1)
    d0, d1 = m0.decode_step(tok, c0), m1.decode_step(tok, c1)
    assert torch.equal(d1, ops.reference.softcap(d0, cap)) and float(d1.abs().max()) <= cap
    # generation without the cache goes through forward(): the same greedy tokens either way
    g_cache = m1.generate(ids, max_new_tokens=4)
    g_plain = m1.generate(ids, max_new_tokens=4, use_cache=False)
    assert torch.equal(g_cache, g_plain)


# ------------------------------------------------------------------------------------------ CLI
BASE = ["--llama-config-file", "configs/llama_tiny.json", "--batch-size", "8", "--per-device-batch-size", "4",
        "--seq-length", "64", "--warmup-steps", "2", "--wandb", "off", "--device", "cpu", "--debug-checks",
        "--data", "synthetic", "--inner-steps", "2", "--total-steps", "4", "--eval-every", "4", "--eval-batches", "1"]


def _torchrun(nproc, args, ok=True, timeout=600):
    env = child_env(OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m", "nanodiloco_amd"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _log(path):
    return [json.loads(l) for l in open(path)]


def _tensors(path):
    from safetensors.torch import load_file
    return load_file(str(path))


def test_cli_flag_parses_and_refuses_bad_values():
    from nanodiloco_amd.trainer import Trainer
    assert parse_args([]).logit_softcap == 0.0
    assert parse_args(["--logit-softcap", "30"]).logit_softcap == 30.0
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            parse_args(["--logit-softcap", bad])
        with pytest.raises(ValueError, match="--logit-softcap"):
            Trainer(dataclasses.replace(parse_args(BASE), logit_softcap=float(bad)))


def _held_out_loss(ckpt, cfg, world):
    """What the run's final evaluation computed, from the checkpoint: every rank's held-out batch through
    ``loss_stats`` of the model that ``config.json`` describes, summed before the division."""
    from nanodiloco_amd.data import build_eval_data
    from nanodiloco_amd.utils.checkpoint import _load_st
    model = LlamaForCausalLM(cfg, "cpu", torch.float32)
    model.load_state_dict(_load_st(os.path.join(ckpt, "model.safetensors")))
    acc = torch.zeros(3, dtype=torch.float64)
    for rank in range(world):
        stream = build_eval_data("synthetic", vocab_size=cfg.vocab_size, seq_len=64, batch_size=4, seed=1337, rank=rank,
                                 world_size=world, device=torch.device("cpu"), eval_dataset_path=None)
        stream.reset()
        b = next(stream)
        acc += model.loss_stats(b["input_ids"], b["labels"])
    return float(acc[0] / acc[1])


@pytest.mark.slow
def test_cli_two_workers_resume_config_and_evaluate(tmp_path):
    """Two gloo workers, 4 steps, H = 2, --logit-softcap 30: stopping at step 2 and resuming (the flag dropped: the
    cap comes from config.json) gives the uninterrupted run bit for bit; config.json carries the key; a mismatching
    --logit-softcap is refused on resume; the stand-alone evaluation of the checkpoint (one process, rank 0's
    held-out data) is the number the model of config.json gives, and the run's own final eval_loss (both ranks'
    held-out data, token-weighted: more than the one-process tool reads) is reproduced from the checkpoint by the same
    model on both ranks' streams."""
    a, b = tmp_path / "a", tmp_path / "b"
    la, lb = tmp_path / "a.jsonl", tmp_path / "b.jsonl"
    run = BASE + ["--logit-softcap", "30"]
    _torchrun(2, run + ["--checkpoint-dir", str(a), "--log-file", str(la)])
    ra = _log(la)
    steps = [x for x in ra if "loss" in x]
    evals = [x for x in ra if "eval_loss" in x]
    assert [x["step"] for x in steps] == [1, 2, 3, 4] and len(evals) == 1 and math.isfinite(evals[0]["eval_loss"])
    with open(a / "config.json") as f:
        cj = json.load(f)
    assert cj["final_logit_softcapping"] == 30.0 and cj["architectures"] == ["LlamaForCausalLM"]
    _torchrun(2, run + ["--stop-at-step", "2", "--checkpoint-dir", str(b), "--checkpoint-every", "1"])
    r = _torchrun(2, BASE + ["--logit-softcap", "20", "--resume", str(b), "--checkpoint-dir", str(b)], ok=False)
    assert "--logit-softcap 20 differs from the checkpoint's final_logit_softcapping (30" in r.stdout + r.stderr
    _torchrun(2, BASE + ["--resume", str(b), "--checkpoint-dir", str(b), "--log-file", str(lb)])
    rb = _log(lb)
    assert [x["step"] for x in rb if "loss" in x] == [3, 4]
    for x, y in zip(steps[2:], [x for x in rb if "loss" in x]):
        assert x["loss"] == y["loss"]
    assert [x["eval_loss"] for x in rb if "eval_loss" in x] == [evals[0]["eval_loss"]]
    for f in ("model.safetensors", "diloco_state.safetensors"):
        ta, tb = _tensors(a / f), _tensors(b / f)
        assert ta.keys() == tb.keys()
        for k in ta:
            assert torch.equal(ta[k], tb[k]), (f, k)
    with open(b / "config.json") as f:
        assert json.load(f)["final_logit_softcapping"] == 30.0
    # evaluation takes the cap from config.json
    cfg = LlamaConfig.from_json(str(a / "config.json"))
    want = _held_out_loss(str(a), cfg, 2)
    assert abs(want - evals[0]["eval_loss"]) <= 1e-12 * abs(want)
    r = subprocess.run([sys.executable, "-m", "nanodiloco_amd.evaluate", "--checkpoint", str(a), "--data", "synthetic",
                        "--eval-batches", "1", "--per-device-batch-size", "4", "--seq-length", "64", "--device", "cpu"],
                       cwd=ROOT, env=child_env(OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["eval_loss"] == _held_out_loss(str(a), cfg, 1)
