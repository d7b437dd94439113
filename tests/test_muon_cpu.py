"""Muon inner optimizer on the CPU: the Newton-Schulz iteration, ``FlatMuon`` against an independent per-tensor loop,
its AdamW part against ``FlatAdamW`` bit for bit, the device-side skip, and the CLI (train, resume, refusal)."""
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
from nanodiloco_amd.models.llama import LlamaForCausalLM
from nanodiloco_amd.optim import FlatAdamW, FlatMuon

from ._mp import child_env, free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUON_SUFFIXES = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "o_proj.weight", "gate_proj.weight",
                 "up_proj.weight", "down_proj.weight")


def _is_muon(name):
    return ".layers." in name and name.endswith(MUON_SUFFIXES)


def _gauss(shape, seed, dtype=torch.float64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ------------------------------------------------------------------------------------------------ 1. the iteration
@pytest.mark.parametrize("shape", [(96, 160), (160, 96), (64, 256)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_newton_schulz_singular_values(shape, seed):
    """Five steps of the (3.4445, -4.7750, 2.0315) iteration bring every singular value of a Gaussian matrix into
    [0.65, 1.20] (the reference iteration, float64: [0.682, 1.134] on all nine)."""
    Y = ops.newton_schulz(_gauss(shape, seed), 5)
    assert Y.shape == shape and Y.dtype == torch.float64
    s = torch.linalg.svdvals(Y)
    print(f"{shape} seed {seed}: singular values in [{float(s.min()):.4f}, {float(s.max()):.4f}]")
    assert float(s.min()) >= 0.65 and float(s.max()) <= 1.20


def test_newton_schulz_keeps_rank():
    X = _gauss((96, 4), 0) @ _gauss((4, 160), 1)
    s = torch.linalg.svdvals(ops.newton_schulz(X, 5))
    assert int((s > 0.5).sum()) == 4, s[:8]


def test_newton_schulz_batched_equals_single():
    X = torch.stack([_gauss((24, 40), s, torch.float32) for s in range(3)])
    Y = ops.newton_schulz(X, 5)
    for i in range(3):
        torch.testing.assert_close(Y[i], ops.newton_schulz(X[i], 5), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 2.-4. FlatMuon
def _model(seed=0):
    cfg = LlamaConfig(vocab_size=96, hidden_size=64, intermediate_size=160, num_attention_heads=4,
                      num_key_value_heads=2, num_hidden_layers=2, max_position_embeddings=64)
    return LlamaForCausalLM(cfg, "cpu", torch.float32).init_weights(seed)


def _fill_grad(store, seed, scale=0.05):
    """A gradient on every parameter (padding stays zero, as the backward leaves it)."""
    g = torch.Generator().manual_seed(seed)
    store.grad.zero_()
    for n in store.names:
        v = store.grad_view(n)
        v.copy_(torch.randn(v.shape, generator=g) * scale)


def _reference_muon(W, G, M, coef, lr, wd, mu=0.95, steps=5):
    """Muon on one tensor, written from the algorithm's text (fp32, nothing rounded to bf16)."""
    a, b, c = 3.4445, -4.7750, 2.0315
    M.mul_(mu).add_(coef * G)
    U = coef * G + mu * M
    X = U / (U.norm() + 1e-7)
    m, n = W.shape
    if m > n:
        X = X.t()
    for _ in range(steps):
        A = X @ X.t()
        B = b * A + c * (A @ A.t())
        X = a * X + B @ X
    if m > n:
        X = X.t()
    W.mul_(1 - lr * wd).sub_(lr * 0.2 * math.sqrt(max(m, n)) * X)


def test_flat_muon_equals_per_tensor_loop():
    m = _model()
    st = m.store
    opt = FlatMuon(st, lr=1e-3)
    ref_w = {n: st.master_view(n).clone() for n in st.names if _is_muon(n)}
    ref_m = {n: torch.zeros_like(w) for n, w in ref_w.items()}
    assert len(ref_w) == 14 and sorted(opt.plan.muon_names) == sorted(ref_w)
    lr, wd = 2e-3, 0.01
    for step in range(3):
        _fill_grad(st, 10 + step, scale=0.05 * (step + 1))  # the clip is active from the first step
        total = st.grad.norm()
        coef = torch.clamp(1.0 / (total + 1e-6), max=1.0)
        assert float(coef) < 1.0
        for n in ref_w:
            _reference_muon(ref_w[n], st.grad_view(n), ref_m[n], coef, lr, wd)
        opt.step(lr)
        assert float(opt.last_grad_norm) == float(total)
    for n in ref_w:
        a, b = st.range(n)
        torch.testing.assert_close(st.master_view(n), ref_w[n], rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(opt.exp_avg[a:b].view(ref_m[n].shape), ref_m[n], rtol=1e-5, atol=1e-9)
        assert not opt.exp_avg_sq[a:b].any()  # the Muon spans keep no second moment
    assert opt.step_count == 3 and st.version >= 3


def test_flat_muon_adamw_part_is_bitwise_flat_adamw():
    ma, mb = _model(), _model()
    oa, ob = FlatAdamW(ma.store, lr=1e-3), FlatMuon(mb.store, lr=1e-3)
    assert torch.equal(ma.store.master, mb.store.master)
    for step in range(2):
        _fill_grad(ma.store, 20 + step, scale=0.1)
        mb.store.grad.copy_(ma.store.grad)
        oa.step(1e-3)
        ob.step(1e-3)
        assert torch.equal(oa.last_grad_norm, ob.last_grad_norm)
    rest = [n for n in ma.store.names if not _is_muon(n)]
    assert "model.embed_tokens.weight" in rest and "model.norm.weight" in rest
    for n in rest:
        a, b = ma.store.range(n)
        assert torch.equal(ma.store.master[a:b], mb.store.master[a:b]), n
        assert torch.equal(oa.exp_avg[a:b], ob.exp_avg[a:b]), n
        assert torch.equal(oa.exp_avg_sq[a:b], ob.exp_avg_sq[a:b]), n
    n = "model.layers.0.self_attn.q_proj.weight"
    assert not torch.equal(ma.store.master_view(n), mb.store.master_view(n))  # Muon did run


def test_flat_muon_skip_nonfinite():
    m = _model()
    st = m.store
    opt = FlatMuon(st, lr=1e-3, skip_nonfinite=True)
    _fill_grad(st, 3)
    opt.step(1e-3)
    w0, m0, v0 = st.master.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    st.grad_view("model.layers.1.mlp.up_proj.weight")[3, 5] = float("nan")
    opt.step(1e-3)
    assert torch.equal(st.master, w0) and torch.equal(opt.exp_avg, m0) and torch.equal(opt.exp_avg_sq, v0)
    assert int(opt.skipped_steps) == 1
    _fill_grad(st, 4)
    opt.step(1e-3)
    assert not torch.equal(st.master, w0) and int(opt.skipped_steps) == 1


def test_flat_muon_state_dict_roundtrip():
    m = _model()
    opt = FlatMuon(m.store, lr=1e-3)
    _fill_grad(m.store, 5)
    opt.step(1e-3)
    sd = opt.state_dict()
    assert set(sd) >= {"exp_avg", "exp_avg_sq", "step", "momentum", "ns_steps"}
    other = FlatMuon(_model().store, lr=1e-3)
    other.load_state_dict(sd)
    assert other.step_count == 1 and torch.equal(other.exp_avg, opt.exp_avg)


# ------------------------------------------------------------------------------------------------ 5. the CLI
BASE = ["--llama-config-file", "configs/llama_tiny.json", "--batch-size", "8", "--per-device-batch-size", "4",
        "--seq-length", "64", "--warmup-steps", "2", "--wandb", "off", "--device", "cpu", "--data", "memmap",
        "--inner-steps", "4", "--total-steps", "8", "--lr", "2e-3"]


def _torchrun(args, check=True):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), "-m", "nanodiloco_amd"] + BASE + args
    r = subprocess.run(cmd, cwd=ROOT, env=child_env(OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=600)
    if check:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


@pytest.mark.slow
def test_cli_muon_trains_resumes_and_refuses_adamw(tmp_path):
    from safetensors.torch import load_file

    from nanodiloco_amd.data.memmap import write_token_shard

    # a learnable stream (the synthetic one is uniform noise: no optimizer lowers its loss in 8 steps)
    data = tmp_path / "data"
    data.mkdir()
    write_token_shard(str(data / "shard0.bin"), [i % 16 for i in range(1 << 16)])
    a, b, log = tmp_path / "a", tmp_path / "b", tmp_path / "a.jsonl"
    muon = ["--inner-optimizer", "muon", "--dataset-path", str(data)]
    _torchrun(muon + ["--checkpoint-dir", str(a), "--log-file", str(log)])
    losses = [json.loads(line)["loss"] for line in open(log)]
    assert len(losses) == 8 and all(math.isfinite(x) for x in losses)
    assert losses[-1] < losses[0], losses
    assert json.load(open(a / "trainer_state.json"))["inner_optimizer"] == "muon"
    _torchrun(muon + ["--stop-at-step", "4", "--checkpoint-dir", str(b), "--checkpoint-every", "1"])
    mid = str(tmp_path / "mid")
    subprocess.run(["cp", "-r", str(b), mid], check=True)
    _torchrun(muon + ["--resume", str(b), "--checkpoint-dir", str(b)])
    ta, tb = load_file(str(a / "model.safetensors")), load_file(str(b / "model.safetensors"))
    assert ta.keys() == tb.keys()
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
    r = _torchrun(["--inner-optimizer", "adamw", "--dataset-path", str(data), "--resume", mid], check=False)
    assert r.returncode != 0
    assert "--inner-optimizer muon" in r.stdout + r.stderr
    # a checkpoint without the key is an AdamW checkpoint
    st = json.load(open(os.path.join(mid, "trainer_state.json")))
    del st["inner_optimizer"]
    json.dump(st, open(os.path.join(mid, "trainer_state.json"), "w"))
    r = _torchrun(muon + ["--resume", mid], check=False)
    assert r.returncode != 0 and "--inner-optimizer adamw" in r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ 6. the parser
def test_parser_defaults_and_choices(capsys):
    a = parse_args([])
    assert (a.inner_optimizer, a.muon_momentum, a.muon_ns_steps) == ("adamw", 0.95, 5)
    a = parse_args(["--inner-optimizer", "muon", "--muon-momentum", "0.9", "--muon-ns-steps", "3"])
    assert (a.inner_optimizer, a.muon_momentum, a.muon_ns_steps) == ("muon", 0.9, 3)
    with pytest.raises(SystemExit):
        parse_args(["--inner-optimizer", "lion"])
    assert "invalid choice" in capsys.readouterr().err
