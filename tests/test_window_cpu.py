"""Sliding-window attention on the CPU: the reference mask, the config key and its HF spellings, the FLOP count, the
PyTorch path against HF Mistral, generation with and without the cache, and the CLI on two workers."""
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
from nanodiloco_amd.ops import reference as ref
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
from nanodiloco_amd.parallel.diloco import Diloco
from nanodiloco_amd.parallel.dist import DistEnv
from nanodiloco_amd.trainer import check_sliding_window
from nanodiloco_amd.utils.checkpoint import save_checkpoint

from . import _model_oracle as mo
from . import _oracle64 as o64
from ._mp import child_env, free_port
from ._window_oracle import dense_window_mask, kstart_eff, window_doc_start

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
           vocab_size=211, rms_norm_eps=1e-5)
W = 6


def _config(window=W, **kw):
    return LlamaConfig.from_dict(dict(CFG, **({"sliding_window": window} if window else {}), **kw))


def _model(window=W, seed=1, **kw):
    return LlamaForCausalLM(_config(window, **kw)).init_weights(seed)


def _batch(T=16, B=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, CFG["vocab_size"], (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, :5] = 0
    ids[mask == 0] = 2
    labels = ids.clone()
    labels[mask == 0] = -100
    labels[0, 3:6] = -100
    return ids, labels, mask


# ------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("T,window", [(1, 1), (9, 1), (9, 4), (33, 32), (33, 33), (20, 7)])
def test_window_mask_and_helpers(T, window):
    B = 3
    ks = torch.tensor([0, 2, min(T, 11)])
    for kstart in (None, ks):
        dense = dense_window_mask(B, T, window, "cpu", kstart)
        m = ref.window_causal_mask(window, T, kstart, "cpu")
        assert torch.equal(m.expand(B, 1, T, T)[:, 0], dense)
        lo = window_doc_start(B, T, window, "cpu", kstart)
        assert torch.equal(o64.attention_mask(B, T, "cpu", doc_start=lo)[:, 0], dense)
        # the decode bound of the last query is the training bound of row T - 1
        pos = torch.full((B,), T - 1)
        assert torch.equal(kstart_eff(pos, window, kstart).long(), lo[:, -1].long())
    with pytest.raises(ValueError):
        ref.window_causal_mask(0, T)


@pytest.mark.parametrize("window", [1, 5, 16])
def test_reference_attention_block_against_dense_mask_and_oracle(window):
    B, T, nh, nkv, hd = 2, 24, 4, 2, 16
    torch.manual_seed(window)
    qkv = torch.randn(B * T, (nh + 2 * nkv) * hd)
    cos, sin = ref.rope_tables(T, hd, 10000.0)
    ks = torch.tensor([0, 5])
    for kstart in (None, ks):
        o = ref.attention_block(qkv, cos, sin, B, T, nh, nkv, hd, kstart=kstart, window=window)
        # explicit dense mask, explicit math
        q, k, v = ref.split_qkv(qkv, B, T, nh, nkv, hd)
        q, k = ref.apply_rope(q, cos, sin), ref.apply_rope(k, cos, sin)
        k, v = k.repeat_interleave(nh // nkv, 1), v.repeat_interleave(nh // nkv, 1)
        ok = dense_window_mask(B, T, window, "cpu", kstart)[:, None]
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        seen = ok.any(-1, keepdim=True)
        p = torch.softmax(torch.where(seen, s.masked_fill(~ok, float("-inf")), torch.zeros_like(s)), -1) * seen
        want = (p @ v).transpose(1, 2).reshape(B * T, nh * hd)
        assert torch.allclose(o, want, atol=2e-6)
        # the float64 oracle on the rotated rows
        rot = o64.rope(qkv, cos, sin, B, T, nh, nkv, hd)
        r = o64.attention(rot, B, T, nh, nkv, hd, hd ** -0.5, doc_start=window_doc_start(B, T, window, "cpu", kstart))
        assert torch.allclose(o.double(), r["o"], atol=1e-5)
    # a window of T or more keys is no window: today's path, bit for bit
    plain = ref.attention_block(qkv, cos, sin, B, T, nh, nkv, hd)
    for big in (T, T + 3, None, 0):
        assert torch.equal(ref.attention_block(qkv, cos, sin, B, T, nh, nkv, hd, window=big), plain)
    t = torch.arange(T, dtype=torch.int32).expand(B, T)
    with pytest.raises(ValueError):
        ref.attention_block(qkv, cos, sin, B, T, nh, nkv, hd, window=4, doc_bounds=(torch.zeros_like(t), t + 1))
    with pytest.raises(ValueError):
        ops.attention(qkv, cos, sin, B, T, nh, nkv, hd, window=-2)
    with pytest.raises(ValueError):
        ops.attention(qkv, cos, sin, B, T, nh, nkv, hd, window=4, doc_bounds=(torch.zeros_like(t), t + 1))


def test_decode_twin_window():
    from nanodiloco_amd.ops.decode import attention_decode_torch
    B, nh, nkv, hd, S = 2, 4, 2, 16, 20
    torch.manual_seed(0)
    kc, vc = torch.randn(B, nkv, S, hd), torch.randn(B, nkv, S, hd)
    qkv = torch.randn(B, (nh + 2 * nkv) * hd)
    cos, sin = ref.rope_tables(S, hd, 10000.0)
    pos, ks = torch.tensor([12, 7], dtype=torch.int32), torch.tensor([2, 6], dtype=torch.int32)
    a = attention_decode_torch(qkv, cos, sin, pos, ks, kc.clone(), vc.clone(), nh, nkv, hd, window=5)
    b = attention_decode_torch(qkv, cos, sin, pos, kstart_eff(pos, 5, ks), kc.clone(), vc.clone(), nh, nkv, hd)
    assert torch.equal(a, b)
    c = attention_decode_torch(qkv, cos, sin, pos, ks, kc.clone(), vc.clone(), nh, nkv, hd)
    assert not torch.equal(a, c)
    with pytest.raises(ValueError):
        attention_decode_torch(qkv, cos, sin, pos, ks, kc, vc, nh, nkv, hd, window=0)


# ------------------------------------------------------------------------------------------------ config
def test_config_roundtrip_and_hf_spellings():
    c = _config()
    assert c.sliding_window == W and c.to_dict()["sliding_window"] == W
    assert LlamaConfig.from_dict(c.to_dict()).sliding_window == W
    assert LlamaConfig.from_dict(c.to_hf_json()).sliding_window == W
    off = _config(None)
    assert off.sliding_window is None and "sliding_window" not in off.to_dict()
    assert "sliding_window" not in off.to_hf_json() and off.to_hf_json()["model_type"] == "llama"
    assert LlamaConfig.from_dict(dict(CFG, sliding_window=0)).sliding_window is None
    assert LlamaConfig.from_dict(dict(CFG, sliding_window=None)).sliding_window is None
    hf = c.to_hf_json()
    assert (hf["model_type"], hf["architectures"], hf["head_dim"], hf["sliding_window"]) == \
        ("mistral", ["MistralForCausalLM"], 32, W)
    q = _config(qk_norm=True).to_hf_json()
    assert (q["model_type"], q["architectures"]) == ("qwen3", ["Qwen3ForCausalLM"])
    assert (q["sliding_window"], q["use_sliding_window"], q["max_window_layers"]) == (W, True, 0)
    back = LlamaConfig.from_dict(q)
    assert back.sliding_window == W and back.qk_norm
    # a Mistral config as HF writes it
    m = LlamaConfig.from_dict(dict(CFG, model_type="mistral", architectures=["MistralForCausalLM"], sliding_window=4096))
    assert m.sliding_window == 4096 and not m.qk_norm
    # Qwen's switch and first windowed layer
    assert LlamaConfig.from_dict(dict(CFG, model_type="qwen3", sliding_window=64, use_sliding_window=False)).sliding_window is None
    assert LlamaConfig.from_dict(dict(CFG, model_type="qwen3", sliding_window=64, use_sliding_window=True,
                                      max_window_layers=2)).sliding_window is None
    assert LlamaConfig.from_dict(dict(CFG, model_type="qwen3", sliding_window=64)).sliding_window is None  # HF default
    with pytest.raises(ValueError, match="per-layer"):
        LlamaConfig.from_dict(dict(CFG, model_type="qwen3", sliding_window=64, use_sliding_window=True, max_window_layers=1))
    for bad in (-1, 2.5, "8", True):
        with pytest.raises(ValueError, match="sliding_window"):
            LlamaConfig.from_dict(dict(CFG, sliding_window=bad))


def test_flops_per_token():
    T = 1024
    off = _config(None)
    base = off.flops_per_token(T)
    L, qs = off.num_hidden_layers, off.q_size
    for w in (1, 128, 1023):
        got = _config(w).flops_per_token(T)
        assert got == base - 12 * L * qs * T / 2 + 12 * L * qs * w * (2 * T - w) / (2 * T)
        assert got < base
    assert _config(T).flops_per_token(T) == base and _config(4096).flops_per_token(T) == base


def test_start_up_refusals():
    for on_gpu, backend in ((True, "auto"), (False, "auto"), (True, "torch")):
        with pytest.raises(ValueError, match="doc-mask"):
            check_sliding_window(16, True, "synthetic", 64, on_gpu, backend)
    with pytest.raises(ValueError, match="multiple of 64"):
        check_sliding_window(16, False, "memmap", 100, True)
    with pytest.raises(ValueError, match="data hf"):
        check_sliding_window(16, False, "hf", 128, True)
    check_sliding_window(16, False, "hf", 100, False)
    check_sliding_window(16, False, "memmap", 100, True, "torch")
    check_sliding_window(128, False, "memmap", 100, True)  # no window at this length
    check_sliding_window(0, True, "hf", 100, True)
    with pytest.raises(ValueError, match="combined"):
        LlamaForCausalLM(_config(), doc_mask=True)
    with pytest.raises(SystemExit):
        parse_args(["--sliding-window", "16", "--doc-mask"])
    with pytest.raises(SystemExit):
        parse_args(["--sliding-window", "-4"])
    assert parse_args(["--sliding-window", "16"]).sliding_window == 16 and parse_args([]).sliding_window == 0


# ------------------------------------------------------------------------------------------------ HF parity
def _save(m, path):
    d = Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store), 2, 8, 4, env=DistEnv())
    save_checkpoint(str(path), m, d, DistEnv(), step=0)


def test_checkpoint_loads_as_hf_mistral(tmp_path):
    transformers = pytest.importorskip("transformers")
    if not hasattr(transformers, "MistralForCausalLM"):
        pytest.skip("this transformers has no Mistral")
    m = _model()
    _save(m, tmp_path / "ck")
    cfg = json.load(open(tmp_path / "ck" / "config.json"))
    assert cfg["model_type"] == "mistral" and cfg["sliding_window"] == W
    hf = transformers.MistralForCausalLM.from_pretrained(str(tmp_path / "ck"), torch_dtype=torch.float64,
                                                         attn_implementation="sdpa", local_files_only=True)
    assert hf.dtype == torch.float64 and hf.config.sliding_window == W
    names = dict(hf.named_parameters())
    assert set(names) == set(m.store.names)
    assert [n for n in hf.state_dict() if "rotary" not in n] == list(m.state_dict())
    ids, labels, mask = _batch()  # T 16 > W 6
    out = m(ids, labels=labels, attention_mask=mask)
    out.loss.backward()
    ho = hf(input_ids=ids, labels=labels, attention_mask=mask)
    ho.loss.backward()
    assert abs(float(out.loss.detach()) - float(ho.loss.detach())) < 1e-5
    for n, p in names.items():
        assert torch.allclose(p.grad.float(), m.store.grad_view(n), atol=2e-6, rtol=1e-4), n
    logits = m(ids, attention_mask=mask).logits
    sel = mask.bool()
    assert torch.allclose(logits[sel], ho.logits.detach().float()[sel], atol=1e-5)
    # the window is exercised: the same weights without it give another loss
    plain = _model(None)
    plain.load_state_dict(m.state_dict())
    assert abs(float(plain(ids, labels=labels, attention_mask=mask).loss.detach()) - float(out.loss.detach())) > 1e-4
    # the float64 oracle with the window as a lower bound agrees with HF: what the GPU tests are held against
    lower = window_doc_start(ids.shape[0], ids.shape[1], W, "cpu", mo.key_start(mask))
    with torch.no_grad():
        l64 = mo.loss64(mo.logits64(m.config, mo.weights64(m, "cpu"), ids, doc_start=lower), labels)
    assert abs(float(l64) - float(ho.loss.detach())) < 1e-6


# ------------------------------------------------------------------------------------------------ generation
def test_generation_with_and_without_cache():
    m = _model()
    ids, _, mask = _batch(T=9, B=3)
    a = m.generate(ids, attention_mask=mask, max_new_tokens=12, use_cache=True, eos_token_id=None)
    b = m.generate(ids, attention_mask=mask, max_new_tokens=12, use_cache=False, eos_token_id=None)
    assert a.shape == (3, 21) and torch.equal(a, b)
    assert m.new_cache(3, 32).window == W and _model(None).new_cache(3, 32).window is None
    # cached logits against the full recompute of the grown sequence, fp32 on both sides
    seq, cached = m.generate(ids, attention_mask=mask, max_new_tokens=12, eos_token_id=None, return_logits=True)
    full_mask = torch.cat([mask, torch.ones(3, 12, dtype=torch.long)], dim=1)
    m.training = False
    with torch.no_grad():
        for j in range(12):
            L = 9 + j
            full = m(seq[:, :L], attention_mask=full_mask[:, :L]).logits[:, -1]
            assert torch.allclose(cached[:, j], full, atol=1e-4), j
    plain = _model(None)
    plain.load_state_dict(m.state_dict())
    _, lp = plain.generate(ids, attention_mask=mask, max_new_tokens=12, eos_token_id=None, return_logits=True)
    assert not torch.allclose(lp, cached, atol=1e-4)  # the window bites once the sequence outgrows it


# ------------------------------------------------------------------------------------------------ the CLI
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
def test_cli_two_workers_train_and_resume_with_the_window(tmp_path):
    from safetensors.torch import load_file

    from nanodiloco_amd.data.memmap import write_token_shard

    data = tmp_path / "data"
    data.mkdir()
    write_token_shard(str(data / "shard0.bin"), [i % 16 for i in range(1 << 16)])
    a, b, log = tmp_path / "a", tmp_path / "b", tmp_path / "a.jsonl"
    on = ["--sliding-window", "16", "--dataset-path", str(data)]
    _torchrun(on + ["--checkpoint-dir", str(a), "--log-file", str(log)])
    losses = [json.loads(line)["loss"] for line in open(log)]
    assert len(losses) == 8 and all(math.isfinite(x) for x in losses) and losses[-1] < losses[0], losses
    assert json.load(open(a / "trainer_state.json"))["sliding_window"] == 16
    cfg = json.load(open(a / "config.json"))
    assert cfg["sliding_window"] == 16 and cfg["model_type"] == "mistral"
    ta = load_file(str(a / "model.safetensors"))
    _torchrun(on + ["--stop-at-step", "4", "--checkpoint-dir", str(b), "--checkpoint-every", "1"])
    # resumed WITHOUT the flag: the checkpoint's config.json carries the window
    _torchrun(["--dataset-path", str(data), "--resume", str(b), "--checkpoint-dir", str(b)])
    tb = load_file(str(b / "model.safetensors"))
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
    assert json.load(open(b / "config.json"))["sliding_window"] == 16
    # resumed with ANOTHER window: refused, the checkpoint's config.json says what model it holds
    r = _torchrun(["--dataset-path", str(data), "--resume", str(b), "--checkpoint-dir", str(b), "--sliding-window", "8"],
                  check=False)
    assert r.returncode != 0 and "differs from the checkpoint" in r.stderr
    # a run without the flag trains another model and writes no key
    c = tmp_path / "c"
    _torchrun(["--dataset-path", str(data), "--checkpoint-dir", str(c)])
    assert "sliding_window" not in json.load(open(c / "config.json"))
    assert "sliding_window" not in json.load(open(c / "trainer_state.json"))
    tc = load_file(str(c / "model.safetensors"))
    assert any(not torch.equal(ta[k], tc[k]) for k in ta)
    # refused combinations
    r = _torchrun(on + ["--doc-mask"], check=False)
    assert r.returncode != 0 and "doc-mask" in r.stderr
    r = _torchrun(["--sliding-window", "-2", "--dataset-path", str(data)], check=False)
    assert r.returncode != 0
