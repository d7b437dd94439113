"""QK-norm on the CPU: the config key and the parameter list, the PyTorch path against the float64 oracle and against
HF Qwen3, generation with and without the cache, what the optimizer / transport plans do with the new tensors, and
the CLI on two workers (train, stop, resume bit for bit)."""
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
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
from nanodiloco_amd.parallel.diloco import Diloco
from nanodiloco_amd.parallel.dist import DistEnv
from nanodiloco_amd.parallel.fragments import plan_fragments
from nanodiloco_amd.utils.checkpoint import save_checkpoint

from . import _model_oracle as mo
from . import _oracle64 as o64
from . import _qknorm_oracle as qo
from ._mp import child_env, free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 2 layers, d128, 4 query / 2 kv heads: hd 32
CFG = dict(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
           vocab_size=211, rms_norm_eps=1e-5)


def _config(on=True, **kw):
    return LlamaConfig.from_dict(dict(CFG, **({"qk_norm": True} if on else {}), **kw))


def _model(on=True, seed=1, perturb=True, **kw):
    m = LlamaForCausalLM(_config(on, **kw)).init_weights(seed)
    if on and perturb:  # ones would hide a q / k weight mix-up and a missing weight factor in dx
        g = torch.Generator().manual_seed(7)
        for n in m.store.names:
            if "q_norm" in n or "k_norm" in n:
                m.store.master_view(n).copy_(0.5 + torch.rand(m.store.master_view(n).shape, generator=g))
        m.store.sync_shadow()
    return m


def _batch(T=16, B=3, seed=0):
    """ids, labels and an attention mask whose row 1 is left-padded by 5."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, CFG["vocab_size"], (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, :5] = 0
    ids[mask == 0] = 2
    labels = ids.clone()
    labels[mask == 0] = -100
    labels[0, 3:6] = -100
    return ids, labels, mask


# ------------------------------------------------------------------------------------------------ config
def test_config_roundtrip_and_qwen3_detection():
    c = _config()
    assert c.qk_norm and c.to_dict()["qk_norm"] is True
    assert LlamaConfig.from_dict(c.to_dict()).qk_norm
    assert LlamaConfig.from_dict(c.to_hf_json()).qk_norm
    assert not _config(False).qk_norm
    assert LlamaConfig.from_dict(dict(CFG, model_type="qwen3")).qk_norm
    assert LlamaConfig.from_dict(dict(CFG, architectures=["Qwen3ForCausalLM"])).qk_norm
    assert not LlamaConfig.from_dict(dict(CFG, architectures=["LlamaForCausalLM"], model_type="llama")).qk_norm
    hf = c.to_hf_json()
    assert (hf["model_type"], hf["architectures"], hf["head_dim"]) == ("qwen3", ["Qwen3ForCausalLM"], 32)


def test_off_is_what_it_was():
    """Without the key nothing names QK-norm: the dicts, the parameter list and the state dict are today's."""
    c = _config(False)
    assert "qk_norm" not in c.to_dict() and "qk_norm" not in c.to_hf_json()
    assert c.to_hf_json()["model_type"] == "llama" and c.to_hf_json()["architectures"] == ["LlamaForCausalLM"]
    names = [n for n, _ in c.param_shapes()]
    assert not any("q_norm" in n or "k_norm" in n for n in names)
    per_layer = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
                 "mlp.up_proj", "mlp.down_proj", "input_layernorm", "post_attention_layernorm"]
    want = ["model.embed_tokens.weight"] + [f"model.layers.{i}.{k}.weight" for i in range(2) for k in per_layer] \
        + ["model.norm.weight", "lm_head.weight"]
    assert names == want
    assert list(LlamaForCausalLM(c).state_dict()) == want


def test_on_names_order_shapes_and_count():
    on, off = _config(), _config(False)
    shapes = on.param_shapes()
    names = [n for n, _ in shapes]
    for i in range(2):
        p = f"model.layers.{i}.self_attn."
        k = names.index(p + "o_proj.weight")
        assert names[k - 3:k + 4] == [p + "q_proj.weight", p + "k_proj.weight", p + "v_proj.weight", p + "o_proj.weight",
                                      p + "q_norm.weight", p + "k_norm.weight", f"model.layers.{i}.mlp.gate_proj.weight"]
        assert dict(shapes)[p + "q_norm.weight"] == (32,) and dict(shapes)[p + "k_norm.weight"] == (32,)
    assert [n for n in names if "_norm." not in n] == [n for n, _ in off.param_shapes()]
    assert on.num_params() == off.num_params() + 2 * 32 * 2
    m = LlamaForCausalLM(on).init_weights(0)
    assert list(m.state_dict()) == names
    assert bool((m.store.master_view("model.layers.1.self_attn.k_norm.weight") == 1).all())  # a norm weight: ones
    # q|k|v still adjacent: the fused view is the three projections
    assert m._fused(m._qkv_names[0], "shadow").shape == (128 + 64 + 64, 128)


def test_parser_flag():
    assert parse_args([]).qk_norm is False
    assert parse_args(["--qk-norm"]).qk_norm is True


# ------------------------------------------------------------------------------------------------ ops on the CPU
@pytest.mark.parametrize("nh,nkv,hd", [(4, 2, 32), (1, 1, 64), (3, 3, 16)])
def test_torch_ops_match_oracle(nh, nkv, hd):
    g = torch.Generator().manual_seed(nh * 100 + hd)
    B, T = 2, 7
    W = (nh + 2 * nkv) * hd
    x = torch.randn(B * T, W, generator=g)
    x[3, hd:2 * hd] = 0  # an all-zero head
    wq, wk = 0.5 + torch.rand(hd, generator=g), 0.5 + torch.rand(hd, generator=g)
    wq[1] = 0.0
    dy = torch.randn(B * T, W, generator=g)
    ref = qo.qk_norm(x, wq, wk, nh, nkv, hd, 1e-5, dy=dy)
    y = ops.qk_norm(x.clone(), wq, wk, nh, nkv, hd, 1e-5)
    assert torch.allclose(y.double(), ref["y"], atol=1e-5, rtol=1e-5)
    assert torch.equal(y[:, (nh + nkv) * hd:], x[:, (nh + nkv) * hd:])
    cos, sin = ops.rope_cache(T, hd, 10000.0, None, "cpu")
    gwq, gwk = torch.full((hd,), 0.25), torch.full((hd,), -0.5)
    xin = x.clone().requires_grad_(True)
    out, rotated = ops.qk_norm_rope(xin, wq, wk, gwq, gwk, cos, sin, T, nh, nkv, hd, 1e-5)
    assert rotated is False and torch.equal(out, y)  # the CPU path: normed, un-rotated
    out.backward(dy)
    assert torch.allclose(xin.grad.double(), ref["dx"], atol=1e-5, rtol=1e-5)
    assert torch.equal(xin.grad[:, (nh + nkv) * hd:], dy[:, (nh + nkv) * hd:])
    assert torch.allclose(gwq.double(), 0.25 + ref["dwq"], atol=1e-5, rtol=1e-5)  # accumulated, beta = 1
    assert torch.allclose(gwk.double(), -0.5 + ref["dwk"], atol=1e-5, rtol=1e-5)
    assert bool(torch.isfinite(xin.grad).all())


def test_oracle_backward_is_the_derivative():
    """The oracle's hand-written backward against autograd through its own forward, in float64."""
    nh, nkv, hd = 2, 1, 8
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, (nh + 2 * nkv) * hd, generator=g, dtype=torch.float64, requires_grad=True)
    wq = torch.rand(hd, generator=g, dtype=torch.float64, requires_grad=True)
    wk = torch.rand(hd, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(5, (nh + 2 * nkv) * hd, generator=g, dtype=torch.float64)
    ref = qo.qk_norm(x, wq, wk, nh, nkv, hd, 1e-5, dy=dy)
    gx, gq, gk = torch.autograd.grad((ref["y"] * dy).sum(), [x, wq, wk])
    for a, b in ((gx, ref["dx"]), (gq, ref["dwq"]), (gk, ref["dwk"])):
        assert torch.allclose(a, b.detach(), atol=1e-12, rtol=1e-10)


# ------------------------------------------------------------------------------------------------ the model
def test_torch_path_matches_float64_oracle():
    m = _model()
    ids, labels, mask = _batch()
    out = m(ids, labels=labels, attention_mask=mask)
    out.loss.backward()
    l64, g64 = qo.grads64(m, ids, labels, kstart=mo.key_start(mask))
    assert abs(float(out.loss.detach()) - float(l64)) < 1e-5
    assert set(g64) == set(m.store.names)
    for n in m.store.names:
        assert torch.allclose(m.store.grad_view(n).double(), g64[n], atol=2e-6, rtol=1e-4), n
    for i in range(2):
        for k in ("q_norm", "k_norm"):
            assert bool(g64[f"model.layers.{i}.self_attn.{k}.weight"].any())
    # and it is not the model without the norms
    l_plain = mo.loss64(mo.forward64(m, ids, kstart=mo.key_start(mask)), labels)
    assert abs(float(l_plain) - float(l64)) > 1e-4


def _save(m, path):
    d = Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store), 2, 8, 4, env=DistEnv())
    save_checkpoint(str(path), m, d, DistEnv(), step=0)


def test_checkpoint_loads_as_hf_qwen3(tmp_path):
    transformers = pytest.importorskip("transformers")
    if not hasattr(transformers, "Qwen3ForCausalLM"):
        pytest.skip("this transformers has no Qwen3")
    m = _model()
    _save(m, tmp_path / "ck")
    cfg = json.load(open(tmp_path / "ck" / "config.json"))
    assert cfg["model_type"] == "qwen3" and cfg["qk_norm"] is True
    hf = transformers.Qwen3ForCausalLM.from_pretrained(str(tmp_path / "ck"), torch_dtype=torch.float64,
                                                       attn_implementation="sdpa", local_files_only=True)
    assert hf.dtype == torch.float64
    names = dict(hf.named_parameters())
    assert set(names) == set(m.store.names)
    assert [n for n in hf.state_dict() if "rotary" not in n] == list(m.state_dict())  # HF Qwen3's own order
    ids, labels, mask = _batch()
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
    # the float64 oracle agrees with the same HF model's loss: what the GPU tests are held against
    l64, _ = qo.grads64(m, ids, labels, kstart=mo.key_start(mask))
    assert abs(float(l64) - float(ho.loss.detach())) < 1e-6


def test_generation_with_and_without_cache():
    m = _model()
    ids, _, mask = _batch(T=9, B=3)
    a = m.generate(ids, attention_mask=mask, max_new_tokens=12, use_cache=True, eos_token_id=None)
    b = m.generate(ids, attention_mask=mask, max_new_tokens=12, use_cache=False, eos_token_id=None)
    assert a.shape == (3, 21) and torch.equal(a, b)
    plain = _model(on=False).generate(ids, attention_mask=mask, max_new_tokens=12, eos_token_id=None)
    assert not torch.equal(a, plain)


# ------------------------------------------------------------------------------------------------ plans
def test_plans_treat_the_new_tensors_as_norm_weights():
    m = _model()
    st = m.store
    new = [n for n in st.names if "q_norm" in n or "k_norm" in n]
    assert len(new) == 4
    plan = ops.MuonPlan.from_store(st)
    assert not set(new) & set(plan.muon_names)
    muon_offsets = {off for offs in plan.groups.values() for off in offs}
    for n in new:
        a, b = st.range(n)
        assert a not in muon_offsets
        assert any(s <= a and b <= e for s, e in plan.adamw.spans), n
        ia, ib = st.range(n.replace("self_attn.q_norm", "input_layernorm").replace("self_attn.k_norm", "input_layernorm"))
        assert any(s <= ia and ib <= e for s, e in plan.adamw.spans)
    low = ops.LowRankPlan(st.names, st.shapes, st.offsets, rank=4)
    assert not set(new) & set(low.mat_names)
    for n in new:
        a, b = st.range(n)
        assert any(s <= a and b <= e for s, e in low.dense), n
    frags = plan_fragments(st, 2, 2, "strided")
    for n in new:
        layer = int(n.split(".")[2])
        a, b = st.range(n)
        owners = [p for p, spans in enumerate(frags) if any(s <= a and b <= e for s, e in spans)]
        assert owners == [layer % 2], (n, owners)
        la, lb = st.span(f"model.layers.{layer}.")
        assert la <= a and b <= lb  # inside the layer's span (inner DDP's bucket, the layer hook)


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
def test_cli_two_workers_train_stop_resume_bitwise(tmp_path):
    from safetensors.torch import load_file

    from nanodiloco_amd.data.memmap import write_token_shard

    data = tmp_path / "data"
    data.mkdir()
    write_token_shard(str(data / "shard0.bin"), [i % 16 for i in range(1 << 16)])
    a, b, log = tmp_path / "a", tmp_path / "b", tmp_path / "a.jsonl"
    on = ["--qk-norm", "--dataset-path", str(data)]
    _torchrun(on + ["--checkpoint-dir", str(a), "--log-file", str(log)])
    losses = [json.loads(line)["loss"] for line in open(log)]
    assert len(losses) == 8 and all(math.isfinite(x) for x in losses) and losses[-1] < losses[0], losses
    assert json.load(open(a / "trainer_state.json"))["qk_norm"] is True
    cfg = json.load(open(a / "config.json"))
    assert cfg["qk_norm"] is True and cfg["model_type"] == "qwen3"
    ta = load_file(str(a / "model.safetensors"))
    qn = "model.layers.1.self_attn.q_norm.weight"
    assert ta[qn].shape == (32,) and not bool((ta[qn] == 1).all())  # the new weights are trained
    _torchrun(on + ["--stop-at-step", "4", "--checkpoint-dir", str(b), "--checkpoint-every", "1"])
    # resumed WITHOUT the flag: the checkpoint's config.json builds the QK-norm model
    _torchrun(["--dataset-path", str(data), "--resume", str(b), "--checkpoint-dir", str(b)])
    tb = load_file(str(b / "model.safetensors"))
    assert ta.keys() == tb.keys()
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
    assert json.load(open(b / "trainer_state.json"))["qk_norm"] is True
    # a run without the flag has neither the tensors nor the keys
    c = tmp_path / "c"
    _torchrun(["--dataset-path", str(data), "--checkpoint-dir", str(c), "--total-steps", "4"])
    assert "qk_norm" not in json.load(open(c / "trainer_state.json"))
    assert "qk_norm" not in json.load(open(c / "config.json"))
    assert qn not in load_file(str(c / "model.safetensors"))
