"""Text generation on the MI355X: bf16, the tiny model (nh = nkv = 4, hd 32) and a GQA model with rep 4 (hd 64), the
HIP path of every op.

The float64 reference of the logits is the plain Llama forward of tests/_model_oracle.py (float64, CPU) on the
bf16-rounded weights the GPU model computes with -- never the code under test.  The cached decode step and the full forward of the same
prefix go through the same bf16 GEMMs and norms and differ in the attention kernel and in where RoPE rounds, so the
cached logits must be as close to the reference as the full-forward logits are: per step,
max|cached - ref| <= 2 max|full - ref|.  docs/PARITY.md (Generation) has the measured ratios.
"""
import json
import subprocess
import sys

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig, resolve_llama_config
from nanodiloco_amd.models import LlamaForCausalLM

from ._frames import _ints
from ._model_oracle import forward64
from ._mp import ROOT, child_env

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
GQA = dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=1, num_hidden_layers=2,
           vocab_size=512, rms_norm_eps=1e-5, max_position_embeddings=512)


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    yield
    ops.set_backend("auto")


def _config(name):
    if name == "tiny":
        c = resolve_llama_config("llama_tiny.json")
        c.vocab_size = 1024
        return c
    return LlamaConfig.from_dict(GQA)


@pytest.mark.parametrize("name", ["tiny", "gqa"])
def test_cached_logits_against_float64(name):
    cfg = _config(name)
    m = LlamaForCausalLM(cfg, DEV, BF16).init_weights(7)
    B, T, n = 2, 16, 8
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(3, cfg.vocab_size, (B, T), generator=g).to(DEV)
    mask = torch.ones(B, T, dtype=torch.long, device=DEV)
    mask[1, :5] = 0  # one left-padded row
    seq, cached = m.generate(ids, mask, max_new_tokens=n, eos_token_id=None, hip_graph=False, return_logits=True)
    full_mask = torch.cat([mask, torch.ones(B, n, dtype=torch.long, device=DEV)], dim=1)
    ref64 = forward64(m, seq.cpu(), ops.key_start(full_mask).cpu())  # float64 on the CPU, as before
    worst = 0.0
    for j in range(n):
        L = T + j
        with torch.no_grad():
            was = m.training
            m.training = False
            full = m(seq[:, :L], attention_mask=full_mask[:, :L]).logits[:, -1]
            m.training = was
        e_full = float((full.double().cpu() - ref64[:, L - 1]).abs().max())
        e_cached = float((cached[:, j].double().cpu() - ref64[:, L - 1]).abs().max())
        worst = max(worst, e_cached / e_full)
        print(f"[{name}] step {j}: cached error {e_cached:.3e}, full-forward error {e_full:.3e}, "
              f"ratio {e_cached / e_full:.2f}")
        assert e_cached <= 2.0 * e_full, (j, e_cached, e_full)
    print(f"[{name}] worst ratio {worst:.2f} (allowed 2)")
    # and the recompute path draws the same greedy tokens wherever the reference's top two are apart
    top2 = ref64[:, T - 1:T + n - 1].topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > 4 * float((cached.double().cpu() - ref64[:, T - 1:T + n - 1]).abs().max())
    assert bool(clear.any())
    assert torch.equal(seq[:, T:].cpu()[clear], ref64[:, T - 1:T + n - 1].argmax(-1)[clear])


@pytest.mark.parametrize("name", ["tiny", "gqa"])
def test_graph_equals_eager(name):
    cfg = _config(name)
    m = LlamaForCausalLM(cfg, DEV, BF16).init_weights(7)
    g = torch.Generator().manual_seed(12)
    ids = torch.randint(3, cfg.vocab_size, (3, 9), generator=g).to(DEV)
    mask = torch.ones(3, 9, dtype=torch.long, device=DEV)
    mask[0, :8] = 0
    mask[2, :4] = 0
    kw = dict(max_new_tokens=21, eos_token_id=None, return_logits=True)  # 20 decode steps after the prefill
    a, la = m.generate(ids, mask, hip_graph=False, **kw)
    b, lb = m.generate(ids, mask, hip_graph=True, **kw)
    c, lc = m.generate(ids, mask, hip_graph="auto", **kw)
    assert torch.equal(a, b) and torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert torch.equal(a, c) and torch.equal(la.view(torch.int32), lc.view(torch.int32))
    # sampling sits outside the graph: the same seed draws the same tokens either way
    kw = dict(max_new_tokens=12, eos_token_id=None, temperature=1.0, top_k=20, seed=3)
    assert torch.equal(m.generate(ids, mask, hip_graph=False, **kw), m.generate(ids, mask, hip_graph=True, **kw))


def _snapshot(m):
    s = {"grad": m.store.grad.clone(), "master": m.store.master.clone(), "shadow": m.store.shadow.clone(),
         "version": m.store.version, "training": m.training}
    if m.fp8 is not None:
        r = m.fp8.recipe
        s.update(amax=r.amax.clone(), hist=r.hist.clone(), scale=r.scale.clone(), inv=r.inv.clone(),
                 ready=list(r.ready), pos=r.pos, n=r.n, wver={k: w.version for k, w in m.fp8.weights.items()})
    return s


def test_fp8_model_generates_on_bf16_projections():
    cfg = _config("tiny")
    m8 = LlamaForCausalLM(cfg, DEV, BF16, fp8=True).init_weights(4)
    mb = LlamaForCausalLM(cfg, DEV, BF16).init_weights(4)
    ids = torch.randint(3, cfg.vocab_size, (2, 64), device=DEV)
    m8(ids, labels=ids).loss.backward()  # live delayed-scaling state and a live grad buffer
    m8.fp8.recipe.update()
    m8(ids, labels=ids).loss.backward()
    torch.cuda.synchronize()
    assert any(m8.fp8.recipe.ready) and bool(m8.fp8.recipe.amax.any()) and bool(m8.store.grad.any())
    before = _snapshot(m8)
    kw = dict(max_new_tokens=10, eos_token_id=None, return_logits=True)
    a, la = m8.generate(ids[:, :12], **kw)
    torch.cuda.synchronize()
    after = _snapshot(m8)
    for k in before:
        if isinstance(before[k], torch.Tensor):
            assert torch.equal(_ints(before[k].reshape(-1)), _ints(after[k].reshape(-1))), k
        else:
            assert before[k] == after[k], k
    assert m8.proj.lm_y8 is None
    b, lb = mb.generate(ids[:, :12], hip_graph=False, **kw)
    assert torch.equal(a, b) and torch.equal(la.view(torch.int32), lb.view(torch.int32))
    with pytest.raises(ValueError):
        from nanodiloco_amd.utils.graphs import GraphedMicroStep
        GraphedMicroStep(m8)  # unchanged: the training graph still refuses fp8


def test_cli_on_gpu(tmp_path):
    from nanodiloco_amd.trainer import TrainArgs, Trainer
    ck = tmp_path / "ck"
    Trainer(TrainArgs(llama_config_file="configs/llama_tiny.json", batch_size=4, per_device_batch_size=4,
                      seq_length=64, warmup_steps=1, total_steps=2, inner_steps=2, wandb="off", device="cuda",
                      data="synthetic", log_every=1, checkpoint_dir=str(ck), seed=3)).train()
    r = subprocess.run([sys.executable, "-m", "nanodiloco_amd.generate", "--checkpoint", str(ck), "--prompt-ids",
                        "1,2,3", "--prompt-ids", "7,8,9,10,11", "--max-new-tokens", "16"], cwd=ROOT, env=child_env(),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.strip().splitlines()]
    assert len(lines) == 3 and lines[0]["token_ids"][:3] == [1, 2, 3] and 1 <= lines[0]["new_tokens"] <= 16
    assert lines[2]["decode_tokens_per_s"] >= 0 and lines[2]["prefill_s"] > 0
