"""The model with ``sliding_window`` on the HIP path: loss and per-parameter gradients against the float64 model
oracle (the window reaches it as ``doc_start[b, t] = max(kstart[b], t - W + 1)``), the exact receptive field, graph
replay, generation with the KV cache, the trainer.

Margins are those of ``test_model_grads_gpu.py`` for its bf16 GQA cases (margin 8, |beta| <= 1e-2, loss floor
7.4e-4); the generation rule is that of ``test_generate_gpu.py`` (per step, max|cached - ref| <= 2 max|full - ref|).
"""
import dataclasses
import math

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM

from . import _model_oracle as mo
from . import _qknorm_oracle as qo
from ._window_oracle import window_doc_start
from .test_model_grads_gpu import BETA_BOUND, LOSS_FLOOR, MARGIN

pytestmark = pytest.mark.gpu

DEV, BF16, SEED = "cuda", torch.bfloat16, 3
W = 48
CFG = dict(hidden_size=128, intermediate_size=384, num_attention_heads=4, num_key_value_heads=2, vocab_size=256,
           num_hidden_layers=2, rms_norm_eps=1e-5, max_position_embeddings=512)
WIN = ["nd_attn_fwd_win", "nd_attn_bwd_fused_win"]
PLAIN = ["nd_attn_fwd", "nd_attn_fwd_ks", "nd_attn_fwd_doc", "nd_attn_bwd", "nd_attn_bwd_ks", "nd_attn_bwd_fused",
         "nd_attn_bwd_fused_ks", "nd_attn_bwd_fused_doc"]


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    det = ops.deterministic()
    ops.set_backend("hip")
    yield
    ops.set_backend("auto")
    ops.set_deterministic(det)


def config(**kw):
    return LlamaConfig.from_dict(dict(CFG, sliding_window=W, **kw))


def batch(masked, B=3, T=128, seed=0):
    g = torch.Generator().manual_seed(100 + masked + 17 * seed)
    ids = torch.randint(3, CFG["vocab_size"], (B, T), generator=g)
    mask = None
    if masked:
        mask = torch.ones(B, T, dtype=torch.long)
        for b, npad in enumerate([0, 5, 11]):
            if npad:
                mask[b, :npad] = 0
        ids[mask == 0] = 2
    labels = ids.clone()
    for b in range(B):
        labels[b, 20 + 9 * b:20 + 9 * b + 12] = -100
    if mask is not None:
        labels[mask == 0] = -100
    return ids.to(DEV), labels.to(DEV), mask.to(DEV) if mask is not None else None


def run(c, backend, ids, labels, mask):
    ops.set_backend(backend)
    m = LlamaForCausalLM(c, DEV, BF16).init_weights(SEED)
    if c.qk_norm:  # ones would hide a q / k weight mix-up (as in test_qknorm_gpu.py)
        g = torch.Generator().manual_seed(11)
        for n in m.store.names:
            if "q_norm" in n or "k_norm" in n:
                v = m.store.master_view(n)
                v.copy_((0.5 + torch.rand(v.shape, generator=g)).to(DEV))
        m.store.sync_shadow()
    out = m(ids, labels=labels, attention_mask=mask)
    out.loss.backward()
    torch.cuda.synchronize()
    return float(out.loss.detach()), mo.model_grads(m), m


def grads64_window(m, ids, labels, lower):
    """``_model_oracle.grads64`` with an explicit per-query lower bound."""
    c = m.config
    P = {k: v.requires_grad_(True) for k, v in mo.weights64(m, ids.device).items()}
    logits64 = qo.logits64 if c.qk_norm else mo.logits64
    loss = mo.loss64(logits64(c, P, ids, doc_start=lower), labels)
    keys = list(P)
    gs = dict(zip(keys, torch.autograd.grad(loss, [P[k] for k in keys])))
    out = {k: g for k, g in gs.items() if k not in ("embed", "lm")}
    out["model.embed_tokens.weight"], out["lm_head.weight"] = gs["embed"], gs["lm"]
    return float(loss.detach()), out


def _against_float64(c, masked, case, ran, never):
    """The HIP model's loss and per-parameter gradients under ``check_loss`` / ``check_grads`` of
    ``test_model_grads_gpu.py`` (its margins): oracle = the float64 model with the window as a lower bound, twin = the
    same model on the PyTorch path."""
    ids, labels, mask = batch(masked)
    B, T = ids.shape
    logits64 = qo.logits64 if c.qk_norm else mo.logits64
    l_twin, g_twin, m = run(c, "torch", ids, labels, mask)
    ks = mo.key_start(mask) if mask is not None else None
    l64, g64 = grads64_window(m, ids, labels, window_doc_start(B, T, W, DEV, ks))
    # the window is exercised: the un-windowed oracle's loss is another number
    with torch.no_grad():
        l_full = float(mo.loss64(logits64(c, mo.weights64(m, DEV), ids, kstart=ks), labels))
    assert abs(l_full - l64) > 1e-4
    with mo.spying() as spy:
        l, g, _ = run(c, "hip", ids, labels, mask)
    spy.expect(ran=ran, at_least=c.num_hidden_layers, never=never, case=case)
    report = {}
    err = None
    try:
        mo.check_grads(g, g64, g_twin, MARGIN, BETA_BOUND, report, case)
    except AssertionError as e:
        err = e
    worst = max(report.items(), key=lambda kv: (kv[1]["margin"] != kv[1]["margin"], kv[1]["margin"]))
    wb = max(report.items(), key=lambda kv: kv[1]["beta"])
    print(f"[window-model] {case} masked={masked}: margin {worst[1]['margin']:.2f} ({worst[0]}), |beta| "
          f"{wb[1]['beta']:.2e} ({wb[0]}), loss err {abs(l - l64):.2e}, twin loss err {abs(l_twin - l64):.2e}")
    if err is not None:
        raise err
    mo.check_loss(l, l64, l_twin, MARGIN, LOSS_FLOOR, case)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "left_padded"])
def test_loss_and_gradients_against_float64(masked):
    _against_float64(config(), masked, "window", WIN, PLAIN)


def test_qk_norm_with_window_against_float64():
    """QK-norm + window: ``ops.qk_norm_rope`` feeds the windowed kernels unchanged.  Held to the same rule and
    margins, against the float64 QK-norm model (``_qknorm_oracle.logits64``) with the window as a lower bound."""
    _against_float64(config(qk_norm=True), True, "window/qk_norm", WIN + ["nd_qk_norm_rope_fwd", "nd_qk_norm_bwd"],
                     PLAIN + ["nd_rope_inplace", "nd_gemm_pp_rope"])


def test_receptive_field_exact():
    """L layers of window W: token 0 reaches positions <= L (W - 1) and no further, bit for bit."""
    small = 16
    c = dataclasses.replace(config(), sliding_window=small)
    L = c.num_hidden_layers
    ops.set_deterministic(True)
    m = LlamaForCausalLM(c, DEV, BF16).init_weights(SEED)
    m.training = False
    ids = torch.randint(3, 256, (2, 128), generator=torch.Generator().manual_seed(5)).to(DEV)
    ids2 = ids.clone()
    ids2[:, 0] = (ids[:, 0] + 7) % 250 + 3
    with torch.no_grad():
        a, b = m(ids).logits, m(ids2).logits
    reach = L * (small - 1)
    assert torch.equal(a[:, reach + 1:], b[:, reach + 1:]), "token 0 was seen beyond L (W - 1)"
    assert not torch.equal(a[:, reach], b[:, reach]), "token 0 did not reach position L (W - 1)"


def test_graphed_micro_step_bitwise():
    from nanodiloco_amd.utils.graphs import GraphedMicroStep
    c = config()
    ops.set_deterministic(True)  # bitwise claims need the deterministic reductions, as in test_docmask_gpu.py
    batches = [batch(False, seed=i)[:2] for i in range(4)]  # the first replay comes after the warm-up steps
    eager = LlamaForCausalLM(c, DEV, BF16).init_weights(SEED)
    le = []
    for ids, labels in batches:
        out = eager(ids, labels=labels)
        out.loss.backward()
        le.append(out.loss.detach().clone())
    m = LlamaForCausalLM(c, DEV, BF16).init_weights(SEED)
    step = GraphedMicroStep(m)
    lg = [step(ids, labels, 1.0).clone() for ids, labels in batches]
    torch.cuda.synchronize()
    assert step.graph is not None and step.eager_fallbacks == 0
    assert step.warmup < len(batches)
    assert all(torch.equal(x, y) for x, y in zip(le, lg)), (le, lg)
    assert len({float(x) for x in le}) == len(le)  # every replay followed its own batch
    assert torch.equal(eager.store.grad, m.store.grad)


def test_generation_against_full_windowed_forward():
    """Prefill of a left-padded batch at T 70 (the register-staged windowed forward), then 40 cached decode steps: each
    step's logits against the float64 model with the window on the grown sequence, by test_generate_gpu.py's rule."""
    c = dataclasses.replace(config(), sliding_window=32)
    m = LlamaForCausalLM(c, DEV, BF16).init_weights(7)
    B, T, n, Wg = 2, 70, 40, 32
    ids = torch.randint(3, 256, (B, T), generator=torch.Generator().manual_seed(11)).to(DEV)
    mask = torch.ones(B, T, dtype=torch.long, device=DEV)
    mask[1, :5] = 0
    with mo.spying() as spy:
        seq, cached = m.generate(ids, mask, max_new_tokens=n, eos_token_id=None, hip_graph=False, return_logits=True)
    spy.expect(ran=["nd_attn_fwd_win", "nd_attn_decode_win"], never=["nd_attn_decode", "nd_attn_fwd_ks"], case="generate")
    full_mask = torch.cat([mask, torch.ones(B, n, dtype=torch.long, device=DEV)], dim=1)
    lower = window_doc_start(B, T + n, Wg, "cpu", mo.key_start(full_mask).cpu())
    with torch.no_grad():
        ref64 = mo.logits64(c, mo.weights64(m, "cpu"), seq.cpu(), doc_start=lower)
    worst = 0.0
    m.training = False
    for j in range(n):
        L = T + j
        with torch.no_grad():
            full = m(seq[:, :L], attention_mask=full_mask[:, :L]).logits[:, -1]
        e_full = float((full.double().cpu() - ref64[:, L - 1]).abs().max())
        e_cached = float((cached[:, j].double().cpu() - ref64[:, L - 1]).abs().max())
        worst = max(worst, e_cached / e_full)
        assert e_cached <= 2.0 * e_full, (j, e_cached, e_full)
    print(f"[window-model] generation: worst cached / full error ratio {worst:.2f} (allowed 2)")


def _trainer(**kw):
    from nanodiloco_amd.trainer import TrainArgs, Trainer
    base = dict(llama_config_file="configs/llama_tiny.json", batch_size=8, per_device_batch_size=4, seq_length=64,
                warmup_steps=1, total_steps=4, inner_steps=4, lr=2e-3, wandb="off", device="cuda", dtype="bf16",
                data="synthetic", log_every=0, deterministic=True)
    base.update(kw)
    return Trainer(TrainArgs(**base))


def test_trainer_trains_with_a_window():
    t = _trainer(sliding_window=32)
    assert t.llama_config.sliding_window == 32 and t.model.config.sliding_window == 32
    ids = torch.randint(0, 512, (4, 64), generator=torch.Generator().manual_seed(11)).to(DEV)
    b = {"input_ids": ids, "labels": ids}
    t.data = iter(lambda: b, None)
    t.model.train()
    with mo.spying() as spy:
        losses = [float(t.inner_step()) for _ in range(4)]
    spy.expect(ran=WIN, never=PLAIN, case="trainer")
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0], losses


def test_trainer_start_up_refusals():
    from nanodiloco_amd.trainer import check_sliding_window
    with pytest.raises(ValueError, match="doc-mask"):
        check_sliding_window(32, True, "synthetic", 64, True)
    with pytest.raises(ValueError, match="multiple of 64"):
        check_sliding_window(32, False, "synthetic", 96, True)
    with pytest.raises(ValueError, match="data hf"):
        check_sliding_window(32, False, "hf", 64, True)
    with pytest.raises(ValueError, match="multiple of 64"):
        _trainer(sliding_window=32, seq_length=96)
    with pytest.raises(ValueError, match="doc-mask"):
        _trainer(sliding_window=32, doc_mask=True)
    with pytest.raises(ValueError, match="data hf"):
        _trainer(sliding_window=32, data="hf")
    # not a window at this length, the CPU, --ops torch: allowed (doc-mask never)
    check_sliding_window(128, False, "hf", 96, True)
    check_sliding_window(32, False, "hf", 96, False)
    check_sliding_window(32, False, "hf", 96, True, "torch")
    with pytest.raises(ValueError, match="doc-mask"):
        check_sliding_window(32, True, "synthetic", 64, False)
