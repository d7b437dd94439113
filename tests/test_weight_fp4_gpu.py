"""``generate(weight_dtype="fp4")`` on the MI355X: the model is put on the format's grid first, so the option is
lossless and the float64 forward is the reference, under the logit rule of tests/test_weight_dtype_gpu.py."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import gemv

from ._model_oracle import forward64, spying
from .test_generate_gpu import _config
from .test_weight_dtype_gpu import _hip  # noqa: F401  (autouse: HIP backend, skip without a GPU)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name", ["tiny", "gqa"])
def test_cached_logits_against_float64_and_graph_equals_eager(name):
    cfg = _config(name)
    m = LlamaForCausalLM(cfg, DEV, torch.bfloat16).init_weights(7)
    for k in m.store.names:
        if "_proj.weight" in k or k == "lm_head.weight":
            w = m.store.master_view(k)
            w.copy_(gemv.dequantize_weight_fp4(*gemv.quantize_weight_fp4(w)))
    m.store.sync_shadow()
    B, T, n = 2, 16, 8
    ids = torch.randint(3, cfg.vocab_size, (B, T), generator=torch.Generator().manual_seed(11)).to(DEV)
    mask = torch.ones(B, T, dtype=torch.long, device=DEV)
    mask[1, :5] = 0
    kw = dict(max_new_tokens=n, eos_token_id=None, return_logits=True, weight_dtype="fp4")
    with spying() as spy:
        seq, cached = m.generate(ids, mask, hip_graph=False, **kw)
    assert spy.ran("nd_gemv_w4") == spy.calls["nd_gemv_w4"] == (n - 1) * (4 * cfg.num_hidden_layers + 1), dict(spy.calls)
    assert not spy.calls["nd_gemv_w8"]
    with spying() as spy:
        seq_g, cached_g = m.generate(ids, mask, hip_graph=True, **kw)
    spy.expect(ran=["nd_gemv_w4"], never=["nd_gemv_w8"], case=name)  # the warm-up steps and the capture launch it
    assert torch.equal(seq, seq_g) and torch.equal(cached.view(torch.int32), cached_g.view(torch.int32))
    assert m.wq is None
    full_mask = torch.cat([mask, torch.ones(B, n, dtype=torch.long, device=DEV)], dim=1)
    ref64 = forward64(m, seq.cpu(), ops.key_start(full_mask).cpu())
    for j in range(n):
        L = T + j
        with m._inference():
            full = m(seq[:, :L], attention_mask=full_mask[:, :L]).logits[:, -1]
        e_full = float((full.double().cpu() - ref64[:, L - 1]).abs().max())
        e_cached = float((cached[:, j].double().cpu() - ref64[:, L - 1]).abs().max())
        print(f"[{name}] step {j}: cached {e_cached:.3e}, full forward {e_full:.3e}, ratio {e_cached / e_full:.2f}")
        assert e_cached <= 2.0 * e_full, (j, e_cached, e_full)
