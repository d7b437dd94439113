"""``generate(weight_dtype="fp8")`` on the MI355X.  The models are put on the fp8 grid first (masters replaced by
dequant(quant(master))), so the option is lossless and the float64 forward of tests/_model_oracle.py is the reference
as it stands: the rule and the number are ``test_generate_gpu.test_cached_logits_against_float64``'s."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import gemv

from ._model_oracle import forward64, spying
from .test_generate_gpu import _config

pytestmark = pytest.mark.gpu
DEV, BF16 = "cuda", torch.bfloat16


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    yield
    ops.set_backend("auto")


def _grid_model(name):
    cfg = _config(name)
    m = LlamaForCausalLM(cfg, DEV, BF16).init_weights(7)
    for n in m.store.names:
        if "_proj.weight" in n or n == "lm_head.weight":
            w = m.store.master_view(n)
            w.copy_(gemv.dequantize_weight(*gemv.quantize_weight(w)))
    m.store.sync_shadow()
    return cfg, m


@pytest.mark.parametrize("name", ["tiny", "gqa"])
def test_cached_logits_against_float64(name):
    cfg, m = _grid_model(name)
    B, T, n = 2, 16, 8
    ids = torch.randint(3, cfg.vocab_size, (B, T), generator=torch.Generator().manual_seed(11)).to(DEV)
    mask = torch.ones(B, T, dtype=torch.long, device=DEV)
    mask[1, :5] = 0
    with spying() as spy:
        seq, cached = m.generate(ids, mask, max_new_tokens=n, eos_token_id=None, hip_graph=False, return_logits=True,
                                 weight_dtype="fp8")
    assert spy.ran("nd_gemv_w8") == spy.calls["nd_gemv_w8"] == (n - 1) * (4 * cfg.num_hidden_layers + 1), dict(spy.calls)
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


@pytest.mark.parametrize("name", ["tiny", "gqa"])
def test_graph_equals_eager_and_model_restored(name):
    cfg, m = _grid_model(name)
    m.store.master_view("lm_head.weight").mul_(1.37)  # off the grid again: the context has something to restore
    m.store.sync_shadow()
    before = m.store.shadow.clone(), m.store.master.clone()
    ids = torch.randint(3, cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(12)).to(DEV)
    mask = torch.ones(3, 9, dtype=torch.long, device=DEV)
    mask[0, :8], mask[2, :4] = 0, 0
    kw = dict(max_new_tokens=21, eos_token_id=None, return_logits=True, weight_dtype="fp8")
    a, la = m.generate(ids, mask, hip_graph=False, **kw)
    with spying() as spy:
        b, lb = m.generate(ids, mask, hip_graph=True, **kw)
    assert spy.ran("nd_gemv_w8") > 0  # the warm-up steps and the capture launch it; the replays carry it
    assert torch.equal(a, b) and torch.equal(la.view(torch.int32), lb.view(torch.int32))
    kw.update(kv_dtype="fp8", prefill_chunk=4)  # the 12-row extend takes the kernel too
    (c, lc), (d, ld) = m.generate(ids, mask, hip_graph=True, **kw), m.generate(ids, mask, hip_graph=False, **kw)
    assert torch.equal(c, d) and torch.equal(lc.view(torch.int32), ld.view(torch.int32))
    assert m.wq is None and torch.equal(m.store.shadow.view(torch.int16), before[0].view(torch.int16))
    assert torch.equal(m.store.master.view(torch.int32), before[1].view(torch.int32))
