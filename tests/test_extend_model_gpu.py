"""Chunked prefill on the MI355X (tiny bf16 model, HIP path) under test_generate_gpu.py's rule between its cached and
uncached paths: against a high-precision reference the chunked run may err at most twice as much as the full forward
of the same prefix.  Reference: the fp32 PyTorch path on the CPU with the weights the GPU model computes with."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import resolve_llama_config
from nanodiloco_amd.models import LlamaForCausalLM

pytestmark = pytest.mark.gpu
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj", "lm_head")


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    yield
    ops.set_backend("auto")


@pytest.mark.parametrize("extra", [{}, dict(sliding_window=24, attn_logit_softcapping=20.0, qk_norm=True)],
                         ids=["plain", "window-softcap-qknorm"])
def test_chunked_prefill_logits(extra):
    cfg = resolve_llama_config("llama_tiny.json")
    cfg.vocab_size = 1024
    for k, v in extra.items():
        setattr(cfg, k, v)
    m = LlamaForCausalLM(cfg, "cuda", torch.bfloat16).init_weights(7)
    cpu = LlamaForCausalLM(cfg, "cpu", torch.float32)
    cpu.load_state_dict({n: (m.store.shadow_view(n) if any(k in n for k in PROJ) else m.store.master_view(n))
                         .detach().float().cpu() for n in m.store.names})
    B, T, n = 2, 40, 6  # pieces of 16, 16 and 8
    ids = torch.randint(3, cfg.vocab_size, (B, T), generator=torch.Generator().manual_seed(11)).cuda()
    mask = torch.ones(B, T, dtype=torch.long, device="cuda")
    mask[1, :21] = 0  # one left-padded row: its first real token sits inside the second piece
    seq, got = m.generate(ids, mask, max_new_tokens=n, eos_token_id=None, hip_graph=False, return_logits=True,
                          prefill_chunk=16)
    full_mask = torch.cat([mask, torch.ones(B, n, dtype=torch.long, device="cuda")], dim=1)
    cpu.eval(), m.eval()
    with torch.no_grad():
        ops.set_backend("auto")  # the reference runs on CPU tensors
        ref = cpu(seq.cpu(), attention_mask=full_mask.cpu()).logits.double()
        ops.set_backend("hip")
        for j in range(n):
            full = m(seq[:, :T + j], attention_mask=full_mask[:, :T + j]).logits[:, -1]
            e_full = float((full.double().cpu() - ref[:, T + j - 1]).abs().max())
            e_got = float((got[:, j].double().cpu() - ref[:, T + j - 1]).abs().max())
            print(f"step {j}: chunked error {e_got:.3e}, full-forward error {e_full:.3e}, ratio {e_got / e_full:.2f}")
            assert e_got <= 2.0 * e_full, (j, e_got, e_full)
