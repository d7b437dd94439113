"""Multi-token KV-cache attention on the CPU (fp32, the PyTorch path): the twin against ``reference.attention_block``
on the whole sequence, ``model.extend`` in pieces against ``model.forward``, chunked prefill against the recompute
path, the CLI flag.  Tolerance: the same fp32 function with sums in another order -- 1e-5 on values of order 1."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.generate import build_parser
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import reference as ref

CFG = dict(hidden_size=64, intermediate_size=96, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
           vocab_size=101, rms_norm_eps=1e-5, max_position_embeddings=48)
TOL = 1e-5


@pytest.mark.parametrize("window,cap", [(None, None), (5, None), (None, 3.0), (7, 3.0)])
def test_twin_equals_the_whole_sequence_attention(window, cap):
    B, T, nh, nkv, hd = 2, 24, 6, 2, 16
    torch.manual_seed(1)
    qkv = torch.randn(B * T, (nh + 2 * nkv) * hd)
    cos, sin = ops.rope_cache(32, hd, 10000.0, None, "cpu")
    kstart = torch.tensor([0, 12], dtype=torch.int32)  # sequence 1: pad queries inside the second piece
    want = ref.attention_block(qkv, cos, sin, B, T, nh, nkv, hd, kstart=kstart, window=window, softcap=cap)
    kc, vc = torch.zeros(B, nkv, 32, hd), torch.zeros(B, nkv, 32, hd)
    pos, got = torch.zeros(B, dtype=torch.int32), []
    for t0, n in ((0, 1), (1, 10), (11, 13)):
        rows = qkv.view(B, T, -1)[:, t0:t0 + n].reshape(B * n, -1)
        got.append(ops.attention_extend_torch(rows, cos, sin, pos, kstart, kc, vc, n, nh, nkv, hd, window=window,
                                              softcap=cap).view(B, n, -1))
        pos += n
    got, want = torch.cat(got, 1), want.view(B, T, -1)
    assert bool((got[1, :12] == 0).all())  # pad queries: zeros
    assert float((got[0] - want[0]).abs().max()) < TOL and float((got[1, 12:] - want[1, 12:]).abs().max()) < TOL


@pytest.fixture(scope="module")
def model():
    return LlamaForCausalLM(LlamaConfig.from_dict(CFG)).init_weights(5)


def test_model_extend_in_pieces_equals_forward(model):
    ids = torch.randint(3, CFG["vocab_size"], (2, 19), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = model(ids).logits
    cache = model.new_cache(2, 19)
    got = torch.cat([model.extend(ids[:, :7], cache), model.extend(ids[:, 7:8], cache), model.extend(ids[:, 8:], cache)], 1)
    assert cache.max_pos == 19 and cache.pos.tolist() == [19, 19]
    assert float((got - want).abs().max()) < 10 * TOL
    with pytest.raises(ValueError, match="full"):
        model.extend(ids[:, :1], cache)


def test_chunked_prefill_generates_what_recompute_does(model):
    ids = torch.randint(3, CFG["vocab_size"], (2, 11), generator=torch.Generator().manual_seed(4))
    mask = torch.ones(2, 11, dtype=torch.long)
    mask[1, :4] = 0
    a, la = model.generate(ids, mask, max_new_tokens=6, eos_token_id=None, return_logits=True, prefill_chunk=4)
    b, lb = model.generate(ids, mask, max_new_tokens=6, eos_token_id=None, return_logits=True, use_cache=False)
    assert torch.equal(a, b) and float((la - lb).abs().max()) < 10 * TOL


def test_cli_flag_parses():
    assert build_parser().parse_args(["--checkpoint", "x", "--prefill-chunk", "64"]).prefill_chunk == 64
    assert build_parser().parse_args(["--checkpoint", "x"]).prefill_chunk == 0
