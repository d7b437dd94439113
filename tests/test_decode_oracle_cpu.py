"""The float64 decode oracle (``_decode_oracle``) on the CPU against the project's two PyTorch paths: the twin of
``ops.attention_decode`` on a cache, and the last row of ``reference.attention_block`` on the packed window the cache
was cut from.  fp32 throughout (``round_dtype=None``: nothing is stored as bf16 here); the three agree to fp32
rounding of sums of T <= 70 terms, checked with the project's rule: margin 8 on the fp32 twin's own distance."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.ops import reference as ref

from . import _oracle64 as o64
from ._decode_oracle import decode_refs


def _cfg(nh, nkv, hd):
    return LlamaConfig.from_dict(dict(hidden_size=nh * hd, num_attention_heads=nh, num_key_value_heads=nkv,
                                      head_dim=hd, num_hidden_layers=1, intermediate_size=64, vocab_size=64,
                                      max_position_embeddings=128))


@pytest.mark.parametrize("nh,nkv,hd", [(4, 4, 32), (4, 2, 64), (8, 1, 32)])
@pytest.mark.parametrize("T,ks", [(1, (0, 0)), (9, (0, 3)), (70, (5, 69))])
def test_oracle_matches_twin_and_training_reference(nh, nkv, hd, T, ks):
    torch.manual_seed(T + nh + hd)
    B = 2
    W = (nh + 2 * nkv) * hd
    qkv = o64.spiked(B * T, W, "cpu")
    cos, sin = ref.rope_tables(80, hd, 10000.0)
    kstart = torch.tensor(ks, dtype=torch.int32)
    # the training-path reference on the whole window; its last row is the decode step
    full = ref.attention_block(qkv, cos, sin, B, T, nh, nkv, hd, kstart=kstart).view(B, T, nh * hd)[:, -1]
    cache = ops.KVCache(_cfg(nh, nkv, hd), B, 80, "cpu", torch.float32)
    if T > 1:
        first = qkv.view(B, T, W)[:, :T - 1].reshape(B * (T - 1), W)
        ops.cache_fill(cache, 0, first, B, T - 1, cos, sin, rotated=False)
    cache.set_positions([T - 1] * B, ks)
    last = qkv.view(B, T, W)[:, -1].contiguous()
    want, twin = decode_refs(last, cache.k[0], cache.v[0], [T - 1] * B, list(ks), nh, nkv, hd, cos, sin,
                             round_dtype=None)
    keep = last.clone()
    got = ops.attention_decode(last, cache, 0, cos, sin)
    assert torch.equal(last, keep)
    o64.check(got, want, twin, name="twin")
    o64.check(full, want, twin, name="attention_block")
    # the twin appended exactly slot T-1: k rotated at T-1, v as given
    q, k, v = ref.split_qkv(qkv, B, T, nh, nkv, hd)
    torch.testing.assert_close(cache.k[0][:, :, T - 1], ref.apply_rope(k, cos[:T], sin[:T])[:, :, -1], rtol=0, atol=1e-6)
    assert torch.equal(cache.v[0][:, :, T - 1], v[:, :, -1])
    assert not bool(cache.k[0][:, :, T:].any()) and not bool(cache.v[0][:, :, T:].any())
    assert int(cache.pos[0]) == T - 1  # attention_decode does not advance


def test_no_key_gives_zero():
    nh, nkv, hd = 2, 2, 32
    cos, sin = ref.rope_tables(8, hd, 10000.0)
    row = torch.randn(1, (nh + 2 * nkv) * hd)
    kc = torch.zeros(1, nkv, 8, hd)
    want, twin = decode_refs(row, kc, kc.clone(), [2], [5], nh, nkv, hd, cos, sin, round_dtype=None)
    assert not bool(want.any()) and not bool(twin.any())
