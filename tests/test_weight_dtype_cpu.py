"""``weight_dtype="fp8"`` on the CPU: an ordinary (off-grid) model under the option computes what a second model
computes whose projection weights were rounded by hand with the torch definition of the format."""
import json

import pytest
import torch

from nanodiloco_amd import generate as cli
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops.decode import kv8_dequantize, kv8_quantize
from nanodiloco_amd.utils.checkpoint import _save_st

CFG = dict(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
           vocab_size=101, rms_norm_eps=1e-5, max_position_embeddings=48)
KW = dict(max_new_tokens=8, eos_token_id=None, return_logits=True)
PROMPT = torch.randint(3, 101, (2, 7), generator=torch.Generator().manual_seed(1))


def _model(**over):
    return LlamaForCausalLM(LlamaConfig.from_dict({**CFG, **over})).init_weights(5)


def test_fp8_weights_equal_a_hand_rounded_model():
    m, hand = _model(), _model()
    for n in hand.store.names:
        if "_proj.weight" in n or n == "lm_head.weight":
            w = hand.store.master_view(n)
            w.copy_(kv8_dequantize(*kv8_quantize(w.view(w.shape[0], -1, 128))).view_as(w))
    before = m.store.master.clone()
    a, la = m.generate(PROMPT, weight_dtype="fp8", **KW)
    b, lb = hand.generate(PROMPT, **KW)
    assert torch.equal(a, b) and torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert m.wq is None and torch.equal(m.store.master.view(torch.int32), before.view(torch.int32))  # restored
    assert not torch.equal(m.generate(PROMPT, **KW)[1], la)  # and the unrounded model differs
    with m.quantized_weights("fp8"):  # held by the caller: generate joins it, every path sees the rounded weights
        assert torch.equal(m.generate(PROMPT, weight_dtype="fp8", **KW)[1].view(torch.int32), lb.view(torch.int32))
        assert torch.equal(m.generate(PROMPT, **KW)[1].view(torch.int32), lb.view(torch.int32))
        with pytest.raises(RuntimeError), m.quantized_weights("fp8"):
            pass
        assert m.wq is not None
    assert torch.equal(m.store.master.view(torch.int32), before.view(torch.int32))


def test_refusals():
    m = _model()
    for kw in (dict(weight_dtype="int4"), dict(weight_dtype="fp8", use_cache=False)):
        with pytest.raises(ValueError):
            m.generate(PROMPT, max_new_tokens=2, **kw)
    odd = _model(hidden_size=64, intermediate_size=96)  # K = 64 and 96: not multiples of 128
    with pytest.raises(ValueError, match="multiple of 128"):
        odd.generate(PROMPT, max_new_tokens=2, weight_dtype="fp8")
    assert odd.wq is None


def test_cli_echoes_weight_dtype(tmp_path):
    m = _model()
    (tmp_path / "config.json").write_text(json.dumps(m.config.to_dict()))
    (tmp_path / "trainer_state.json").write_text("{}")
    _save_st(str(tmp_path / "model.safetensors"), m.state_dict())
    args = ["--checkpoint", str(tmp_path), "--prompt-ids", "5,6,7", "--max-new-tokens", "4", "--device", "cpu"]
    plain, fp8 = cli.main(args), cli.main(args + ["--weight-dtype", "fp8"])
    assert "weight_dtype" not in plain[-1] and fp8[-1]["weight_dtype"] == "fp8"
    want = m.generate(torch.tensor([[5, 6, 7]]), max_new_tokens=4, weight_dtype="fp8")[0].tolist()
    got = fp8[0]["token_ids"]  # cut after an EOS, if one was drawn
    assert len(got) > 3 and got == want[:len(got)]
