"""The fp4 weight format (``ops.gemv.quantize_weight_fp4``) and ``weight_dtype="fp4"`` on the CPU."""
import json

import pytest
import torch

from nanodiloco_amd.ops.gemv import dequantize_weight_fp4, quantize_weight_fp4

from .test_weight_dtype_cpu import KW, PROMPT, _model, _save_st, cli


def test_quantiser():
    w = torch.randn(6, 256, generator=torch.Generator().manual_seed(2)) * 0.02
    w[:3, :32] = 0  # (0, 0): a zero group; (1, 0): amax 6, e = 0, ties; (2, 0): e clamped at 100, saturation
    w[1, :8] = torch.tensor([6.0, 2.5, 5.0, -3.5, 0.25, 0.75, -1.25, 2.6])
    w[2, :3] = torch.tensor([2.0 ** 110, -(2.0 ** 105), 2.0 ** 100])
    codes, exps = quantize_weight_fp4(w)
    d = dequantize_weight_fp4(codes, exps)
    # idempotent in value (a group whose amax rounds down to 3 takes the next exponent down and twice the codes)
    assert torch.equal(dequantize_weight_fp4(*quantize_weight_fp4(d)).view(torch.int32), d.view(torch.int32))
    assert torch.equal(d.bfloat16().float(), d)  # exact in bf16
    scaled = torch.ldexp(w.view(6, 8, 32), -exps.int()[..., None]).abs().amax(-1)[3:]  # the plain rows
    assert bool(((scaled > 3) & (scaled <= 6)).all())
    assert int(exps[0, 0]) == 0 and not bool(codes[0, :16].any())
    assert int(exps[1, 0]) == 0 and d[1, :8].tolist() == [6.0, 2.0, 4.0, -4.0, 0.0, 1.0, -1.0, 3.0]
    assert int(exps[2, 0]) == 100 and d[2, :3].tolist() == [6.0 * 2.0 ** 100, -6.0 * 2.0 ** 100, 2.0 ** 100]
    assert codes[1, :4].tolist() == [0x47, 0xe6, 0x20, 0x5a]  # element k: low nibble of byte k / 2 for even k
    for bad in (float("nan"), float("inf")):
        w[3, 5] = bad
        with pytest.raises(ValueError):
            quantize_weight_fp4(w)


def test_fp4_weights_equal_a_hand_rounded_model():
    m, hand = _model(), _model()
    for n in hand.store.names:
        if "_proj.weight" in n or n == "lm_head.weight":
            w = hand.store.master_view(n)
            w.copy_(dequantize_weight_fp4(*quantize_weight_fp4(w)))
    before = m.store.master.clone()
    a, la = m.generate(PROMPT, weight_dtype="fp4", **KW)
    b, lb = hand.generate(PROMPT, **KW)
    assert torch.equal(a, b) and torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert m.wq is None and m.wq_dtype is None
    assert torch.equal(m.store.master.view(torch.int32), before.view(torch.int32))  # restored


def test_refusals():
    m = _model()
    for kw in (dict(weight_dtype="int4"), dict(weight_dtype="fp4", use_cache=False)):
        with pytest.raises(ValueError):
            m.generate(PROMPT, max_new_tokens=2, **kw)
    with m.quantized_weights("fp4"):
        with pytest.raises(ValueError, match="inside"):
            m.generate(PROMPT, max_new_tokens=2, weight_dtype="fp8")
        with pytest.raises(RuntimeError), m.quantized_weights("fp8"):
            pass
        m.generate(PROMPT, max_new_tokens=2, weight_dtype="fp4")  # joins the held context
    odd = _model(hidden_size=64, intermediate_size=96)  # K = 64 and 96: not multiples of 128
    with pytest.raises(ValueError, match="multiple of 128"):
        odd.generate(PROMPT, max_new_tokens=2, weight_dtype="fp4")


def test_cli_echoes_weight_dtype(tmp_path):
    m = _model()
    (tmp_path / "config.json").write_text(json.dumps(m.config.to_dict()))
    (tmp_path / "trainer_state.json").write_text("{}")
    _save_st(str(tmp_path / "model.safetensors"), m.state_dict())
    args = ["--checkpoint", str(tmp_path), "--prompt-ids", "5,6,7", "--max-new-tokens", "4", "--device", "cpu"]
    assert cli.main(args + ["--weight-dtype", "fp4"])[-1]["weight_dtype"] == "fp4"
