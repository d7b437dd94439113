"""The fp8 KV cache on the CPU: the format's PyTorch definition against a float64 search over the codes, the fp8
``KVCache`` through the PyTorch twins, the CLI flag."""
import pytest
import torch

from nanodiloco_amd import generate
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import decode

from . import _oracle64 as o64
from ._kv8 import edge_rows, quantize64

CFG = dict(hidden_size=64, intermediate_size=96, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
           vocab_size=101, rms_norm_eps=1e-5, max_position_embeddings=48)
TOL = 1e-4  # test_extend_cpu.py's bound for logits of the same fp32 function with sums in another order


@pytest.mark.parametrize("hd", [32, 64, 128])
def test_quantiser_is_the_nearest_code_search(hd):
    torch.manual_seed(hd)
    rows = torch.cat([edge_rows(hd), o64.spiked(40, hd, "cpu").bfloat16(), o64.spiked(8, hd, "cpu", scale=1e-3).bfloat16()])
    codes, exps = decode.kv8_quantize(rows)
    want_c, want_e = quantize64(rows)
    assert codes.dtype == torch.uint8 and exps.dtype == torch.int8
    assert torch.equal(exps, want_e), (exps.tolist(), want_e.tolist())
    assert torch.equal(codes, want_c)
    assert exps[:7].tolist() == [0, -5, -4, 0, -100, -100, 0]  # the rule's two sides; the lower clamp
    assert codes[3, :4].tolist() == [0x7E, 0x58, 0x5A, 0xDA] and codes[5, 3] == 0x80  # ties to even, -0 keeps its sign
    back = decode.kv8_dequantize(codes, exps)
    assert torch.equal(back, o64.fp8_codes(0)[codes.long()].float() * torch.exp2(exps.float())[:, None])
    assert torch.equal(back.bfloat16().float(), back), "code * 2^e must be exact in bf16"
    amax = rows.float().abs().amax(-1, keepdim=True)
    assert bool(((back - rows.float()).abs() <= amax / 14 + 2.0 ** -110).all())  # half a code step (16) over the least scaled amax (224)


def test_fp8_cache_decode_step_equals_extend():
    m = LlamaForCausalLM(LlamaConfig.from_dict(CFG)).init_weights(5)
    ids = torch.randint(3, CFG["vocab_size"], (2, 14), generator=torch.Generator().manual_seed(3))
    mask = torch.ones(2, 14, dtype=torch.long)
    mask[1, :4] = 0
    a, b = m.new_cache(2, 14, kv_dtype="fp8"), m.new_cache(2, 14, kv_dtype="fp8")
    m.prefill(ids[:, :13], mask[:, :13], a)
    m.prefill(ids[:, :13], mask[:, :13], b)
    assert a.k[0].dtype == torch.uint8 and a.k_exp[0].dtype == torch.int8 and bool(a.k[0][0, :, :13].any())
    one, ext = m.decode_step(ids[:, 13], a), m.extend(ids[:, 13:], b, last_only=True)
    assert float((one - ext).abs().max()) < TOL
    for x, y in zip(a.k + a.v + a.k_exp + a.v_exp, b.k + b.v + b.k_exp + b.v_exp):
        assert torch.equal(x, y), "both paths store the same codes and exponents"
    cap = LlamaConfig.from_dict(dict(CFG, attn_logit_softcapping=5.0))
    with pytest.raises(ValueError, match="softcapping"):
        decode.KVCache(cap, 2, 14, "cpu", torch.float32, kv_dtype="fp8")


def test_cli_runs_with_an_fp8_cache(tmp_path):
    from nanodiloco_amd.trainer import TrainArgs, Trainer
    ck = tmp_path / "ck"
    Trainer(TrainArgs(llama_config_file="configs/llama_tiny.json", batch_size=4, per_device_batch_size=4, seq_length=32,
                      warmup_steps=1, total_steps=1, inner_steps=1, wandb="off", device="cpu", data="synthetic",
                      log_every=1, checkpoint_dir=str(ck), seed=3)).train()
    argv = ["--checkpoint", str(ck), "--prompt-ids", "1,2,3", "--prompt-ids", "5,6,7,8", "--max-new-tokens", "5",
            "--device", "cpu"]
    fp8 = generate.main(argv + ["--kv-dtype", "fp8"])
    assert fp8[-1]["kv_dtype"] == "fp8" and 1 <= fp8[0]["new_tokens"] <= 5 and fp8[1]["prompt_ids"] == [5, 6, 7, 8]
    assert "kv_dtype" not in generate.main(argv)[-1]  # the default line is the one it was
