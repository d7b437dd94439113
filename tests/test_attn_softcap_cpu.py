"""Attention logit soft-capping off the GPU: the PyTorch path against the dense float64 formula of
``tests/_attn_softcap.py`` under every mask mode, the config key, the CLI flag, and a checkpointed CPU run."""
import dataclasses
import json

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.main import parse_args
from nanodiloco_amd.ops import reference as ref

from . import _attn_softcap as ac
from .test_softcap_cpu import _log, _torchrun

B, T, NH, NKV, HD = 2, 40, 4, 2, 16
TINY = dict(hidden_size=64, intermediate_size=128, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=1,
            vocab_size=128)
RUN = ["--llama-config-file", "configs/llama_tiny.json", "--batch-size", "4", "--per-device-batch-size", "4",
       "--seq-length", "64", "--warmup-steps", "1", "--wandb", "off", "--device", "cpu", "--data", "synthetic",
       "--inner-steps", "2", "--total-steps", "2"]
KS = torch.tensor([5, 0], dtype=torch.int32)
IDS = torch.ones(B, T, dtype=torch.long)
IDS[0, 11] = IDS[1, 30] = 0
DOC = ops.doc_bounds(IDS, 0)
MASKS = {"none": ({}, {}), "kstart": (dict(kstart=KS), dict(kstart=KS)), "doc": (dict(doc_bounds=DOC), dict(doc_start=DOC[0])),
         "window": (dict(window=7), dict(window=7)), "window+kstart": (dict(window=7, kstart=KS), dict(window=7, kstart=KS))}
QKV = torch.randn(B * T, (NH + 2 * NKV) * HD, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 2.0


@pytest.mark.parametrize("kind", list(MASKS))
@pytest.mark.parametrize("cap", [1.0, 50.0])
def test_reference_against_the_dense_formula(kind, cap):
    kw, mk = MASKS[kind]
    one, zero = torch.ones(T, HD, dtype=torch.float64), torch.zeros(T, HD, dtype=torch.float64)
    x = QKV.clone().requires_grad_(True)
    o = ref.attention_block(x, one, zero, B, T, NH, NKV, HD, softcap=cap, **kw)
    dO = torch.randn(B * T, NH * HD, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    o.backward(dO)
    want = ac.attention(QKV, B, T, NH, NKV, HD, cap, ac.mask(B, T, "cpu", **mk), dO)
    # the block multiplies q k^T and P V in fp32: 2^-24 relative per product, summed over hd / T terms
    assert float((o.detach() - want["o"]).abs().max()) <= 1e-5
    assert float((x.grad - want["dqkv"]).abs().max()) <= 1e-4
    assert not bool(o[~want["seen"].reshape(-1)].any())  # a fully masked row gives 0, as the kernels do


@pytest.mark.parametrize("kind", list(MASKS))
def test_softcap_off_is_todays_output(kind):
    cos, sin = ref.rope_tables(T, HD, 10000.0)
    base = ref.attention_block(QKV.float(), cos, sin, B, T, NH, NKV, HD, **MASKS[kind][0])
    for off in (None, 0, 0.0):
        for fn in (ref.attention_block, ops.attention):
            assert torch.equal(fn(QKV.float(), cos, sin, B, T, NH, NKV, HD, softcap=off, **MASKS[kind][0]), base)


def test_config_key_and_cli_flag():
    from nanodiloco_amd.trainer import Trainer
    assert "attn_logit_softcapping" not in LlamaConfig.from_dict(TINY).to_dict()
    assert "attn_logit_softcapping" not in LlamaConfig.from_dict(dict(TINY, attn_logit_softcapping=0)).to_dict()
    c = LlamaConfig.from_dict(dict(TINY, attn_logit_softcapping=50.0))
    assert c.to_dict()["attn_logit_softcapping"] == 50.0
    assert LlamaConfig.from_dict(c.to_dict()).attn_logit_softcapping == 50.0
    for bad in (-1.0, float("nan"), float("inf"), "50", True):
        with pytest.raises(ValueError, match="attn_logit_softcapping"):
            LlamaConfig.from_dict(dict(TINY, attn_logit_softcapping=bad))
    assert parse_args([]).attn_softcap == 0.0 and parse_args(["--attn-softcap", "50"]).attn_softcap == 50.0
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            parse_args(["--attn-softcap", bad])
        with pytest.raises(ValueError, match="--attn-softcap"):
            Trainer(dataclasses.replace(parse_args(RUN), attn_softcap=float(bad)))
        with pytest.raises(ValueError, match="soft-cap"):
            ref.attention_block(QKV, None, None, B, T, NH, NKV, HD, softcap=float(bad))


def test_cpu_run_checkpoint_and_resume(tmp_path):
    """Two CPU trainer steps with --attn-softcap 1: the losses differ from the uncapped run's, config.json carries
    the key, and --resume with another value is refused."""
    a, la, lu = tmp_path / "a", tmp_path / "a.jsonl", tmp_path / "u.jsonl"
    _torchrun(1, RUN + ["--attn-softcap", "1", "--checkpoint-dir", str(a), "--log-file", str(la)])
    _torchrun(1, RUN + ["--log-file", str(lu)])
    capped = [x["loss"] for x in _log(la) if "loss" in x]
    plain = [x["loss"] for x in _log(lu) if "loss" in x]
    assert len(capped) == len(plain) == 2 and all(x == x for x in capped) and capped != plain
    with open(a / "config.json") as f:
        assert json.load(f)["attn_logit_softcapping"] == 1.0
    r = _torchrun(1, RUN + ["--attn-softcap", "2", "--resume", str(a), "--checkpoint-dir", str(a)], ok=False)
    assert "--attn-softcap 2 differs from the checkpoint's attn_logit_softcapping (1" in r.stdout + r.stderr
