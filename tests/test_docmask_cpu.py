"""Document-masked attention for packed windows (``--doc-mask``), CPU side: the bounds derived from the EOS
positions, their validator, the torch reference path, the model flag, the CLI flag and a 2-worker gloo run on a
memmap shard that holds EOS tokens."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import reference as ref

from ._mp import child_env, free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 2


def loop_bounds(row, eos):
    """The definition, one token at a time: a document starts at 0 or right after an EOS."""
    T = len(row)
    start, end = [0] * T, [T] * T
    s = 0
    for t in range(T):
        if t > 0 and row[t - 1] == eos:
            s = t
        start[t] = s
    e = T
    for t in range(T - 1, -1, -1):
        if row[t] == eos:
            e = t + 1
        end[t] = e
    return start, end


ROWS = {
    "no_eos": [5, 6, 7, 8, 9, 10, 11, 12],
    "eos_at_0": [EOS, 6, 7, 8, 9, 10, 11, 12],
    "eos_at_last": [5, 6, 7, 8, 9, 10, 11, EOS],
    "consecutive_eos": [5, 6, EOS, EOS, EOS, 10, 11, 12],
    "mixed": [5, EOS, 7, 8, EOS, 10, EOS, 12],
}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_doc_bounds_matches_loop(name):
    row = ROWS[name]
    ds, de = ops.doc_bounds(torch.tensor([row]), EOS)
    assert ds.dtype == torch.int32 and de.dtype == torch.int32 and ds.shape == (1, len(row))
    s, e = loop_bounds(row, EOS)
    assert ds[0].tolist() == s and de[0].tolist() == e
    ops.check_doc_bounds(ds, de)


def test_doc_bounds_rows_are_independent():
    names = sorted(ROWS)
    ds, de = ops.doc_bounds(torch.tensor([ROWS[n] for n in names]), EOS)
    for i, n in enumerate(names):
        s, e = loop_bounds(ROWS[n], EOS)
        assert ds[i].tolist() == s and de[i].tolist() == e, n
    ops.check_doc_bounds(ds, de)
    # one-token documents: an EOS right after an EOS is a document of its own
    i = names.index("consecutive_eos")
    assert ds[i].tolist() == [0, 0, 0, 3, 4, 5, 5, 5] and de[i].tolist() == [3, 3, 3, 4, 5, 8, 8, 8]


def test_check_doc_bounds_rejects_broken_invariants():
    ds, de = ops.doc_bounds(torch.tensor([ROWS["mixed"]]), EOS)
    bad = ds.clone()
    bad[0, 5] = 1  # falls back below its predecessor: not monotone
    with pytest.raises(ValueError):
        ops.check_doc_bounds(bad, de)
    bad = ds.clone()
    bad[0, 3] = 4  # doc_start[t] > t
    with pytest.raises(ValueError):
        ops.check_doc_bounds(bad, de)
    bad = de.clone()
    bad[0, 3] = 3  # doc_end[t] <= t
    with pytest.raises(ValueError):
        ops.check_doc_bounds(ds, bad)
    with pytest.raises(ValueError):
        ops.check_doc_bounds(ds.long(), de.long())  # the kernels read int32


def test_reference_attention_equals_per_document_causal():
    """attention_block(..., doc_bounds) in fp32 == plain causal attention on each document's own slice, with the
    RoPE tables taken at the slice's positions (positions are not reset at document starts)."""
    torch.manual_seed(0)
    B, T, nh, nkv, hd = 2, 24, 4, 2, 16
    ids = torch.randint(3, 50, (B, T))
    ids[0, [4, 5, 13]] = EOS
    ids[1, [0, 22]] = EOS
    ds, de = ops.doc_bounds(ids, EOS)
    qkv = torch.randn(B * T, (nh + 2 * nkv) * hd)
    cos, sin = ref.rope_tables(T, hd, 10000.0)
    out = ref.attention_block(qkv, cos, sin, B, T, nh, nkv, hd, doc_bounds=(ds, de)).view(B, T, nh * hd)
    x = qkv.view(B, T, -1)
    for b in range(B):
        t = 0
        while t < T:
            e = int(de[b, t])
            n = e - t
            q, k, v = ref.split_qkv(x[b, t:e].reshape(n, -1), 1, n, nh, nkv, hd)
            q, k = ref.apply_rope(q, cos[t:e], sin[t:e]), ref.apply_rope(k, cos[t:e], sin[t:e])
            o = ref.causal_attention(q, k, v).transpose(1, 2).reshape(n, nh * hd)
            assert torch.allclose(out[b, t:e], o, atol=1e-5, rtol=1e-5), (b, t, e)
            t = e
    with pytest.raises(ValueError):
        ops.attention(qkv, cos, sin, B, T, nh, nkv, hd, kstart=torch.zeros(B, dtype=torch.int32), doc_bounds=(ds, de))


def _tiny(doc_mask):
    cfg = LlamaConfig.from_dict(dict(hidden_size=64, intermediate_size=128, num_attention_heads=4,
                                     num_key_value_heads=2, num_hidden_layers=2, vocab_size=97, eos_token_id=EOS))
    return LlamaForCausalLM(cfg, "cpu", torch.float32, doc_mask=doc_mask).init_weights(0).eval()


def test_model_doc_mask_isolates_documents():
    """With doc_mask, the logits of document B do not depend on the tokens of the earlier document A; without it
    they do."""
    torch.manual_seed(1)
    T = 32
    ids = torch.randint(3, 97, (2, T))
    ids[:, 11] = EOS  # document A = [0, 12), document B = [12, T)
    other = ids.clone()
    other[:, 2:9] = torch.randint(3, 97, (2, 7))
    assert not torch.equal(ids, other)
    with torch.no_grad():
        m = _tiny(True)
        a, b = m(ids).logits, m(other).logits
        assert torch.allclose(a[:, 12:], b[:, 12:], atol=1e-6, rtol=0)
        assert not torch.allclose(a[:, 2:12], b[:, 2:12], atol=1e-6, rtol=0)
        m = _tiny(False)
        a, b = m(ids).logits, m(other).logits
        assert not torch.allclose(a[:, 12:], b[:, 12:], atol=1e-6, rtol=0)


def test_model_doc_mask_rejects_attention_mask():
    ids = torch.randint(3, 97, (1, 16))
    with pytest.raises(ValueError):
        _tiny(True)(ids, attention_mask=torch.ones_like(ids))


def test_cli_flag():
    from nanodiloco_amd.main import parse_args
    from nanodiloco_amd.trainer import check_doc_mask

    assert parse_args([]).doc_mask is False
    assert parse_args(["--doc-mask"]).doc_mask is True
    assert parse_args(["--doc-mask", "--data", "memmap"]).doc_mask is True
    with pytest.raises(SystemExit):
        parse_args(["--doc-mask", "--data", "hf"])
    # --data auto that resolves to hf, and the GPU's tile constraint, are caught when the trainer starts
    with pytest.raises(ValueError, match="hf"):
        check_doc_mask(True, "hf", 1024, on_gpu=False)
    with pytest.raises(ValueError, match="64"):
        check_doc_mask(True, "memmap", 96, on_gpu=True)
    check_doc_mask(True, "memmap", 96, on_gpu=False)
    check_doc_mask(True, "synthetic", 1024, on_gpu=True)
    check_doc_mask(False, "hf", 96, on_gpu=True)


def _first_loss(tmp_path, shard_dir, tag, extra):
    log = tmp_path / f"{tag}.jsonl"
    env = child_env(OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), "-m", "nanodiloco_amd",
           "--llama-config-file", "configs/llama_tiny.json", "--batch-size", "4", "--per-device-batch-size", "4",
           "--seq-length", "64", "--warmup-steps", "1", "--wandb", "off", "--device", "cpu", "--debug-checks",
           "--data", "memmap", "--dataset-path", str(shard_dir), "--total-steps", "2", "--inner-steps", "2",
           "--log-file", str(log)] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [json.loads(l) for l in open(log)]
    assert [x["step"] for x in rows] == [1, 2]
    return rows


@pytest.mark.slow
def test_two_worker_gloo_run_on_packed_shard(tmp_path):
    from nanodiloco_amd.data.memmap import write_token_shard

    rng = np.random.default_rng(0)
    toks = rng.integers(3, 30000, size=64 * 64)
    toks[rng.random(toks.shape) < 0.04] = EOS  # documents of ~25 tokens: several per 64-token window
    shard = tmp_path / "shards"
    shard.mkdir()
    write_token_shard(str(shard / "a.bin"), toks)
    plain = _first_loss(tmp_path, shard, "plain", [])
    doc = _first_loss(tmp_path, shard, "doc", ["--doc-mask"])
    assert all(np.isfinite(x["loss"]) for x in doc)
    assert doc[0]["loss"] != plain[0]["loss"]
