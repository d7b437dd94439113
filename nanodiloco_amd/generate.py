"""Text generation from a saved checkpoint.

    python -m nanodiloco_amd.generate --checkpoint DIR (--prompt-ids "1,2,3" ... | --prompt-file F | --prompt "text" ...)
        [--llama-config-file F] [--max-new-tokens 32] [--temperature 0] [--top-k 0] [--top-p 1.0] [--seed 0]
        [--dtype auto] [--residual-dtype auto] [--device auto] [--hip-graph auto|on|off]
        [--tokenizer PATH] [--prefill-chunk 0] [--kv-dtype bf16|fp8] [--sampler torch|fused]
        [--weight-dtype bf16|fp8|fp4]

Single process.  Only the model weights of a checkpoint written by ``utils.checkpoint.save_checkpoint`` are read
(``model.safetensors``), the config comes from ``--llama-config-file`` or the checkpoint's ``config.json`` -- as
``nanodiloco_amd.evaluate`` does (QK-norm, a sliding window and ``final_logit_softcapping`` come with it: the logits
every token is drawn from are the capped ones).  ``--prompt-ids`` may be given several times; ``--prompt-file`` holds one JSON list
of ids per line.  The prompts form one left-padded batch.  Output: one JSON line per prompt (``prompt_ids``,
``token_ids``: prompt + continuation, ``new_tokens``; with a tokenizer also ``text``), then one line with
``prefill_s``, ``decode_s`` and ``decode_tokens_per_s``.  ``--tokenizer PATH`` (optional) encodes ``--prompt`` and decodes
the result through ``AutoTokenizer.from_pretrained(PATH, local_files_only=True)``: nothing is ever fetched; without
it only ids are accepted.  ``--prefill-chunk N`` (N > 0) prefills the prompt in pieces of N tokens through the
multi-token KV-cache attention (``model.extend``) instead of one whole-prompt forward.  ``--kv-dtype fp8`` keeps the KV
cache as e4m3 codes plus one exponent per row (about half the bytes of bf16; docs/DESIGN.md "fp8 KV cache"); the
timing line then echoes the value as ``kv_dtype``.  ``--sampler fused`` (with ``--temperature`` > 0) draws every token
with the one-launch HIP sampler (``ops.sample``; docs/DESIGN.md "Fused sampler") instead of ``filter_logits`` +
``torch.multinomial``; the timing line then echoes ``sampler``.  The two draw different tokens from one seed.  ``--weight-dtype fp8`` runs the decoder's projections and the
lm head on e4m3 codes plus one exponent per 128 input features (``model.quantized_weights``; docs/DESIGN.md "fp8
weight-only decode"): the decode step streams the codes through ``ops.gemv_w8``, every other path computes with the
same rounded weights; the timing line then echoes ``weight_dtype``.  ``--weight-dtype fp4`` does the same with e2m1
codes, two to a byte, plus one exponent per 32 input features (``ops.gemv_w4``; docs/DESIGN.md "fp4 weight-only
decode"): about a quarter of the bf16 bytes and a much coarser rounding (relative weight error about 0.12 against
0.027 for fp8).
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time
from typing import Any, Dict, List, Optional

import torch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="nanodiloco_amd.generate", description="generate from a checkpoint")
    p.add_argument("--checkpoint", required=True, help="a directory written by save_checkpoint (--checkpoint-dir)")
    p.add_argument("--llama-config-file", default=None, help="default: the checkpoint's config.json")
    p.add_argument("--prompt-ids", action="append", default=[], help='comma-separated token ids, e.g. "1,2,3"')
    p.add_argument("--prompt-file", default=None, help="one JSON list of token ids per line")
    p.add_argument("--prompt", action="append", default=[], help="text (needs --tokenizer)")
    p.add_argument("--tokenizer", default=None, help="a local tokenizer directory (never downloaded)")
    p.add_argument("--max-new-tokens", type=int, default=32)
    p.add_argument("--temperature", type=float, default=0.0)
    p.add_argument("--top-k", type=int, default=0)
    p.add_argument("--top-p", type=float, default=1.0)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--dtype", default="auto", help="auto | fp32 | bf16")
    p.add_argument("--residual-dtype", default="auto", help="auto | fp32 | bf16")
    p.add_argument("--device", default="auto", help="auto | cpu | cuda")
    p.add_argument("--hip-graph", default="auto", choices=["auto", "on", "off"])
    p.add_argument("--prefill-chunk", type=int, default=0,
                   help="prefill the prompt in pieces of N tokens through model.extend (0: one whole-prompt forward)")
    p.add_argument("--kv-dtype", default="bf16", choices=["bf16", "fp8"],
                   help="KV cache storage: bf16, or fp8 (e4m3 codes + one exponent per row)")
    p.add_argument("--sampler", default="torch", choices=["torch", "fused"],
                   help="with --temperature > 0: torch (filter_logits + multinomial) or fused (ops.sample, one launch)")
    p.add_argument("--weight-dtype", default="bf16", choices=["bf16", "fp8", "fp4"],
                   help="projection weights: bf16, fp8 weight-only (e4m3 codes + one exponent per 128 inputs) or fp4 "
                        "weight-only (e2m1 codes + one exponent per 32 inputs; lossy)")
    return p


def _prompts(a, tok) -> List[List[int]]:
    out = []
    for s in a.prompt_ids:
        out.append([int(x) for x in s.replace(" ", "").split(",") if x != ""])
    if a.prompt_file:
        with open(a.prompt_file) as f:
            for line in f:
                if line.strip():
                    out.append([int(x) for x in json.loads(line)])
    if a.prompt:
        if tok is None:
            raise ValueError("--prompt needs --tokenizer PATH; without a tokenizer only token ids are accepted")
        out.extend(list(tok(s)["input_ids"]) for s in a.prompt)
    if not out or any(len(p) == 0 for p in out):
        raise ValueError("give at least one non-empty prompt (--prompt-ids, --prompt-file or --prompt)")
    return out


def main(argv: Optional[List[str]] = None) -> List[Dict[str, Any]]:
    from .config import LlamaConfig, resolve_llama_config
    from .models import LlamaForCausalLM
    from .trainer import _dtype, _residual_dtype
    from .utils.checkpoint import _load_st, find_checkpoint

    a = build_parser().parse_args(argv if argv is not None else sys.argv[1:])
    ckpt = find_checkpoint(a.checkpoint)
    if ckpt is None:
        raise FileNotFoundError(f"no complete checkpoint at {a.checkpoint}")
    tok = None
    if a.tokenizer:
        from transformers import AutoTokenizer
        tok = AutoTokenizer.from_pretrained(a.tokenizer, local_files_only=True)
    prompts = _prompts(a, tok)
    dev = a.device if a.device != "auto" else ("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device("cuda", torch.cuda.current_device()) if dev == "cuda" else torch.device(dev)
    cfg = resolve_llama_config(a.llama_config_file) if a.llama_config_file \
        else LlamaConfig.from_json(os.path.join(ckpt, "config.json"))
    bad = [t for p in prompts for t in p if not 0 <= t < cfg.vocab_size]
    if bad:
        raise ValueError(f"token id {bad[0]} outside the vocabulary of {cfg.vocab_size}")
    model = LlamaForCausalLM(cfg, device, _dtype(a.dtype, device), residual_dtype=_residual_dtype(a.residual_dtype))
    model.load_state_dict(_load_st(os.path.join(ckpt, "model.safetensors")))
    model.eval()
    T = max(len(p) for p in prompts)
    pad = cfg.pad_token_id if cfg.pad_token_id is not None else (cfg.eos_token_id or 0)
    ids = torch.full((len(prompts), T), pad, dtype=torch.long)
    mask = torch.zeros(len(prompts), T, dtype=torch.long)
    for i, p in enumerate(prompts):  # left padding
        ids[i, T - len(p):] = torch.tensor(p)
        mask[i, T - len(p):] = 1
    ids, mask = ids.to(device), mask.to(device)
    kw = dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, seed=a.seed,
              hip_graph={"auto": "auto", "on": True, "off": False}[a.hip_graph], prefill_chunk=a.prefill_chunk,
              kv_dtype=a.kv_dtype, sampler=a.sampler, weight_dtype=a.weight_dtype)
    amask = mask if len(prompts) > 1 else None

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    # the prompt pass alone (one new token), then the whole run: their difference is the decode time; one untimed
    # pass first, so that neither carries the first launches (code objects, GEMM algorithm selection)
    # the weights are quantised once, around all three calls: prefill_s does not carry it
    with model.quantized_weights(a.weight_dtype) if a.weight_dtype != "bf16" else contextlib.nullcontext():
        model.generate(ids, amask, max_new_tokens=1, **kw)
        sync()
        t0 = time.perf_counter()
        model.generate(ids, amask, max_new_tokens=1, **kw)
        sync()
        prefill_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        out = model.generate(ids, amask, max_new_tokens=a.max_new_tokens, **kw)
        sync()
        total_s = time.perf_counter() - t0
    new = out[:, T:].tolist()
    recs = []
    for p, cont in zip(prompts, new):
        eos = cfg.eos_token_id
        if eos is not None and eos in cont:
            cont = cont[:cont.index(eos) + 1]  # what follows a row's EOS is padding
        rec = {"prompt_ids": p, "token_ids": p + cont, "new_tokens": len(cont)}
        if tok is not None:
            rec["text"] = tok.decode(p + cont)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    steps = max(out.shape[1] - T - 1, 0)
    decode_s = max(total_s - prefill_s, 0.0)
    timing = {"prefill_s": prefill_s, "decode_s": decode_s,
              "decode_tokens_per_s": (steps * len(prompts) / decode_s) if decode_s > 0 and steps else 0.0}
    if a.kv_dtype != "bf16":  # the default run's line is unchanged
        timing["kv_dtype"] = a.kv_dtype
    if a.weight_dtype != "bf16":
        timing["weight_dtype"] = a.weight_dtype
    if a.sampler != "torch":
        timing["sampler"] = a.sampler
    print(json.dumps(timing), flush=True)
    return recs + [timing]


if __name__ == "__main__":
    main()
