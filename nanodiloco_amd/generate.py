"""Text generation from a saved checkpoint.

    python -m nanodiloco_amd.generate --checkpoint DIR (--prompt-ids "1,2,3" ... | --prompt-file F | --prompt "text" ...)
        [--llama-config-file F] [--max-new-tokens 32] [--temperature 0] [--top-k 0] [--top-p 1.0] [--seed 0]
        [--dtype auto] [--residual-dtype auto] [--device auto] [--hip-graph auto|on|off]
        [--tokenizer PATH]

Single process.  Only the model weights of a checkpoint written by ``utils.checkpoint.save_checkpoint`` are read
(``model.safetensors``), the config comes from ``--llama-config-file`` or the checkpoint's ``config.json`` -- as
``nanodiloco_amd.evaluate`` does (QK-norm, a sliding window and ``final_logit_softcapping`` come with it: the logits
every token is drawn from are the capped ones).  ``--prompt-ids`` may be given several times; ``--prompt-file`` holds one JSON list
of ids per line.  The prompts form one left-padded batch.  Output: one JSON line per prompt (``prompt_ids``,
``token_ids``: prompt + continuation, ``new_tokens``; with a tokenizer also ``text``), then one line with
``prefill_s``, ``decode_s`` and ``decode_tokens_per_s``.  ``--tokenizer PATH`` (optional) encodes ``--prompt`` and decodes
the result through ``AutoTokenizer.from_pretrained(PATH, local_files_only=True)``: nothing is ever fetched; without
it only ids are accepted.
"""
from __future__ import annotations

import argparse
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
              hip_graph={"auto": "auto", "on": True, "off": False}[a.hip_graph])
    amask = mask if len(prompts) > 1 else None

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    # the prompt pass alone (one new token), then the whole run: their difference is the decode time; one untimed
    # pass first, so that neither carries the first launches (code objects, GEMM algorithm selection)
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
    print(json.dumps(timing), flush=True)
    return recs + [timing]


if __name__ == "__main__":
    main()
