"""Held-out evaluation: the code ``Trainer.evaluate`` runs, and a stand-alone entry for a saved checkpoint.

    python -m nanodiloco_amd.evaluate --checkpoint DIR [--llama-config-file F] --data synthetic|memmap
        [--eval-dataset-path P] [--eval-batches 8] [--per-device-batch-size 8] [--seq-length 1024] [--seed 1337]
        [--dtype auto] [--residual-dtype auto] [--doc-mask] [--device auto]

Single process.  Only the model weights of a checkpoint written by ``utils.checkpoint.save_checkpoint`` are read
(``model.safetensors``, the HF-loadable fp32 master weights) -- no optimizer, no DiLoCo state -- and the model config
comes from ``--llama-config-file`` or the checkpoint's ``config.json`` (with ``final_logit_softcapping`` in it the
loss is that of the soft-capped logits, as in training).  With the data settings of the training run
(rank 0 of world 1) it prints, as one JSON line, the ``eval_loss`` that run logged for the same weights.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
from typing import Any, Dict, List, Optional

import torch


def evaluate_model(model, stream, batches: int, device) -> Dict[str, Any]:
    """``batches`` batches of the rewound ``stream`` (data.EvalStream) through ``model.loss_stats``, summed on the
    device in float64, all-reduced (SUM) over the default process group when there is one, then one host sync.
    ``eval_loss`` = sum of row losses / valid tokens over everything summed: token-weighted."""
    t0 = time.perf_counter()
    stream.reset()
    acc = torch.zeros(3, dtype=torch.float64, device=device)
    for _ in range(batches):
        batch = next(stream)
        acc += model.loss_stats(batch["input_ids"], batch["labels"], batch.get("attention_mask"))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.all_reduce(acc)
    loss_sum, n_valid, n_hit = acc.tolist()  # the one host sync
    loss = loss_sum / n_valid if n_valid else float("nan")
    return {"eval_loss": loss, "eval_perplexity": math.exp(min(loss, 80.0)) if loss == loss else float("nan"),
            "eval_accuracy": n_hit / n_valid if n_valid else float("nan"), "eval_tokens": int(n_valid),
            "eval_s": time.perf_counter() - t0}


def build_parser() -> argparse.ArgumentParser:
    from .main import _bool
    p = argparse.ArgumentParser(prog="nanodiloco_amd.evaluate", description="held-out evaluation of a checkpoint")
    p.add_argument("--checkpoint", required=True, help="a directory written by save_checkpoint (--checkpoint-dir)")
    p.add_argument("--llama-config-file", default=None, help="default: the checkpoint's config.json")
    p.add_argument("--data", default="synthetic", choices=["synthetic", "memmap"])
    p.add_argument("--eval-dataset-path", default=None)
    p.add_argument("--eval-batches", type=int, default=8)
    p.add_argument("--per-device-batch-size", type=int, default=8)
    p.add_argument("--seq-length", type=int, default=1024)
    p.add_argument("--seed", type=int, default=1337)
    p.add_argument("--dtype", default="auto", help="auto | fp32 | bf16")
    p.add_argument("--residual-dtype", default="auto", help="auto | fp32 | bf16")
    p.add_argument("--doc-mask", type=_bool, nargs="?", const=True, default=False)
    p.add_argument("--device", default="auto", help="auto | cpu | cuda")
    return p


def main(argv: Optional[List[str]] = None) -> Dict[str, Any]:
    from .config import LlamaConfig, resolve_llama_config
    from .data import build_eval_data
    from .models import LlamaForCausalLM
    from .trainer import _dtype, _residual_dtype, check_doc_mask
    from .utils.checkpoint import _load_st, find_checkpoint

    a = build_parser().parse_args(argv if argv is not None else sys.argv[1:])
    if a.eval_batches < 1:
        raise ValueError("--eval-batches must be at least 1")
    ckpt = find_checkpoint(a.checkpoint)
    if ckpt is None:
        raise FileNotFoundError(f"no complete checkpoint at {a.checkpoint}")
    dev = a.device if a.device != "auto" else ("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device("cuda", torch.cuda.current_device()) if dev == "cuda" else torch.device(dev)
    cfg = resolve_llama_config(a.llama_config_file) if a.llama_config_file \
        else LlamaConfig.from_json(os.path.join(ckpt, "config.json"))
    check_doc_mask(a.doc_mask, a.data, a.seq_length, device.type == "cuda")
    model = LlamaForCausalLM(cfg, device, _dtype(a.dtype, device), residual_dtype=_residual_dtype(a.residual_dtype),
                             doc_mask=a.doc_mask)
    model.load_state_dict(_load_st(os.path.join(ckpt, "model.safetensors")))
    stream = build_eval_data(a.data, vocab_size=cfg.vocab_size, seq_len=a.seq_length,
                             batch_size=a.per_device_batch_size, seed=a.seed, rank=0, world_size=1, device=device,
                             eval_dataset_path=a.eval_dataset_path)
    rec = {"checkpoint": ckpt, **evaluate_model(model, stream, a.eval_batches, device)}
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    main()
