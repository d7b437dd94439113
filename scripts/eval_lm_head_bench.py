#!/usr/bin/env python
"""Evaluation loss of an lm head: the loss-only path against the training path used for the same number.

  parent : ops.lm_head_ce(y, W, None, targets) under no_grad -- three GEMMs per chunk (logits, dgrad and, with a
           grad buffer, wgrad; without one still logits + dgrad) and the logits overwritten by their gradient
  new    : ops.lm_head_loss(y, W, targets) -- the logits GEMM and nd_ce_loss, which only reads them

Shape: the Llama-150M head (d = 768, V = 32000) at n = 16384 and n = 131072 rows (a 128 x 1024 micro-batch; skipped
with a note when it does not fit).  The two are timed interleaved in one process, round by round, with device
events around each call after a warm-up of every shape; the table gives median and minimum over the rounds, the
ratio, and the share of the new path spent in nd_ce_loss (timed alone on logits of the same shape) with its
achieved read rate.  Both paths must give the same loss (printed).  Needs a GPU: there is no CPU fall-back.

    python scripts/eval_lm_head_bench.py [--rounds 20] [--sizes 16384,131072] [--out profiles/eval_lm_head.md]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.ops import _ext  # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def bench(n, d, V, rounds, warmup, dev):
    g = torch.Generator(device=dev).manual_seed(n)
    y = (0.5 * torch.randn(n, d, device=dev, generator=g)).bfloat16()
    W = (0.05 * torch.randn(V, d, device=dev, generator=g)).bfloat16()
    tgt = torch.randint(0, V, (n,), device=dev, generator=g)
    tgt[::17] = ops.IGNORE_INDEX
    n_valid = int((tgt != ops.IGNORE_INDEX).sum())

    def parent():
        with torch.no_grad():
            return ops.lm_head_ce(y, W, None, tgt)

    def new():
        row_loss, _ = ops.lm_head_loss(y, W, tgt)
        return row_loss.sum(dtype=torch.float64) / n_valid

    logits = ops.mm_nt(y[:min(n, 65536)], W)  # nd_ce_loss alone, on one chunk's worth of rows
    rows = logits.shape[0]
    rl = torch.empty(rows, device=dev)
    hit = torch.empty(rows, dtype=torch.bool, device=dev)

    def kernel():
        _ext.check(_ext.lib().nd_ce_loss(_ext.ptr(logits), _ext.dtcode(logits), _ext.ptr(tgt), rows, V,
                                         ops.IGNORE_INDEX, _ext.ptr(rl), 0, _ext.ptr(hit),
                                         _ext.stream_ptr(y.device)), "nd_ce_loss")

    def gemm():
        return ops.mm_nt(y[:rows], W)

    fns = {"parent": parent, "new": new, "ce_loss_kernel": kernel, "logits_gemm": gemm}
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    vals = {}
    for _ in range(rounds):  # interleaved: one call of each per round
        for k, f in fns.items():
            t, out = timed(f)
            ms[k].append(t)
            vals[k] = out
    res = {"n": n, "d": d, "V": V, "rounds": rounds, "kernel_rows": rows,
           "loss_parent": float(vals["parent"]), "loss_new": float(vals["new"])}
    for k, v in ms.items():
        res[k + "_ms_median"], res[k + "_ms_min"] = statistics.median(v), min(v)
    res["speedup_median"] = res["parent_ms_median"] / res["new_ms_median"]
    res["speedup_min"] = res["parent_ms_min"] / res["new_ms_min"]
    res["ce_loss_read_GBps"] = rows * V * logits.element_size() / (res["ce_loss_kernel_ms_median"] * 1e-3) / 1e9
    return res


def table(results, notes):
    out = ["| n | parent lm_head_ce ms (median / min) | lm_head_loss ms (median / min) | parent / new (median, min) | "
           "logits GEMM ms | nd_ce_loss ms | rows | nd_ce_loss read GB/s | loss parent | loss new |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        out.append(f"| {r['n']} | {r['parent_ms_median']:.3f} / {r['parent_ms_min']:.3f} | "
                   f"{r['new_ms_median']:.3f} / {r['new_ms_min']:.3f} | {r['speedup_median']:.2f}x, "
                   f"{r['speedup_min']:.2f}x | {r['logits_gemm_ms_median']:.3f} | {r['ce_loss_kernel_ms_median']:.3f} | "
                   f"{r['kernel_rows']} | {r['ce_loss_read_GBps']:.0f} | {r['loss_parent']:.6f} | {r['loss_new']:.6f} |")
    return "\n".join(out + [""] + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="16384,131072")
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--out", default=None, help="also write the table (markdown) here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_lm_head_bench needs a GPU: a CPU timing says nothing about the kernels")
    ops.set_backend("hip")
    dev = torch.device("cuda")
    results, notes = [], []
    for n in [int(s) for s in a.sizes.split(",") if s]:
        try:
            r = bench(n, a.d, a.vocab, a.rounds, a.warmup, dev)
        except torch.cuda.OutOfMemoryError:
            notes.append(f"n = {n}: not measured (out of memory)")
            torch.cuda.empty_cache()
            continue
        results.append(r)
        print(json.dumps(r), flush=True)
    text = table(results, notes)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if any(r["speedup_median"] <= 1.0 for r in results):
        raise SystemExit("lm_head_loss is NOT faster than the parent path at every size")


if __name__ == "__main__":
    main()
