#!/usr/bin/env python
"""The sampling step of generation, timed on the GPU: ``sampler="torch"`` (``filter_logits`` + ``torch.multinomial``)
against ``sampler="fused"`` (``torch.rand`` + ``nd_sample_topk_topp``), both through ``models.llama.sample_logits``.

  step : V in {32000, 128256}, B in {1, 32}, temperature 0.8, top_k 50, top_p 0.9 on seeded randn * 4 logits.  The two
         alternate in one process, round by round, device events around ``--inner`` back-to-back calls after a warm-up
         of every shape; per-call median, minimum and p90 over the rounds.  Bytes per row are from the shapes: the
         fused kernel reads V * 4 + 4 and writes 8 (resident rows) -- the streaming variant re-reads the row per pass.
  e2e  : ``model.generate`` of Llama-150M (random weights), prompt 128, 256 new tokens, B in {1, 8}, HIP graph, both
         samplers, rounds interleaved, a host clock around the call with a device synchronise.

    python scripts/sample_bench.py [--rounds 20] [--inner 50] [--e2e-rounds 3] [--skip-e2e] [--out FILE.md]

Kernel times come from a run of their own: ``rocprofv3 --kernel-trace --stats -- python scripts/sample_bench.py
--skip-e2e --rounds 3``.  Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.models.llama import sample_logits  # noqa: E402

KW = dict(temperature=0.8, top_k=50, top_p=0.9)
SAMPLERS = ("torch", "fused")


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def bench_step(V, B, rounds, inner, warmup, dev):
    g = torch.Generator(device=dev).manual_seed(V + B)
    logits = torch.randn(B, V, device=dev, generator=g) * 4
    gen = torch.Generator(device=dev).manual_seed(1)
    fns = {k: (lambda k=k: sample_logits(logits, generator=gen, sampler=k, **KW)) for k in SAMPLERS}
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):  # interleaved: one timed burst of each per round
        for k, f in fns.items():
            ms[k].append(timed(f, inner))
    r = {"V": V, "B": B, "rounds": rounds, "inner": inner, "row_bytes": V * 4}
    for k, v in ms.items():
        r[k + "_us_median"], r[k + "_us_min"] = 1e3 * statistics.median(v), 1e3 * min(v)
        r[k + "_us_p90"] = 1e3 * sorted(v)[int(0.9 * (len(v) - 1))]
    r["torch_over_fused"] = r["torch_us_median"] / r["fused_us_median"]
    return r


def bench_e2e(B, prompt, new, rounds, dev):
    from nanodiloco_amd.config import resolve_llama_config
    from nanodiloco_amd.models import LlamaForCausalLM
    m = LlamaForCausalLM(resolve_llama_config("llama_150m.json"), dev, torch.bfloat16).init_weights(0).eval()
    ids = torch.randint(3, m.config.vocab_size, (B, prompt), device=dev)
    secs = {k: {1: [], new: []} for k in SAMPLERS}
    for timed_round in [False] + [True] * rounds:  # one untimed pass of every shape first
        for k in SAMPLERS:
            for n in (1, new):  # the prompt pass alone, then the whole run: the difference is the decode time
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.generate(ids, max_new_tokens=n, eos_token_id=None, hip_graph=True, sampler=k, seed=1, **KW)
                torch.cuda.synchronize()
                if timed_round:
                    secs[k][n].append(time.perf_counter() - t0)
    r = {"B": B, "prompt": prompt, "new": new, "rounds": rounds, "V": m.config.vocab_size}
    for k, v in secs.items():
        dec = [a - statistics.median(v[1]) for a in v[new]]
        r[k + "_decode_s_median"], r[k + "_decode_s_min"], r[k + "_decode_s_max"] = statistics.median(dec), min(dec), max(dec)
        r[k + "_decode_tokens_per_s"] = B * (new - 1) / statistics.median(dec)
    return r


def tables(step, e2e):
    out = ["| V | B | row KB | torch us (median / min / p90) | fused us (median / min / p90) | torch / fused |",
           "|---|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k + '_us_median']:.1f} / {r[k + '_us_min']:.1f} / {r[k + '_us_p90']:.1f}"
    for r in step:
        out.append(f"| {r['V']} | {r['B']} | {r['row_bytes'] / 1e3:.0f} | {cell(r, 'torch')} | {cell(r, 'fused')} | "
                   f"{r['torch_over_fused']:.1f}x |")
    if e2e:
        out += ["", "| B | torch decode s (median, min..max) / tok/s | fused decode s (median, min..max) / tok/s |", "|---|---|---|"]
        cell = lambda r, k: (f"{r[k + '_decode_s_median']:.3f} ({r[k + '_decode_s_min']:.3f}..{r[k + '_decode_s_max']:.3f}) / "
                             f"{r[k + '_decode_tokens_per_s']:.0f}")
        out += [f"| {r['B']} | {cell(r, 'torch')} | {cell(r, 'fused')} |" for r in e2e]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench needs a GPU: a CPU timing says nothing about the kernel")
    ops.set_backend("hip")
    dev = torch.device("cuda")
    step, e2e = [], []
    for V in (32000, 128256):
        for B in (1, 32):
            step.append(bench_step(V, B, a.rounds, a.inner, a.warmup, dev))
            print(json.dumps(step[-1]), flush=True)
    if not a.skip_e2e:
        for B in (1, 8):
            e2e.append(bench_e2e(B, 128, 256, a.e2e_rounds, dev))
            print(json.dumps(e2e[-1]), flush=True)
    text = tables(step, e2e)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
