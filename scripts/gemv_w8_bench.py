#!/usr/bin/env python
"""fp8 and fp4 weight-only decode projections, timed on the GPU (profiles/w8_gemv.md, profiles/w4_gemv.md).

  kernel : ``nd_gemv_w8`` (ops.gemv_w8) and ``nd_gemv_w4`` (ops.gemv_w4) against what ``ops.mm_nt`` dispatches for the
           same (M, N, K) on the bf16 weight with the fp8 path's (dequantised) values, at the projection shapes of
           Llama-1B and Llama-150M, the lm head included, M in {1, 4, 16}.  Each variant's launches are captured in a
           HIP graph (as the decode step runs them: no host time between launches) that walks over as many copies of
           the weight as the model streams per token (up to 256), so a copy is as cold at its next use as in a decode
           step.  The graphs alternate in one process, round by round, device events around a replay; per shape the
           median / min / max over the rounds, the ratios, and the weight bytes of a call over the median time.
  e2e    : ``python -m nanodiloco_amd.generate`` semantics in process: Llama-1B from ``init_weights``, prompt 128,
           ``--new`` new tokens, B in {1, 8}, HIP graph; per format (fp8, then fp4) bf16 against the format's weights
           inside its ``quantized_weights`` context, rounds interleaved; decode tokens/s from (whole run) - (prompt
           pass with one new token), as the CLI reports it.

    python scripts/gemv_w8_bench.py [--rounds 15] [--e2e-rounds 3] [--new 128] [--skip-e2e]

Needs a GPU: there is no CPU fall-back.
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
from nanodiloco_amd.config import resolve_llama_config  # noqa: E402
from nanodiloco_amd.ops import gemv  # noqa: E402


def shapes(name):
    c = resolve_llama_config(f"llama_{name}.json")
    d, F = c.hidden_size, c.intermediate_size
    qkv = (c.num_attention_heads + 2 * c.num_key_value_heads) * c.head_dim
    return [("qkv", qkv, d), ("o", d, d), ("gate|up", 2 * F, d), ("down", d, F), ("lm_head", c.vocab_size, d)]


def graphed(fn, copies, inner):
    """``inner`` launches of ``fn(i % copies)`` captured in one HIP graph (no host time between launches)."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(inner):
            fn(i % copies)
    return g


def timed(graph, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    graph.replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def bench_kernel(model, proj, M, N, K, rounds, model_bytes, dev):
    g = torch.Generator(device=dev).manual_seed(N + K + M)
    codes, exps = gemv.quantize_weight(torch.randn(N, K, device=dev, generator=g) * 0.02)
    w = gemv.dequantize_weight(codes, exps, torch.bfloat16)
    # as many copies of the weight as one decode step of the model streams between two uses of it
    copies = max(1, min(256, model_bytes // (2 * N * K)))
    inner = copies * max(1, 32 // copies)
    cs, es, wb = [codes.clone() for _ in range(copies)], [exps.clone() for _ in range(copies)], \
        [w.clone() for _ in range(copies)]
    codes4, exps4 = gemv.quantize_weight_fp4(w)  # other values than fp8's: the times do not depend on them
    cs4, es4 = [codes4.clone() for _ in range(copies)], [exps4.clone() for _ in range(copies)]
    x = torch.randn(M, K, device=dev, generator=g).bfloat16()
    ws, ws4 = gemv.gemv_w8_workspace(N, K, dev), gemv.gemv_w4_workspace(N, K, dev)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    fns = {"bf16": lambda i: ops.mm_nt(x, wb[i]), "fp8": lambda i: gemv.gemv_w8(x, cs[i], es[i], out=out, workspace=ws),
           "fp4": lambda i: gemv.gemv_w4(x, cs4[i], es4[i], out=out, workspace=ws4)}
    vals = {k: f(0).float().clone() for k, f in fns.items()}  # also the warm-up: code objects, GEMM algorithm selection
    ref4 = ops.mm_nt(x, gemv.dequantize_weight_fp4(codes4, exps4, torch.bfloat16)).float()
    torch.cuda.synchronize()
    graphs = {k: graphed(f, copies, inner) for k, f in fns.items()}
    for gr in graphs.values():
        gr.replay()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, gr in graphs.items():
            ms[k].append(timed(gr, inner))
    nbytes = {"bf16": N * K * 2, "fp8": N * K + N * K // 128, "fp4": N * K // 2 + N * K // 32}
    r = {"model": model, "proj": proj, "M": M, "N": N, "K": K, "copies": copies, "inner": inner,
         "max_diff": float((vals["bf16"] - vals["fp8"]).abs().max()),
         "fp4_max_diff": float((ref4 - vals["fp4"]).abs().max())}
    for k, v in ms.items():
        r[k + "_us_median"], r[k + "_us_min"], r[k + "_us_max"] = 1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v)
        r[k + "_GBps"] = nbytes[k] / (r[k + "_us_median"] * 1e-6) / 1e9
    r["fp8_over_bf16"] = r["fp8_us_median"] / r["bf16_us_median"]
    r["fp4_over_bf16"] = r["fp4_us_median"] / r["bf16_us_median"]
    r["fp4_over_fp8"] = r["fp4_us_median"] / r["fp8_us_median"]
    return r


def bench_e2e(m, fmt, B, prompt, new, rounds, dev):
    ids = torch.randint(3, m.config.vocab_size, (B, prompt), device=dev)
    secs = {"bf16": {1: [], new: []}, fmt: {1: [], new: []}}
    with m.quantized_weights(fmt):  # both variants on the same (rounded) numbers; the quantisation stays untimed
        wq = m.wq
        for timed_round in [False] + [True] * rounds:
            for wd in secs:
                m.wq = wq if wd == fmt else None  # None: ops.mm_nt on the rounded shadow, the bf16 path
                for n in (1, new):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    m.generate(ids, max_new_tokens=n, eos_token_id=None, hip_graph=True)
                    torch.cuda.synchronize()
                    if timed_round:
                        secs[wd][n].append(time.perf_counter() - t0)
        m.wq = wq
    r = {"weights": fmt, "B": B, "prompt": prompt, "new": new, "rounds": rounds}
    for wd, v in secs.items():
        dec = [a - b for a, b in zip(v[new], v[1])]
        r[wd + "_decode_tokens_per_s"] = B * (new - 1) / statistics.median(dec)
        r[wd + "_decode_tokens_per_s_range"] = [B * (new - 1) / max(dec), B * (new - 1) / min(dec)]
    r[fmt + "_over_bf16_tokens"] = r[fmt + "_decode_tokens_per_s"] / r["bf16_decode_tokens_per_s"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemv_w8_bench needs a GPU: a CPU timing says nothing about the kernels")
    ops.set_backend("hip")
    dev = torch.device("cuda")
    for model in ("1b", "150m"):
        sh = shapes(model)
        layers = resolve_llama_config(f"llama_{model}.json").num_hidden_layers
        model_bytes = 2 * (layers * sum(N * K for _, N, K in sh[:-1]) + sh[-1][1] * sh[-1][2])
        for proj, N, K in sh:
            for M in (1, 4, 16):
                print(json.dumps(bench_kernel(model, proj, M, N, K, a.rounds, model_bytes, dev)), flush=True)
    if not a.skip_e2e:
        from nanodiloco_amd.models import LlamaForCausalLM
        m = LlamaForCausalLM(resolve_llama_config("llama_1b.json"), dev, torch.bfloat16).init_weights(0).eval()
        for fmt in ("fp8", "fp4"):
            for B in (1, 8):
                print(json.dumps(bench_e2e(m, fmt, B, 128, a.new, a.e2e_rounds, dev)), flush=True)


if __name__ == "__main__":
    main()
