#!/usr/bin/env python
"""Decode attention and cached generation, timed on the GPU.

  kernel : ``nd_attn_decode`` (ops.decode.attn_decode_launch) against its PyTorch twin (the ``--ops torch`` path,
           ops.decode.attention_decode_torch) on the same cache, at the Llama-150M (nh 16, nkv 16, hd 64) and
           Llama-1B (nh 32, nkv 4, hd 64) head shapes, B in {1, 8, 64}, cache lengths {128, 1024, 2048} inside an
           S_max = 2048 cache.  The two are timed interleaved in one process, round by round, device events around
           ``--inner`` back-to-back calls after a warm-up of every shape; the table gives the per-call median and
           minimum over the rounds, the ratio, and the K/V bytes the step has to read (2 * B * nkv * len * hd * 2)
           over the kernel's median time.  Small caches are launch- and latency-bound: their rate says so, not how
           fast the reader is.  Both paths must agree (max difference printed).
  e2e    : ``model.generate`` of Llama-150M (random weights), prompt 128, 256 new tokens, B in {1, 8}: recompute
           (``use_cache=False``, what the code could do before the cache) vs cached eager vs cached HIP graph, a host
           clock around the call with a device synchronise, rounds interleaved; tokens/s = B * new / seconds.

    python scripts/decode_bench.py [--rounds 20] [--inner 20] [--e2e-rounds 3] [--skip-e2e] [--out FILE.md]

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
from nanodiloco_amd.ops import decode  # noqa: E402
from nanodiloco_amd.ops.attention import rope_cache  # noqa: E402

SHAPES = {"150m": (16, 16, 64), "1b": (32, 4, 64)}
S_MAX = 2048


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner, out


def bench_kernel(name, B, length, rounds, inner, warmup, dev):
    nh, nkv, hd = SHAPES[name]
    g = torch.Generator(device=dev).manual_seed(B * 7 + length)
    kc = torch.randn(B, nkv, S_MAX, hd, device=dev, generator=g).bfloat16()
    vc = torch.randn(B, nkv, S_MAX, hd, device=dev, generator=g).bfloat16()
    qkv = torch.randn(B, (nh + 2 * nkv) * hd, device=dev, generator=g).bfloat16()
    cos, sin = rope_cache(S_MAX, hd, 10000.0, None, dev)
    pos = torch.full((B,), length - 1, dtype=torch.int32, device=dev)
    ks = torch.zeros(B, dtype=torch.int32, device=dev)
    part_o, part_ml = decode.decode_workspace(B, nh, hd, S_MAX, dev)
    out = torch.empty(B, nh * hd, dtype=torch.bfloat16, device=dev)
    fns = {"hip": lambda: decode.attn_decode_launch(qkv, cos, sin, pos, ks, kc, vc, part_o, part_ml, nh, nkv, hd, out=out),
           "torch": lambda: decode.attention_decode_torch(qkv, cos, sin, pos, ks, kc, vc, nh, nkv, hd)}
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms, vals = {k: [] for k in fns}, {}
    for _ in range(rounds):  # interleaved: one timed burst of each per round
        for k, f in fns.items():
            t, o = timed(f, inner)
            ms[k].append(t)
            vals[k] = o.float().clone()
    kv_bytes = 2 * B * nkv * length * hd * 2
    r = {"shape": name, "B": B, "len": length, "kv_MB": kv_bytes / 1e6, "rounds": rounds, "inner": inner,
         "max_diff": float((vals["hip"] - vals["torch"]).abs().max())}
    for k, v in ms.items():
        r[k + "_us_median"], r[k + "_us_min"] = 1e3 * statistics.median(v), 1e3 * min(v)
        r[k + "_us_p90"] = 1e3 * sorted(v)[int(0.9 * (len(v) - 1))]
    r["torch_over_hip"] = r["torch_us_median"] / r["hip_us_median"]
    r["hip_kv_GBps"] = kv_bytes / (r["hip_us_median"] * 1e-6) / 1e9
    return r


def bench_window(name, B, length, window, rounds, inner, warmup, dev):
    """``nd_attn_decode_win`` against ``nd_attn_decode`` on the same cache at position ``length - 1``, interleaved."""
    nh, nkv, hd = SHAPES[name]
    s_max = max(S_MAX, length)
    g = torch.Generator(device=dev).manual_seed(B * 7 + length)
    kc = torch.randn(B, nkv, s_max, hd, device=dev, generator=g).bfloat16()
    vc = torch.randn(B, nkv, s_max, hd, device=dev, generator=g).bfloat16()
    qkv = torch.randn(B, (nh + 2 * nkv) * hd, device=dev, generator=g).bfloat16()
    cos, sin = rope_cache(s_max, hd, 10000.0, None, dev)
    pos = torch.full((B,), length - 1, dtype=torch.int32, device=dev)
    ks = torch.zeros(B, dtype=torch.int32, device=dev)
    part_o, part_ml = decode.decode_workspace(B, nh, hd, s_max, dev)
    out = torch.empty(B, nh * hd, dtype=torch.bfloat16, device=dev)
    fns = {"full": lambda: decode.attn_decode_launch(qkv, cos, sin, pos, ks, kc, vc, part_o, part_ml, nh, nkv, hd, out=out),
           "window": lambda: decode.attn_decode_launch(qkv, cos, sin, pos, ks, kc, vc, part_o, part_ml, nh, nkv, hd,
                                                       out=out, window=window)}
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            ms[k].append(timed(f, inner)[0])
    r = {"shape": name, "B": B, "len": length, "window": window, "s_max": s_max}
    for k, v in ms.items():
        r[k + "_us_median"], r[k + "_us_min"] = 1e3 * statistics.median(v), 1e3 * min(v)
    r["window_over_full"] = r["window_us_median"] / r["full_us_median"]
    return r


def bench_e2e(B, prompt, new, rounds, dev):
    from nanodiloco_amd.config import resolve_llama_config
    from nanodiloco_amd.models import LlamaForCausalLM
    cfg = resolve_llama_config("llama_150m.json")
    m = LlamaForCausalLM(cfg, dev, torch.bfloat16).init_weights(0).eval()
    ids = torch.randint(3, cfg.vocab_size, (B, prompt), device=dev)
    modes = {"recompute": dict(use_cache=False, hip_graph=False), "cached_eager": dict(hip_graph=False),
             "cached_graph": dict(hip_graph=True)}
    outs, secs = {}, {k: [] for k in modes}
    for k, kw in modes.items():  # warm-up: every shape of the timed window (the recompute path: 256 lengths)
        outs[k] = m.generate(ids, max_new_tokens=new, eos_token_id=None, **kw)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, kw in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(ids, max_new_tokens=new, eos_token_id=None, **kw)
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
    r = {"B": B, "prompt": prompt, "new": new, "rounds": rounds,
         "same_tokens_graph_eager": bool(torch.equal(outs["cached_eager"], outs["cached_graph"])),
         "tokens_equal_recompute_share": float((outs["cached_eager"] == outs["recompute"]).float().mean())}
    for k, v in secs.items():
        r[k + "_s_median"], r[k + "_s_min"], r[k + "_s_max"] = statistics.median(v), min(v), max(v)
        r[k + "_tok_per_s"] = B * new / statistics.median(v)
    return r


def tables(kern, e2e):
    out = ["| shape | B | len | K/V MB | nd_attn_decode us (median / min / p90) | torch twin us (median / min) | "
           "twin / kernel | K/V read GB/s | max diff |", "|---|---|---|---|---|---|---|---|---|"]
    for r in kern:
        out.append(f"| {r['shape']} | {r['B']} | {r['len']} | {r['kv_MB']:.2f} | {r['hip_us_median']:.1f} / "
                   f"{r['hip_us_min']:.1f} / {r['hip_us_p90']:.1f} | {r['torch_us_median']:.1f} / "
                   f"{r['torch_us_min']:.1f} | {r['torch_over_hip']:.1f}x | {r['hip_kv_GBps']:.0f} | "
                   f"{r['max_diff']:.2e} |")
    if e2e:
        out += ["", "| B | recompute s (median, min..max) / tok/s | cached eager s / tok/s | cached graph s / tok/s | "
                    "graph == eager tokens |", "|---|---|---|---|---|"]
        for r in e2e:
            cell = lambda k: (f"{r[k + '_s_median']:.3f} ({r[k + '_s_min']:.3f}..{r[k + '_s_max']:.3f}) / "
                              f"{r[k + '_tok_per_s']:.0f}")
            out.append(f"| {r['B']} | {cell('recompute')} | {cell('cached_eager')} | {cell('cached_graph')} | "
                       f"{r['same_tokens_graph_eager']} |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--window", type=int, default=0,
                    help="time the sliding-window decode step (this many keys) against the full one at --len, and stop")
    ap.add_argument("--len", type=int, default=4096, help="with --window: keys in the cache (pos = len - 1)")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench needs a GPU: a CPU timing says nothing about the kernels")
    ops.set_backend("hip")
    dev = torch.device("cuda")
    if a.window:
        for name in SHAPES:
            for B in (1, 8, 64):
                print(json.dumps(bench_window(name, B, a.len, a.window, a.rounds, a.inner, a.warmup, dev)), flush=True)
        return
    kern, e2e = [], []
    for name in SHAPES:
        for B in (1, 8, 64):
            for length in (128, 1024, 2048):
                r = bench_kernel(name, B, length, a.rounds, a.inner, a.warmup, dev)
                kern.append(r)
                print(json.dumps(r), flush=True)
    if not a.skip_e2e:
        for B in (1, 8):
            r = bench_e2e(B, 128, 256, a.e2e_rounds, dev)
            e2e.append(r)
            print(json.dumps(r), flush=True)
    text = tables(kern, e2e)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
