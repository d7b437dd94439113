"""Capped against uncapped attention kernels, alternated in one process (docs/PROFILING.md): forward and fused
backward of ``ops.attention`` at the Llama-150M attention shape, device-event times, median of ``--rounds`` rounds.

  python scripts/ab_attn_softcap.py [--batch 8] [--seq 1024] [--heads 16] [--kv-heads 16] [--head-dim 64] [--cap 50]
"""
import argparse
import json
import statistics

import torch

from nanodiloco_amd import ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--kv-heads", type=int, default=16)
    ap.add_argument("--head-dim", type=int, default=64)
    ap.add_argument("--cap", type=float, default=50.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    ops.set_backend("hip")
    B, T, nh, nkv, hd = a.batch, a.seq, a.heads, a.kv_heads, a.head_dim
    dev = "cuda"
    qkv = torch.randn(B * T, (nh + 2 * nkv) * hd, device=dev).bfloat16()
    dO = torch.randn(B * T, nh * hd, device=dev).bfloat16()
    cos, sin = ops.rope_cache(T, hd, 10000.0, None, torch.device(dev))

    def run(cap, backward):
        x = qkv.clone().requires_grad_(backward)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        with torch.set_grad_enabled(backward):
            ev[0].record()
            o = ops.attention(x, cos, sin, B, T, nh, nkv, hd, inplace=True, softcap=cap)
            ev[1].record()
            if backward:
                o.backward(dO)
            ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

    res = {}
    for cap in (None, a.cap):  # warm-up of both
        for _ in range(3):
            run(cap, True)
    times = {(c, k): [] for c in (None, a.cap) for k in ("fwd", "bwd")}
    for _ in range(a.rounds):
        for cap in (None, a.cap):  # alternated
            f = b = 0.0
            for _ in range(a.iters):
                tf, tb = run(cap, True)
                f, b = f + tf, b + tb
            times[(cap, "fwd")].append(f / a.iters)
            times[(cap, "bwd")].append(b / a.iters)
    for k in ("fwd", "bwd"):
        u, c = statistics.median(times[(None, k)]), statistics.median(times[(a.cap, k)])
        res[k] = {"uncapped_ms": round(u, 4), "capped_ms": round(c, 4), "ratio": round(c / u, 3),
                  "uncapped_spread_ms": round(max(times[(None, k)]) - min(times[(None, k)]), 4)}
    print(json.dumps({"shape": [B, T, nh, nkv, hd], "cap": a.cap, **res}))


if __name__ == "__main__":
    main()
