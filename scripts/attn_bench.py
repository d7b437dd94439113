#!/usr/bin/env python3
"""Flash-attention kernel micro-benchmark (HIP path) on the Llama-150M micro-batch shape, with the
PyTorch SDPA (ROCm: AOTriton/CK) time on the same data for comparison.  Causal FLOPs counted as
half the full score matrix: fwd 2 GEMMs, bwd 5 (dkdv 4 + dq 3 recomputed = 7 executed).

``--doc-len L`` (0 = off): uniform documents of L tokens.  Times the document-masked launch
(``ops.attention(..., doc_bounds=...)``) next to the plain causal launch and the left-pad launch with a key start
of zeros (the masked kernels with nothing masked) of the same shape, interleaved in the same process: medians of
``--repeats`` rounds of ``--iters`` launches each, after a warm-up round.  ``--lib PATH`` adds the plain causal
launch of another build of the kernel library (e.g. the parent commit's, ``csrc/build.py --rev``).  The document
mode times the attention kernels alone: q|k count as already rotated, so no RoPE pass and no copy is in the figures.

``--window W`` (0 = off): the sliding-window launch (``ops.attention(..., window=W)``, W < T) timed the same way,
next to the plain causal and the left-pad launch, forward and fused backward."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.ops import _ext  # noqa: E402
from nanodiloco_amd.ops.attention import rope_cache  # noqa: E402


def bench(fn, iters=10):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def doc_mode(a, B, T, nh, nkv, hd):
    """Plain causal vs left-pad (key start 0) vs document mode (--doc-len) or sliding window (--window), forward and
    backward, interleaved."""
    L = a.doc_len or T
    ld = (nh + 2 * nkv) * hd
    qkv = torch.randn(B * T, ld, device="cuda").bfloat16()
    cos, sin = rope_cache(T, hd, 10000.0, None, "cuda")
    ids = torch.full((B, T), 7, dtype=torch.long, device="cuda")
    ids[:, L - 1::L] = 2  # an EOS closes every L-token document
    bounds = ops.doc_bounds(ids, 2)
    ops.check_doc_bounds(*bounds)
    ks0 = torch.zeros(B, dtype=torch.int32, device="cuda")
    x = qkv.clone().requires_grad_(True)
    do = torch.randn(B * T, nh * hd, device="cuda").bfloat16()
    other = _ext.load_library(a.lib) if a.lib else None

    def variant(kw, lib=None):
        def fwd():
            if lib is not None:
                with _ext.using(lib):
                    return ops.attention(x, cos, sin, B, T, nh, nkv, hd, inplace=True, rotated=True, **kw)
            return ops.attention(x, cos, sin, B, T, nh, nkv, hd, inplace=True, rotated=True, **kw)

        def bwd(o):
            if lib is not None:
                with _ext.using(lib):
                    return torch.autograd.grad(o, x, do, retain_graph=True)
            return torch.autograd.grad(o, x, do, retain_graph=True)
        return fwd, bwd

    variants = {"causal": variant({}), "leftpad ks=0": variant({"kstart": ks0})}
    if a.doc_len:
        variants[f"doc L={L}"] = variant({"doc_bounds": bounds})
    if a.window:
        variants[f"window W={a.window}"] = variant({"window": a.window})
    if other is not None:
        variants["causal (--lib)"] = variant({}, other)
    outs = {k: f() for k, (f, _) in variants.items()}
    times = {k: ([], []) for k in variants}
    for r in range(a.repeats + 1):  # round 0 is the warm-up
        for k, (f, g) in variants.items():
            tf = bench(f, a.iters)
            tb = bench(lambda: g(outs[k]), a.iters)
            if r:
                times[k][0].append(tf)
                times[k][1].append(tb)
    med = {k: (statistics.median(v[0]), statistics.median(v[1])) for k, v in times.items()}
    cf, cb = med["causal"]
    print(f"B={B} T={T} nh={nh} nkv={nkv} hd={hd} doc_len={a.doc_len} window={a.window}: median of {a.repeats} x {a.iters} launches")
    print("| launch | fwd us | fwd / causal | bwd us | bwd / causal |")
    print("|---|---|---|---|---|")
    for k, (tf, tb) in med.items():
        print(f"| {k} | {tf * 1e6:.1f} | {tf / cf:.3f} | {tb * 1e6:.1f} | {tb / cb:.3f} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--doc-len", type=int, default=0, help="uniform documents of this many tokens (0 = off)")
    ap.add_argument("--window", type=int, default=0, help="sliding window of this many keys, < T (0 = off)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--lib", default=None, help="another build of the kernel library: its plain causal launch is timed too")
    a = ap.parse_args()
    B = int(os.environ.get("B", 32))
    T = int(os.environ.get("T", 1024))
    nh = int(os.environ.get("NH", 16))
    nkv = int(os.environ.get("NKV", nh))
    hd = int(os.environ.get("HD", 64))
    ops.set_backend("hip")
    if a.doc_len or a.window:
        if a.doc_len and (a.doc_len < 1 or T % a.doc_len):
            raise SystemExit("--doc-len must divide T")
        if a.window and not 1 <= a.window < T:
            raise SystemExit("--window must lie in [1, T)")
        return doc_mode(a, B, T, nh, nkv, hd)
    ld = (nh + 2 * nkv) * hd
    qkv = torch.randn(B * T, ld, device="cuda").bfloat16()
    cos, sin = rope_cache(T, hd, 10000.0, None, "cuda")
    fl_fwd = 2 * 2 * B * nh * T * T * hd / 2
    x = qkv.clone().requires_grad_(True)
    t_fwd = bench(lambda: ops.attention(x, cos, sin, B, T, nh, nkv, hd))
    o = ops.attention(x, cos, sin, B, T, nh, nkv, hd)
    do = torch.randn_like(o)
    t_bwd = bench(lambda: torch.autograd.grad(o, x, do, retain_graph=True))
    print(f"ours  fwd {t_fwd * 1e6:8.1f} us {fl_fwd / t_fwd / 1e12:6.1f} TF/s | "
          f"bwd {t_bwd * 1e6:8.1f} us {2.5 * fl_fwd / t_bwd / 1e12:6.1f} TF/s (5-GEMM count)", flush=True)
    q = torch.randn(B, nh, T, hd, device="cuda").bfloat16().requires_grad_(True)
    k = torch.randn(B, nkv, T, hd, device="cuda").bfloat16().requires_grad_(True)
    v = torch.randn(B, nkv, T, hd, device="cuda").bfloat16().requires_grad_(True)
    f = lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=nkv != nh)
    try:
        t_sf = bench(f)
        out = f()
        g = torch.randn_like(out)
        t_sb = bench(lambda: torch.autograd.grad(out, (q, k, v), g, retain_graph=True))
        print(f"sdpa  fwd {t_sf * 1e6:8.1f} us {fl_fwd / t_sf / 1e12:6.1f} TF/s | "
              f"bwd {t_sb * 1e6:8.1f} us {2.5 * fl_fwd / t_sb / 1e12:6.1f} TF/s", flush=True)
    except Exception as e:  # noqa: BLE001
        print("sdpa unavailable:", type(e).__name__, e)


if __name__ == "__main__":
    main()
