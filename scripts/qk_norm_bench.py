"""Kernel time of the QK-norm kernels (csrc/qk_norm.hip) on one GPU, in process and interleaved:

  fused      nd_qk_norm_rope_fwd (no save: prefill / evaluation)
  fused+save nd_qk_norm_rope_fwd also writing the raw q|k for the backward (the training forward)
  composed   nd_qk_norm followed by nd_rope_inplace: what the fused forward replaces
  bwd        nd_qk_norm_bwd (with the finishing reduction of the weight-gradient partials)
  rmsnorm    nd_rmsnorm_fwd on [N, d] bf16 -> bf16: the streaming rate csrc/norm.hip reaches on the same box

Times are HIP-event times of `--iters` back-to-back launches, the arms alternated `--rounds` times; bytes are the
bytes the algorithm has to move, computed from the shapes.  One JSON line per shape.

  python scripts/qk_norm_bench.py [--shapes 150m,1b] [--iters 20] [--rounds 5]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.ops import _ext  # noqa: E402

qkn = importlib.import_module("nanodiloco_amd.ops.qk_norm")
attn = importlib.import_module("nanodiloco_amd.ops.attention")

# name: (rows of a micro-batch, T, nh, nkv, hd, d)
SHAPES = {"150m": (128 * 1024, 1024, 16, 16, 64, 1024), "1b": (64 * 1024, 1024, 32, 4, 64, 2048)}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="150m,1b")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("qk_norm_bench needs a GPU")
    ops.set_backend("hip")
    dev = "cuda"
    for name in a.shapes.split(","):
        N, T, nh, nkv, hd, d = SHAPES[name]
        B, W, nqk, eps = N // T, (nh + 2 * nkv) * hd, (nh + nkv) * hd, 1e-5
        x = torch.randn(N, W, device=dev).to(torch.bfloat16)
        dy = torch.randn(N, W, device=dev).to(torch.bfloat16)
        wq, wk = 0.5 + torch.rand(hd, device=dev), 0.5 + torch.rand(hd, device=dev)
        gwq, gwk = torch.zeros(hd, device=dev), torch.zeros(hd, device=dev)
        cos, sin = ops.rope_cache(T, hd, 10000.0, None, torch.device(dev))
        rstd, raw = qkn.qk_norm_rope_fwd_launch(x.clone(), wq, wk, cos, sin, T, nh, nkv, hd, eps, save=True)
        h = torch.randn(N, d, device=dev).to(torch.bfloat16)
        wn = torch.ones(d, device=dev)
        L = _ext.lib()
        s = _ext.stream_ptr(torch.device(dev))
        y, rs = torch.empty_like(h), torch.empty(N, dtype=torch.float32, device=dev)
        rstd2 = torch.empty_like(rstd)
        raw2 = torch.empty_like(raw)

        def fused(save):
            _ext.check(L.nd_qk_norm_rope_fwd(_ext.ptr(x), 1, _ext.ptr(wq), _ext.ptr(wk), _ext.ptr(cos), _ext.ptr(sin),
                                             _ext.ptr(rstd2), _ext.ptr(raw2) if save else 0, N, T, nh, nkv, hd, W, eps,
                                             s), "nd_qk_norm_rope_fwd")

        def composed():
            ops.qk_norm(x, wq, wk, nh, nkv, hd, eps)
            attn._rope(x, cos, sin, B, T, nh, nkv, hd, inverse=False)

        arms = {
            "fused": (lambda: fused(False), 2 * nqk * 2 + 4 * (nh + nkv)),
            "fused+save": (lambda: fused(True), 3 * nqk * 2 + 4 * (nh + nkv)),
            "composed": (composed, 4 * nqk * 2),
            "bwd": (lambda: qkn.qk_norm_bwd_launch(dy, raw, rstd, wq, wk, gwq, gwk, nh, nkv, hd),
                    3 * nqk * 2 + 4 * (nh + nkv)),
            "rmsnorm": (lambda: _ext.check(L.nd_rmsnorm_fwd(_ext.ptr(h), 1, 0, 0, _ext.ptr(wn), _ext.ptr(y), 1, 0,
                                                            _ext.ptr(rs), N, d, eps, s), "nd_rmsnorm_fwd"),
                        2 * d * 2 + 4),
        }
        for fn, _ in arms.values():  # warm up every arm (the values drift in place: timing only)
            x.copy_(torch.randn_like(x))
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, (fn, _) in arms.items():
                x.normal_()
                dy.normal_()
                torch.cuda.synchronize()
                times[k].append(timed(fn, a.iters))
        out = {"shape": name, "rows": N, "nh": nh, "nkv": nkv, "hd": hd}
        for k, (_, bytes_per_row) in arms.items():
            med = statistics.median(times[k])
            out[k] = {"us": round(med, 1), "min_us": round(min(times[k]), 1), "max_us": round(max(times[k]), 1),
                      "TB_per_s": round(bytes_per_row * N / med / 1e6, 3)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
