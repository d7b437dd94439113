#!/usr/bin/env python3
"""In-process, interleaved A/B of the lm-head CE kernels with and without z-loss (the style of scripts/ab_kernels.py:
variants are only compared inside one process, alternating).

  python scripts/ab_ce_zloss.py [--rows 8192] [--vocab 32000] [--rounds 20] [--iters 50] [--out FILE.md]

Two forms at the Llama-150M lm-head shape, bf16 logits:
  bf16 : nd_ce_fwd_bwd      vs nd_ce_z_fwd_bwd        (dlogits in place)
  e5m2 : nd_ce_fwd_bwd_q8   vs nd_ce_z_fwd_bwd_q8     (dlogits only as e5m2, the --fp8 lm head)
Every round times plain, z, plain again (HIP events around `iters` launches); the second plain run gives the spread
of the z-free kernel against itself in the same session, which is what the z / plain ratio is read against.  The
in-place form runs on its own output from the second launch on: the kernels have no data-dependent work, so the
time is that of the first launch.  Both z forms are checked once against the plain kernel's lse."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.ops import _ext  # noqa: E402

Z = 1e-4


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def workloads(n, V):
    L, S = _ext.lib(), _ext.stream_ptr()
    x0 = (3 * torch.randn(n, V, device="cuda")).bfloat16()
    logits = x0.clone()
    tgt = torch.randint(0, V, (n,), device="cuda")
    tgt[::11] = -100
    ce, zs = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    sc = torch.full((1,), 1.0 / n, device="cuda")
    q = torch.empty(n, V, device="cuda", dtype=torch.uint8)
    qs = torch.full((1,), 4096.0 * n, device="cuda")
    am = torch.zeros(64, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731

    def plain():
        _ext.check(L.nd_ce_fwd_bwd(p(logits), 1, p(tgt), p(ce), p(sc), n, V, -100, 0, 0, 0.0, S), "ce")

    def z():
        _ext.check(L.nd_ce_z_fwd_bwd(p(logits), 1, p(tgt), p(ce), p(zs), p(sc), n, V, -100, 0, 0, 0, Z, S), "ce_z")

    def plain8():
        _ext.check(L.nd_ce_fwd_bwd_q8(p(x0), 1, p(tgt), p(ce), p(sc), n, V, -100, 0, 0, p(q), p(qs), p(am), 64, 1, S),
                   "ce_q8")

    def z8():
        _ext.check(L.nd_ce_z_fwd_bwd_q8(p(x0), 1, p(tgt), p(ce), p(zs), p(sc), n, V, -100, 0, 0, 0, Z, p(q), p(qs),
                                        p(am), 64, 1, S), "ce_z_q8")

    # both z forms once against the plain kernel's lse: the z accumulator holds sum lse^2 over the valid rows
    lse = torch.empty(n, device="cuda")
    _ext.check(L.nd_ce_fwd_bwd(p(logits), 1, p(tgt), p(ce), p(sc), n, V, -100, p(lse), 0, 0.0, S), "ce")
    want = (lse[tgt != -100].double() ** 2).sum().item()
    for fn in (z, z8):
        logits.copy_(x0)
        zs.zero_()
        fn()
        assert abs(zs.item() - want) <= 1e-4 * want, (fn.__name__, zs.item(), want)
    logits.copy_(x0)
    return {"bf16": (plain, z), "e5m2": (plain8, z8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_ce_zloss.py measures on the GPU; there is none")
    ops.set_backend("hip")
    wl = workloads(a.rows, a.vocab)
    res = {k: {"plain": [], "z": [], "plain2": []} for k in wl}
    for _ in range(a.rounds):
        for k, (plain, z) in wl.items():
            res[k]["plain"].append(timed(plain, a.iters))
            res[k]["z"].append(timed(z, a.iters))
            res[k]["plain2"].append(timed(plain, a.iters))
    lines = [f"| form | plain us (median / min) | z us (median / min) | z / plain (median, min) | plain again / plain "
             f"(median; per-round min .. max) | z / plain per round (min .. max) |", "|---|---|---|---|---|---|"]
    for k, r in res.items():
        med = {v: statistics.median(r[v]) for v in r}
        mn = {v: min(r[v]) for v in r}
        self_r = [b / a_ for a_, b in zip(r["plain"], r["plain2"])]
        z_r = [b / a_ for a_, b in zip(r["plain"], r["z"])]
        lines.append(f"| {k} | {med['plain']:.1f} / {mn['plain']:.1f} | {med['z']:.1f} / {mn['z']:.1f} | "
                     f"{med['z'] / med['plain']:.4f}, {mn['z'] / mn['plain']:.4f} | {med['plain2'] / med['plain']:.4f}; "
                     f"{min(self_r):.4f} .. {max(self_r):.4f} | {min(z_r):.4f} .. {max(z_r):.4f} |")
    text = (f"rows {a.rows}, vocab {a.vocab}, bf16 logits, z_coef {Z}; {a.rounds} interleaved rounds x {a.iters} "
            f"launches, HIP events; {torch.cuda.get_device_name()}\n\n" + "\n".join(lines) + "\n")
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
