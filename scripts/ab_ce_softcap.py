#!/usr/bin/env python3
"""In-process, interleaved A/B of the lm-head CE kernels with and without logit soft-capping (the style of
scripts/ab_ce_zloss.py: variants are only compared inside one process, alternating).

  python scripts/ab_ce_softcap.py [--rows 8192] [--vocab 32000] [--rounds 20] [--iters 20] [--out FILE.md]

Three forms at the Llama-150M lm-head shape, bf16 logits, C = 30:
  bf16 : nd_ce_fwd_bwd      vs nd_ce_cap_fwd_bwd      (dlogits in place)
  e5m2 : nd_ce_fwd_bwd_q8   vs nd_ce_cap_fwd_bwd_q8   (dlogits only as e5m2, the --fp8 lm head)
  loss : nd_ce_loss         vs nd_ce_loss_cap         (evaluation: the logits are only read)
Every round times plain, capped, plain again (HIP events around `iters` launches); the second plain run gives the
spread of the cap-free kernel against itself in the same session, which is what the capped / plain ratio is read
against.  The in-place form runs on its own output from the second launch on: the kernels have no data-dependent work
(both tanh forms are computed and selected), so the time is that of the first launch.  The capped forms are checked
once against float64 on the first rows."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.ops import _ext  # noqa: E402

CAP = 30.0


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
    ce = torch.zeros(1, device="cuda")
    sc = torch.full((1,), 1.0 / n, device="cuda")
    q = torch.empty(n, V, device="cuda", dtype=torch.uint8)
    qs = torch.full((1,), 4096.0 * n, device="cuda")
    am = torch.zeros(64, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731

    def plain():
        _ext.check(L.nd_ce_fwd_bwd(p(logits), 1, p(tgt), p(ce), p(sc), n, V, -100, 0, 0, 0.0, S), "ce")

    def cap():
        _ext.check(L.nd_ce_cap_fwd_bwd(p(logits), 1, p(tgt), p(ce), 0, p(sc), n, V, -100, 0, 0, 0, 0.0, CAP, S), "ce_cap")

    def plain8():
        _ext.check(L.nd_ce_fwd_bwd_q8(p(x0), 1, p(tgt), p(ce), p(sc), n, V, -100, 0, 0, p(q), p(qs), p(am), 64, 1, S),
                   "ce_q8")

    def cap8():
        _ext.check(L.nd_ce_cap_fwd_bwd_q8(p(x0), 1, p(tgt), p(ce), 0, p(sc), n, V, -100, 0, 0, 0, 0.0, CAP, p(q), p(qs),
                                          p(am), 64, 1, S), "ce_cap_q8")

    rows, hit = torch.empty(n, device="cuda"), torch.empty(n, device="cuda", dtype=torch.uint8)

    def loss():
        _ext.check(L.nd_ce_loss(p(x0), 1, p(tgt), n, V, -100, p(rows), 0, p(hit), S), "ce_loss")

    def loss_cap():
        _ext.check(L.nd_ce_loss_cap(p(x0), 1, p(tgt), n, V, -100, p(rows), 0, p(hit), CAP, S), "ce_loss_cap")

    # the capped forms once against float64 on the first 64 rows
    k = min(n, 64)
    y = CAP * torch.tanh(x0[:k].double() / CAP)
    ok = tgt[:k] != -100
    want = (torch.logsumexp(y, -1) - y.gather(1, tgt[:k].clamp_min(0)[:, None])[:, 0])[ok]
    loss_cap()
    assert float((rows[:k][ok].double() - want).abs().max()) <= 1e-4, "nd_ce_loss_cap"
    r2 = torch.empty(n, device="cuda")
    _ext.check(L.nd_ce_cap_fwd_bwd(p(logits), 1, p(tgt), p(ce), 0, p(sc), n, V, -100, 0, p(r2), 0, 0.0, CAP, S), "ce_cap")
    assert float((r2[:k][ok].double() - want).abs().max()) <= 1e-4, "nd_ce_cap_fwd_bwd"
    logits.copy_(x0)
    return {"bf16": (plain, cap), "e5m2": (plain8, cap8), "loss": (loss, loss_cap)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_ce_softcap.py measures on the GPU; there is none")
    ops.set_backend("hip")
    wl = workloads(a.rows, a.vocab)
    res = {k: {"plain": [], "cap": [], "plain2": []} for k in wl}
    for _ in range(a.rounds):
        for k, (plain, cap) in wl.items():
            res[k]["plain"].append(timed(plain, a.iters))
            res[k]["cap"].append(timed(cap, a.iters))
            res[k]["plain2"].append(timed(plain, a.iters))
    lines = [f"| form | plain us (median / min) | capped us (median / min) | capped / plain (median, min) | plain again / "
             f"plain (median; per-round min .. max) | capped / plain per round (min .. max) |", "|---|---|---|---|---|---|"]
    for k, r in res.items():
        med = {v: statistics.median(r[v]) for v in r}
        mn = {v: min(r[v]) for v in r}
        self_r = [b / a_ for a_, b in zip(r["plain"], r["plain2"])]
        c_r = [b / a_ for a_, b in zip(r["plain"], r["cap"])]
        lines.append(f"| {k} | {med['plain']:.1f} / {mn['plain']:.1f} | {med['cap']:.1f} / {mn['cap']:.1f} | "
                     f"{med['cap'] / med['plain']:.4f}, {mn['cap'] / mn['plain']:.4f} | {med['plain2'] / med['plain']:.4f}; "
                     f"{min(self_r):.4f} .. {max(self_r):.4f} | {min(c_r):.4f} .. {max(c_r):.4f} |")
    text = (f"rows {a.rows}, vocab {a.vocab}, bf16 logits, C = {CAP}; {a.rounds} interleaved rounds x {a.iters} "
            f"launches, HIP events; {torch.cuda.get_device_name()}\n\n" + "\n".join(lines) + "\n")
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
