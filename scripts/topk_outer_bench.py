#!/usr/bin/env python
"""Device time of the two top-k transport kernels (csrc/sparse_comm.hip: ``nd_pseudograd_topk``,
``nd_outer_nesterov_topk``) at a model's flat size, interleaved in one process with the dense pair they stand
beside (``nd_pseudograd`` + ``nd_outer_nesterov`` with the same value dtype on the wire).

One sample of an arm is one launch over the whole flat vector.  The dense pair is timed TWICE as two arms (A and
A'): their ratio is the session's A/A spread.  HIP events around ``--iters`` samples, every arm warmed up, arms
alternated over ``--rounds`` rounds, median reported (docs/PROFILING.md).  The residual stays at zero between
samples of the select kernel only when the values are fp32; either way every sample reads and writes the same
bytes.  Writes a markdown report to ``--out``; when the top-k pair takes more than 1.5x the dense pair the report
names the kernel that carries the difference.

    python scripts/topk_outer_bench.py --model llama_150m.json --k 64 --out profiles/topk_outer_bench.md
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.config import resolve_llama_config  # noqa: E402
from nanodiloco_amd.models import LlamaForCausalLM  # noqa: E402

WIRE = {"fp32": torch.float32, "bf16": torch.bfloat16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama_150m.json")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--workers", type=int, default=1, help="slots in the gathered buffer the update reads")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_outer_bench.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    ops.set_backend("hip")
    cfg = resolve_llama_config(a.model)
    n = LlamaForCausalLM(cfg, "cpu").store.numel
    g = torch.Generator().manual_seed(0)
    master = torch.randn(n, generator=g).to(dev)
    sync = master + 0.01 * torch.randn(n, generator=g).to(dev)
    mom = torch.zeros(n, device=dev)
    resid = torch.zeros(n, device=dev)
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    w, lr, mu, k = a.workers, 1e-9, 0.9, a.k
    arms = {}  # name -> (callable, bytes per element)
    pairs = []  # (value dtype, select arm, update arm, dense pseudograd arms, dense update arms)
    for wk, vdt in WIRE.items():
        vs = 4 if vdt == torch.float32 else 2
        sb = ops.topk_slot_bytes(n, k, vdt)
        gath = torch.zeros(w * sb, dtype=torch.uint8, device=dev)
        for r in range(w):  # real slots in every worker's place
            ops.pseudograd_topk(sync, master, resid, gath[r * sb:(r + 1) * sb], k, vdt)
            resid.zero_()
        dense = torch.zeros(n, dtype=vdt, device=dev)
        wire_per_elem = k * (2 + vs) / 4096

        def sel(gath=gath, sb=sb, vdt=vdt):
            ops.pseudograd_topk(sync, master, resid, gath[:sb], k, vdt)

        def upd(gath=gath, vdt=vdt):
            ops.outer_nesterov_topk(master, sync, gath, w, k, vdt, mom, shadow, 1.0 / w, lr, mu, False)

        def dense_pg(dense=dense):
            ops.pseudograd(sync, master, dense)

        def dense_on(dense=dense):
            ops.outer_nesterov(master, sync, dense, mom, shadow, 1.0 / w, lr, mu, False)

        names = [f"nd_pseudograd_topk {wk} k={k}", f"nd_outer_nesterov_topk {wk} k={k} W={w}",
                 f"nd_pseudograd {wk} out A", f"nd_pseudograd {wk} out A'", f"nd_outer_nesterov {wk} in A",
                 f"nd_outer_nesterov {wk} in A'"]
        arms[names[2]] = (dense_pg, 8 + vs)
        arms[names[4]] = (dense_on, vs + 22)
        arms[names[0]] = (sel, 16 + wire_per_elem)          # sync, master, residual in; residual out; the slot
        arms[names[1]] = (upd, 22 + w * wire_per_elem)      # sync, momentum in; master, sync, momentum, shadow out
        arms[names[3]] = (dense_pg, 8 + vs)
        arms[names[5]] = (dense_on, vs + 22)
        pairs.append((wk, *names))
    times = {name: [] for name in arms}
    for fn, _ in arms.values():  # warm up every arm
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (fn, _) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters)
    med = {name: statistics.median(v) for name, v in times.items()}
    lines = ["# Top-k transport kernels (`csrc/sparse_comm.hip`): what they cost", "",
             f"`scripts/topk_outer_bench.py`: flat size n = {n} elements ({a.model}), k = {k} of every 4096, W = {w} "
             f"slot(s) read by the update, one sample = one launch over the whole vector, {a.iters} samples per "
             f"timing, {a.rounds} alternated rounds, median; HIP events; {torch.cuda.get_device_name(0)}.", "",
             "| arm | B / element | median ms | min..max ms | GB/s |", "|---|---|---|---|---|"]
    for name, v in times.items():
        bpe = arms[name][1]
        lines.append(f"| `{name}` | {bpe:.2f} | {med[name]:.4f} | {min(v):.4f}..{max(v):.4f} | "
                     f"{bpe * n / (med[name] * 1e-3) / 1e9:.0f} |")
    lines += ["", "| values | top-k pair ms | dense pair ms (A) | ratio | dense A'/A | select / dense pseudograd | "
                  "update / dense update |", "|---|---|---|---|---|---|---|"]
    notes = []
    for wk, s, u, pg, pg2, on, on2 in pairs:
        topk, dense, dense2 = med[s] + med[u], med[pg] + med[on], med[pg2] + med[on2]
        ratio = topk / dense
        lines.append(f"| {wk} | {topk:.4f} | {dense:.4f} | {ratio:.3f}x | {dense2 / dense:.3f}x | {med[s] / med[pg]:.3f}x | "
                     f"{med[u] / med[on]:.3f}x |")
        if ratio > 1.5:
            ds, du = med[s] - med[pg], med[u] - med[on]
            who = "`nd_pseudograd_topk` (the select)" if ds >= du else "`nd_outer_nesterov_topk` (the update)"
            notes.append(f"* {wk}: the pair takes {ratio:.2f}x the dense pair; {who} carries the difference "
                         f"({ds:+.4f} ms for the select, {du:+.4f} ms for the update against their dense counterparts).")
    lines += [""] + (notes or ["Both ratios are at or below 1.5x."])
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
