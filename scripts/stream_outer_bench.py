#!/usr/bin/env python
"""Device time of the Streaming DiLoCo fragment kernels (csrc/stream_outer.hip) on a model's fragment tables,
interleaved in one process with the contiguous kernels they stand beside (``nd_pseudograd``,
``nd_outer_nesterov``) at the same element count and the same number of launches.

For every P in ``--fragments`` one sample of an arm runs the kernel once per fragment (P launches, together
the whole flat vector); the contiguous baseline runs over ranges ``[0, total_p)`` of the same lengths.  Every
baseline is timed TWICE as two separate arms (A and A'): their ratio is the session's A/A spread, the yardstick
for "within noise".  The expectation is parity with the baseline for ``nd_frag_pseudograd`` and the alpha = 0
update (same bytes per element) and 30/26 of the baseline time for alpha > 0 (the master is read as well).
HIP events around ``--iters`` samples, every arm warmed up, arms alternated over ``--rounds`` rounds, median
reported (docs/PROFILING.md).  Prints a markdown table; ``--out`` writes the bare table to a file.  ``--alt-lib``
adds the fragment kernels of a second build of the library as ALT arms (A/B of a kernel variant in one process).

    python scripts/stream_outer_bench.py --model llama_150m.json --out stream_outer_table.md
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
from nanodiloco_amd.ops import _ext  # noqa: E402
from nanodiloco_amd.parallel.fragments import plan_fragments  # noqa: E402

WIRE = {"f32": torch.float32, "bf16": torch.bfloat16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama_150m.json")
    ap.add_argument("--fragments", default="1,4")
    ap.add_argument("--pattern", default="strided")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--alt-lib", default=None,
                    help="another build of the kernel library (python -m nanodiloco_amd.csrc.build --rev WT --tag X): "
                         "its fragment kernels are timed as extra arms, interleaved with this build's")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_outer_bench.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    ops.set_backend("hip")
    cfg = resolve_llama_config(a.model)
    store = LlamaForCausalLM(cfg, "cpu").store
    n = store.numel
    g = torch.Generator().manual_seed(0)
    master = torch.randn(n, generator=g).to(dev)
    sync = master + 0.01 * torch.randn(n, generator=g).to(dev)
    mom = torch.zeros(n, device=dev)
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    wire = {k: torch.zeros(n, dtype=dt, device=dev) for k, dt in WIRE.items()}
    W, lr, mu = 8, 1e-9, 0.9
    arms = {}  # name -> (callable, bytes per element, baseline name or None, expected time ratio to the baseline)
    alt = _ext.load_library(a.alt_lib) if a.alt_lib else None

    def with_alt(fn):
        def run():
            with _ext.using(alt):
                fn()
        return run
    for P in (int(x) for x in a.fragments.split(",")):
        tables = [ops.SpanTable(sp, dev) for sp in plan_fragments(store, cfg.num_hidden_layers, P, a.pattern)]
        tot = [t.total for t in tables]
        tag = f"P={P} ({sum(len(t) for t in tables)} spans)"
        for wk, wbuf in wire.items():
            wb = wbuf.element_size()

            def contig_pg(wbuf=wbuf, tot=tot):
                for m in tot:
                    ops.pseudograd(sync[:m], master[:m], wbuf[:m])

            def frag_pg(wbuf=wbuf, tables=tables):
                for t in tables:
                    ops.frag_pseudograd(sync, master, t, wbuf)

            def contig_on(wbuf=wbuf, tot=tot):
                for m in tot:
                    ops.outer_nesterov(master[:m], sync[:m], wbuf[:m], mom[:m], shadow[:m], 1.0 / W, lr, mu, False)

            def frag_mix(alpha, wbuf=wbuf, tables=tables):
                for t in tables:
                    ops.frag_outer_mix(master, sync, wbuf, mom, shadow, t, 1.0 / W, lr, mu, False, alpha)

            base_pg, base_on = f"nd_pseudograd {wk} out, {tag} A", f"nd_outer_nesterov {wk} in, {tag} A"
            arms[base_pg] = (contig_pg, 8 + wb, None, 1.0)
            arms[base_pg + "'"] = (contig_pg, 8 + wb, base_pg, 1.0)
            arms[f"nd_frag_pseudograd {wk} out, {tag}"] = (frag_pg, 8 + wb, base_pg, 1.0)
            arms[base_on] = (contig_on, wb + 22, None, 1.0)
            arms[base_on + "'"] = (contig_on, wb + 22, base_on, 1.0)
            arms[f"nd_frag_outer_mix alpha=0 {wk} in, {tag}"] = (lambda f=frag_mix: f(0.0), wb + 22, base_on, 1.0)
            arms[f"nd_frag_outer_mix alpha=0.5 {wk} in, {tag}"] = (lambda f=frag_mix: f(0.5), wb + 26, base_on,
                                                                   (wb + 26) / (wb + 22))
            if alt is not None:
                arms[f"ALT nd_frag_pseudograd {wk} out, {tag}"] = (with_alt(frag_pg), 8 + wb, base_pg, 1.0)
                arms[f"ALT nd_frag_outer_mix alpha=0 {wk} in, {tag}"] = (with_alt(lambda f=frag_mix: f(0.0)), wb + 22,
                                                                         base_on, 1.0)
                arms[f"ALT nd_frag_outer_mix alpha=0.5 {wk} in, {tag}"] = (with_alt(lambda f=frag_mix: f(0.5)), wb + 26,
                                                                           base_on, (wb + 26) / (wb + 22))
    times = {k: [] for k in arms}
    for fn, *_ in arms.values():  # warm up every arm
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (fn, *_) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"flat size n = {n} elements ({a.model}, {a.pattern}), one sample = one launch per fragment over the whole "
             f"vector, {a.iters} samples per timing, {a.rounds} alternated rounds, {torch.cuda.get_device_name(0)}", "",
             "| arm | B / element | median ms | min..max ms | GB/s | time vs baseline A | expected |",
             "|---|---|---|---|---|---|---|"]
    for k, v in times.items():
        _, bpe, base, exp = arms[k]
        rel = f"{med[k] / med[base]:.3f}x" if base else "baseline"
        lines.append(f"| `{k}` | {bpe} | {med[k]:.4f} | {min(v):.4f}..{max(v):.4f} | {bpe * n / (med[k] * 1e-3) / 1e9:.0f} | "
                     f"{rel} | {'%.3fx' % exp if base else ''} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
