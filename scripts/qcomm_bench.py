#!/usr/bin/env python
"""Device time of the quantised-transport kernels (csrc/qcomm.hip) at a model's flat size, interleaved in one
process with the kernels they stand beside: ``nd_pseudograd`` (bf16 out) and ``nd_outer_nesterov`` (bf16 in).

All are HBM streams, so the figure of merit is achieved bytes/s over the bytes each kernel MUST move
(computed from the shapes below), and the expectation is parity with the baselines' bytes/s.  HIP events
around ``--iters`` back-to-back launches, every arm warmed up, arms alternated over ``--rounds`` rounds, median
reported (docs/PROFILING.md).  The error-feedback kernels (``nd_pseudograd_q_ef``, ``nd_qreduce_ef``) stand next
to their stateless siblings and are compared with them: they move the residual in and out on top, 4 + 4 bytes per
element (16 instead of 8 bytes of fp32 per element for the quantiser; both in addition to the wire bytes).  Prints a markdown table; ``--out`` also writes the bare table to a file of its
own (profiles/qcomm_kernels.md is hand-written around a copy of it: paste the table there, do not point
``--out`` at it).

    python scripts/qcomm_bench.py --model llama_150m.json --out qcomm_table.md
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
from nanodiloco_amd.ops import qcomm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama_150m.json")
    ap.add_argument("--workers", type=int, default=8, help="W of the nd_qreduce arm")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qcomm_bench.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    ops.set_backend("hip")
    n = LlamaForCausalLM(resolve_llama_config(a.model), "cpu").store.numel
    W = a.workers
    g = torch.Generator().manual_seed(0)
    master = torch.randn(n, generator=g).to(dev)
    sync = master + 0.01 * torch.randn(n, generator=g).to(dev)
    mom = torch.zeros(n, device=dev)
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    delta_bf16 = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    resid1 = torch.zeros(n, device=dev)  # error-feedback residuals: they evolve over the launches, the bytes do not
    arms = {}  # name -> (callable, bytes it must move, baseline name or None)
    arms["nd_pseudograd (bf16 out)"] = (lambda: ops.pseudograd(sync, master, delta_bf16), 8 * n + 2 * n, None)
    arms["nd_outer_nesterov (bf16 in)"] = (
        lambda: ops.outer_nesterov(master, sync, delta_bf16, mom, shadow, 1.0 / W, 1e-9, 0.9, False), 2 * n + 8 * n + 14 * n, None)
    for bits in (8, 4):
        c1 = qcomm.chunk_elems(n, 1)
        wire = torch.zeros(qcomm.chunk_bytes(c1, bits), dtype=torch.uint8, device=dev)
        wb = wire.numel()
        arms[f"nd_pseudograd_q int{bits}"] = (
            lambda wire=wire, c1=c1, bits=bits: ops.pseudograd_q(sync, master, wire, 1, c1, bits), 8 * n + wb,
            "nd_pseudograd (bf16 out)")
        arms[f"nd_pseudograd_q_ef int{bits}"] = (
            lambda wire=wire, c1=c1, bits=bits: ops.pseudograd_q_ef(sync, master, resid1, wire, 1, c1, bits), 16 * n + wb,
            f"nd_pseudograd_q int{bits}")
        cw = qcomm.chunk_elems(n, W)  # the chunk one worker owns; it receives W of them
        pb = qcomm.chunk_bytes(cw, bits)
        recv = torch.zeros(W * pb, dtype=torch.uint8, device=dev)
        ops.pseudograd_q(sync[:cw], master[:cw], recv[:pb], 1, cw, bits)  # real codes, the same from every worker
        for r in range(1, W):
            recv[r * pb:(r + 1) * pb] = recv[:pb]
        red = torch.zeros(pb, dtype=torch.uint8, device=dev)
        arms[f"nd_qreduce int{bits} (W = {W})"] = (
            lambda recv=recv, cw=cw, bits=bits, red=red: ops.qreduce(recv, W, cw, bits, red), recv.numel() + red.numel(),
            "nd_pseudograd (bf16 out)")
        resid2 = torch.zeros(cw, device=dev)
        arms[f"nd_qreduce_ef int{bits} (W = {W})"] = (
            lambda recv=recv, cw=cw, bits=bits, red=red, resid2=resid2: ops.qreduce_ef(recv, W, cw, bits, resid2, red),
            recv.numel() + red.numel() + 8 * cw, f"nd_qreduce int{bits} (W = {W})")
        arms[f"nd_outer_nesterov_q int{bits}"] = (
            lambda wire=wire, c1=c1, bits=bits: ops.outer_nesterov_q(master, sync, wire, 1, c1, bits, mom, shadow, 1.0 / W,
                                                                     1e-9, 0.9, False), wb + 8 * n + 14 * n,
            "nd_outer_nesterov (bf16 in)")
    times = {k: [] for k in arms}
    for fn, _, _ in arms.values():  # warm up every arm
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (fn, _, _) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters)
    rate = {k: arms[k][1] / (statistics.median(v) * 1e-3) for k, v in times.items()}
    lines = [f"flat size n = {n} elements ({a.model}), {a.iters} launches per sample, {a.rounds} alternated rounds, "
             f"{torch.cuda.get_device_name(0)}", "",
             "| kernel | bytes moved (MB) | median ms | min..max ms | GB/s | vs baseline |", "|---|---|---|---|---|---|"]
    for k, v in times.items():
        base = arms[k][2]
        rel = f"{rate[k] / rate[base]:.2f}x of {base}" if base else "baseline"
        lines.append(f"| `{k}` | {arms[k][1] / 1e6:.1f} | {statistics.median(v):.4f} | {min(v):.4f}..{max(v):.4f} | "
                     f"{rate[k] / 1e9:.0f} | {rel} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
