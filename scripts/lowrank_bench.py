#!/usr/bin/env python
"""Device time of the low-rank transport's outer step (``LowRankTransport``, csrc/lowrank_comm.hip) at a model's
flat size next to the dense transport's (``DenseTransport``: ``nd_pseudograd`` + ``nd_outer_nesterov``), one worker,
all in one process.

Arms: the whole ``Diloco.outer_step()`` of a dense run (timed twice, A and A': their ratio is the session's spread)
and of a low-rank run per ``--ranks`` entry, alternated over ``--rounds`` rounds after a warm-up, HIP events around every
step, median reported.  Before every step the master is moved by the same drift (outside the timed span), so the
kernels see a real pseudo-gradient.  Then the four low-rank kernels one by one at every rank, with the bytes each has
to move, so a kernel far below the copy rate can be named.  ``--rehearse`` runs the same code on the CPU at a tiny
model to check the script; its numbers are host times of the PyTorch path and mean nothing.

    python scripts/lowrank_bench.py --model llama_150m.json --out profiles/lowrank.md
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.config import resolve_llama_config  # noqa: E402
from nanodiloco_amd.models import LlamaForCausalLM  # noqa: E402
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov  # noqa: E402
from nanodiloco_amd.parallel.diloco import Diloco  # noqa: E402
from nanodiloco_amd.parallel.dist import DistEnv  # noqa: E402


class Clock:
    def __init__(self, cuda):
        self.cuda = cuda

    def time(self, fn):
        """milliseconds of fn() on the device (HIP events), or on the host in a rehearsal"""
        if self.cuda:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama_150m.json")
    ap.add_argument("--ranks", default="8,32")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cuda = torch.cuda.is_available() and not a.rehearse
    if not cuda and not a.rehearse:
        raise SystemExit("lowrank_bench.py measures on the GPU; none found (--rehearse checks the script on the CPU)")
    dev = torch.device("cuda:0" if cuda else "cpu")
    if cuda:
        ops.set_backend("hip")
    clock = Clock(cuda)
    cfg = resolve_llama_config(a.model)
    ranks = [int(r) for r in a.ranks.split(",")]

    def make(rank):
        m = LlamaForCausalLM(cfg, dev, torch.bfloat16 if cuda else torch.float32).init_weights(0)
        return m, Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store, lr=1e-9, momentum=0.9), 1, 1000, 100,
                         env=DistEnv(device=dev), comm_dtype=torch.float32, lowrank=rank)

    arms = {"dense A": make(0), "dense A'": make(0)}
    for r in ranks:
        arms[f"low-rank R={r}"] = make(r)
    n = arms["dense A"][0].store.numel
    drift = (1e-3 * torch.randn(n, generator=torch.Generator().manual_seed(0))).to(dev)

    def step(arm):
        m, dl = arms[arm]
        m.store.master.add_(drift)
        return clock.time(dl.outer_step)

    for arm in arms:  # warm up: code objects, the first step's `first` path
        for _ in range(2):
            step(arm)
    times = {arm: [] for arm in arms}
    for _ in range(a.rounds):
        for arm in arms:
            times[arm].append(statistics.mean(step(arm) for _ in range(a.iters)))
    med = {arm: statistics.median(v) for arm, v in times.items()}
    where = torch.cuda.get_device_name(0) if cuda else "CPU REHEARSAL: host times of the PyTorch path, not a measurement"
    lines = ["# Low-rank transport (`csrc/lowrank_comm.hip`): what the outer step costs", "",
             f"`scripts/lowrank_bench.py`: flat size n = {n} elements ({a.model}), one worker, one sample = one "
             f"`Diloco.outer_step()`, {a.iters} samples per timing, {a.rounds} alternated rounds, median; HIP events; "
             f"{where}.", "",
             "| arm | wire bytes / step | median ms | min..max ms | vs dense A |", "|---|---|---|---|---|"]
    for arm, v in times.items():
        lines.append(f"| {arm} | {arms[arm][1].transport.bytes_per_step} | {med[arm]:.4f} | {min(v):.4f}..{max(v):.4f} | "
                     f"{med[arm] / med['dense A']:.3f}x |")
    # ---- the kernels one by one
    lines += ["", "| kernel | rank | bytes moved | median ms | GB/s |", "|---|---|---|---|---|"]
    m0, d0 = arms["dense A"]
    delta, opt0 = d0.transport.delta, d0.outer_optimizer
    dense_ops = {
        "nd_pseudograd": (lambda: ops.pseudograd(d0.sync, m0.store.master, delta), 12 * n),
        "nd_outer_nesterov": (lambda: ops.outer_nesterov(m0.store.master, d0.sync, delta, opt0.momentum_buffer,
                                                         m0.store.separate_shadow, 1.0, 1e-9, 0.9, False),
                              (26 if m0.store.separate_shadow is not None else 24) * n),
    }
    for name, (fn, nbytes) in dense_ops.items():
        fn()
        t = statistics.median(clock.time(fn) for _ in range(a.iters * a.rounds))
        lines.append(f"| `{name}` | - | {nbytes} | {t:.4f} | {nbytes / (t * 1e-3) / 1e9:.0f} |")
    for r in ranks:
        m, dl = arms[f"low-rank R={r}"]
        t, plan, st, opt = dl.transport, dl.transport.plan, m.store, dl.outer_optimizer
        c, dn, w1, w2 = plan.compressed_elems, plan.dense_total, plan.wire1_elems, plan.wire2_elems
        sh = st.separate_shadow
        kernels = {
            # sync, master, e in; e out; Q in (once per matrix); wire 1 out
            "nd_lowrank_project": (lambda: ops.lowrank_project(dl.sync, st.master, t.residual, t.q, t.wire1, plan),
                                   16 * c + 8 * dn + 4 * (w1 + w2)),
            # column c is read and written once per earlier column and twice for its norms
            "nd_lowrank_orthonormalize": (lambda: ops.lowrank_orthonormalize(t.wire1, plan), 4 * (w1 - dn) * (r + 3)),
            "nd_lowrank_backproject": (lambda: ops.lowrank_backproject(t.residual, t.wire1, t.wire2, plan),
                                       4 * c + 4 * (w1 - dn) + 4 * w2),
            # e, momentum, sync in; e, momentum, sync, master (+ bf16 shadow) out; both factors in; Q out
            "nd_outer_nesterov_lowrank": (lambda: ops.outer_nesterov_lowrank(
                st.master, dl.sync, t.residual, t.wire1, t.wire2, t.q, t.q0, opt.momentum_buffer, sh, plan, 1.0, 1e-9,
                0.9, False), (30 if sh is not None else 28) * c + (26 if sh is not None else 24) * dn + 4 * w1 + 12 * w2),
        }
        st.master.add_(drift)
        for name, (fn, nbytes) in kernels.items():
            fn()
            ts = statistics.median(clock.time(fn) for _ in range(a.iters * a.rounds))
            lines.append(f"| `{name}` | {r} | {nbytes} | {ts:.4f} | {nbytes / (ts * 1e-3) / 1e9:.0f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
