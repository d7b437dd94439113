"""Top-k sparse outer transport on ONE GPU over the own RCCL communicator (run by tests/test_topk_gpu.py in its own
process, under a time limit; a one-rank process group must not leak into the other tests).

A one-rank ``nccl`` group with every collective forced on runs the real code: the in-place all-gather of every
bucket's ``gath`` buffer and whole ``Diloco`` outer steps with ``topk``.  With one rank the gather is the identity,
so the steps must equal, bit for bit, the same steps over torch's ProcessGroupNCCL (``comm_impl="c10d"``) and the
in-test oracle's (tests/_topk_oracle.py) fed to ``nd_outer_nesterov``.  ``gloo`` as the first argument runs what does
not need a GPU on CPU (a rehearsal of the script itself)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.config import LlamaConfig  # noqa: E402
from nanodiloco_amd.models import LlamaForCausalLM  # noqa: E402
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov  # noqa: E402
from nanodiloco_amd.parallel.diloco import Diloco  # noqa: E402
from nanodiloco_amd.parallel.dist import DistEnv, destroy_distributed, init_distributed  # noqa: E402
from tests import _topk_oracle as to  # noqa: E402

BACKEND = sys.argv[1] if len(sys.argv) > 1 else "nccl"
CPU = BACKEND == "gloo"
CFG = dict(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_hidden_layers=2, vocab_size=500,
           rms_norm_eps=1e-5)  # ~0.1k chunks: the oracle sorts every one in Python
BUCKET_MB = 0.01  # a few tens of chunks per bucket
LR, MU = 0.7, 0.9
K = 64


def sync():
    if not CPU:
        torch.cuda.synchronize()


def check(cond, what):
    if not cond:
        raise SystemExit(f"FAIL: {what}")
    print(f"ok: {what}", flush=True)


def outer_run(env, comm_dtype, drift, steps=2):
    model = LlamaForCausalLM(LlamaConfig(**CFG), env.device, torch.float32 if CPU else torch.bfloat16).init_weights(7)
    dl = Diloco(model, FlatAdamW(model.store, lr=1e-3), FlatOuterNesterov(model.store, lr=LR, momentum=MU),
                warmup_steps=1, total_steps=100, inner_steps=2, env=env, comm_dtype=comm_dtype, bucket_mb=BUCKET_MB, topk=K)
    rc = dl.outer_comm.rccl
    calls0 = rc.stats()["calls"] if rc is not None else 0
    start = model.store.master.clone()
    for s in range(steps):
        model.store.master.add_(drift, alpha=1.0 / (s + 1))
        dl.outer_step(phases=(s == steps - 1))
    sync()
    grew = rc.stats()["calls"] - calls0 if rc is not None else 0
    return start, model.store.master.clone(), dl.sync.clone(), model.store.shadow.clone(), dl, grew


def oracle_run(start, drift, bf16, steps=2):
    """The same steps through the oracle (one worker) and ``ops.outer_nesterov`` on the device under test."""
    dev = start.device
    theta, mom = start.clone(), torch.zeros_like(start)
    e = np.zeros(start.numel(), dtype=np.float32)
    for s in range(steps):
        local = theta.clone().add_(drift, alpha=1.0 / (s + 1))
        idx, val, e, _ = to.select(theta.cpu().numpy(), local.cpu().numpy(), e, K, bf16)
        dsum = torch.from_numpy(to.dense_sum([(idx, val)], start.numel())).to(dev)
        ops.outer_nesterov(local, theta, dsum, mom, None, 1.0, LR, MU, s == 0)
    return theta, torch.from_numpy(e).to(dev)


def main():
    env = init_distributed(BACKEND, device="cpu" if CPU else None, force_pg=True)
    dev = env.device
    check(dist.is_initialized() and env.force_collectives, f"one-rank {BACKEND} group, collectives forced on")
    if not CPU:
        check(env.comm_impl == "rccl", f"own RCCL communicator selected ({env.comm_impl})")
    cc = env if CPU else DistEnv(device=dev, backend="nccl", force_collectives=True, comm_impl="c10d")
    n = LlamaForCausalLM(LlamaConfig(**CFG), "cpu").store.numel
    drift = (0.01 * torch.randn(n, generator=torch.Generator().manual_seed(3))).to(dev)
    for comm in (torch.bfloat16, torch.float32):
        start, m_r, s_r, sh_r, dl_r, grew = outer_run(env, comm, drift)
        nb = dl_r.buckets_per_outer_step
        check(nb > 1 and dl_r.outer_comm.stats.calls == 2 * nb, f"{comm}: {nb} buckets, one all-gather per bucket and step")
        if not CPU:
            check(dl_r.outer_comm.impl == "rccl" and grew == 2 * nb,
                  f"{comm}: rccl_calls grew by one collective per bucket and outer step ({grew})")
        _, m_c, s_c, sh_c, dl_c, _ = outer_run(cc, comm, drift)
        check(CPU or dl_c.outer_comm.impl == "c10d", f"{comm}: the same steps over c10d")
        check(torch.equal(m_r, m_c) and torch.equal(s_r, s_c) and torch.equal(sh_r, sh_c)
              and torch.equal(dl_r.topk_residual, dl_c.topk_residual), f"{comm}: own RCCL == c10d, bitwise")
        check(torch.equal(m_r, s_r) and torch.equal(sh_r, m_r.to(sh_r.dtype)), f"{comm}: master == sync, shadow = cast(master)")
        want, want_e = oracle_run(start, drift, comm == torch.bfloat16)
        check(torch.equal(m_r, want) and torch.equal(dl_r.topk_residual, want_e), f"{comm}: two steps == the oracle's, bitwise")
        check(bool((dl_r.topk_residual != 0).any()), f"{comm}: something is still owed")
        ph = dl_r.outer_phase_ms()
        check(CPU and ph == {} or set(ph) == {"pseudograd_ms", "allreduce_ms", "outer_update_ms"}
              and all(v >= 0 for v in ph.values()), f"{comm}: outer phase spans {ph}")
        check(dl_r.bytes_per_outer_step == sum(ops.topk_slot_bytes(bk.y - bk.x, K, comm) for bk in dl_r.transport._plan) > 0,
              f"{comm}: wire bytes reported ({dl_r.bytes_per_outer_step})")
    if not CPU:
        from nanodiloco_amd.parallel import rccl
        for c in list(rccl._COMMS.values()):  # a clean destroy: the drain and ncclCommDestroy report no error
            rc = rccl.lib().nd_comm_destroy2(c._h, 0)
            c._h = None
            check(rc == 0, f"communicator {c.key} destroyed cleanly (code {rc})")
        rccl._COMMS.clear()
    destroy_distributed()
    print("TOPK_RCCL_CHECK_PASSED", flush=True)


if __name__ == "__main__":
    main()
