"""Low-rank outer transport on ONE GPU over the own RCCL communicator (run by tests/test_lowrank_gpu.py in its own
process, under a time limit; a one-rank process group must not leak into the other tests).

A one-rank ``nccl`` group with every collective forced on runs the real code: the bucketed all-reduce of both wire
buffers and whole ``Diloco`` outer steps with ``lowrank``.  With one rank the all-reduce is the identity, so the steps
must equal, bit for bit, the same steps over torch's ProcessGroupNCCL (``comm_impl="c10d"``) and the four ops called
by hand.  ``gloo`` as the first argument runs what does not need a GPU on CPU (a rehearsal of the script itself)."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.config import LlamaConfig  # noqa: E402
from nanodiloco_amd.models import LlamaForCausalLM  # noqa: E402
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov  # noqa: E402
from nanodiloco_amd.parallel.comm import plan_buckets  # noqa: E402
from nanodiloco_amd.parallel.diloco import Diloco  # noqa: E402
from nanodiloco_amd.parallel.dist import DistEnv, destroy_distributed, init_distributed  # noqa: E402
from tests._lowrank_checks import TINY, covered  # noqa: E402

BACKEND = sys.argv[1] if len(sys.argv) > 1 else "nccl"
CPU = BACKEND == "gloo"
BUCKET_MB = 0.01  # several buckets per round
LR, MU = 0.7, 0.9
R = 8


def sync():
    if not CPU:
        torch.cuda.synchronize()


def check(cond, what):
    if not cond:
        raise SystemExit(f"FAIL: {what}")
    print(f"ok: {what}", flush=True)


def outer_run(env, drift, steps=2):
    model = LlamaForCausalLM(LlamaConfig(**TINY), env.device, torch.float32 if CPU else torch.bfloat16).init_weights(7)
    dl = Diloco(model, FlatAdamW(model.store, lr=1e-3), FlatOuterNesterov(model.store, lr=LR, momentum=MU),
                warmup_steps=1, total_steps=100, inner_steps=2, env=env, comm_dtype=torch.float32, bucket_mb=BUCKET_MB,
                lowrank=R)
    rc = dl.outer_comm.rccl
    calls0 = rc.stats()["calls"] if rc is not None else 0
    start = model.store.master.clone()
    for s in range(steps):
        model.store.master.add_(drift, alpha=1.0 / (s + 1))
        dl.outer_step(phases=(s == steps - 1))
    sync()
    grew = rc.stats()["calls"] - calls0 if rc is not None else 0
    return start, model.store.master.clone(), dl.sync.clone(), model.store.shadow.clone(), dl, grew


def by_hand(start, drift, plan, steps=2):
    """The same steps through the four ops, no communicator."""
    dev = start.device
    theta, mom, e = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
    q0 = plan.init_q().to(dev)
    q = q0.clone()
    w1, w2 = (torch.zeros(n, device=dev) for n in ops.lowrank_wire_elems(plan))
    for s in range(steps):
        local = theta.clone().add_(drift, alpha=1.0 / (s + 1))
        ops.lowrank_project(theta, local, e, q, w1, plan)
        ops.lowrank_orthonormalize(w1, plan)
        ops.lowrank_backproject(e, w1, w2, plan)
        ops.outer_nesterov_lowrank(local, theta, e, w1, w2, q, q0, mom, None, plan, 1.0, LR, MU, s == 0)
    return theta, e, q


def main():
    env = init_distributed(BACKEND, device="cpu" if CPU else None, force_pg=True)
    dev = env.device
    check(dist.is_initialized() and env.force_collectives, f"one-rank {BACKEND} group, collectives forced on")
    if not CPU:
        check(env.comm_impl == "rccl", f"own RCCL communicator selected ({env.comm_impl})")
    cc = env if CPU else DistEnv(device=dev, backend="nccl", force_collectives=True, comm_impl="c10d")
    n = LlamaForCausalLM(LlamaConfig(**TINY), "cpu").store.numel
    drift = 0.01 * torch.randn(n, generator=torch.Generator().manual_seed(3))
    mask, _ = covered(ops.LowRankPlan.from_store(LlamaForCausalLM(LlamaConfig(**TINY), "cpu").store, R), n)
    drift = (drift * torch.from_numpy(mask)).to(dev)  # the padding between tensors never moves, and no table row covers it
    start, m_r, s_r, sh_r, dl_r, grew = outer_run(env, drift)
    plan = dl_r.transport.plan
    w1, w2 = ops.lowrank_wire_elems(plan)
    bb = dl_r.outer_comm.bucket_bytes
    nb = len(plan_buckets(0, w1, 4, bb)) + len(plan_buckets(0, w2, 4, bb))
    check(dl_r.buckets_per_outer_step == nb > 2 and dl_r.outer_comm.stats.calls == 2 * nb,
          f"{nb} buckets over the two rounds, one all-reduce per bucket and step")
    if not CPU:
        check(dl_r.outer_comm.impl == "rccl" and grew == 2 * nb,
              f"rccl_calls grew by one collective per bucket and outer step ({grew})")
    check(dl_r.bytes_per_outer_step == 4 * (w1 + w2) > 0, f"wire bytes reported ({dl_r.bytes_per_outer_step})")
    _, m_c, s_c, sh_c, dl_c, _ = outer_run(cc, drift)
    check(CPU or dl_c.outer_comm.impl == "c10d", "the same steps over c10d")
    check(torch.equal(m_r, m_c) and torch.equal(s_r, s_c) and torch.equal(sh_r, sh_c)
          and torch.equal(dl_r.lowrank_residual, dl_c.lowrank_residual) and torch.equal(dl_r.lowrank_q, dl_c.lowrank_q),
          "own RCCL == c10d, bitwise")
    check(torch.equal(m_r, s_r) and torch.equal(sh_r, m_r.to(sh_r.dtype)), "master == sync, shadow = cast(master)")
    want, want_e, want_q = by_hand(start, drift, plan)
    check(torch.equal(m_r, want) and torch.equal(dl_r.lowrank_residual, want_e) and torch.equal(dl_r.lowrank_q, want_q),
          "two steps == the four ops by hand, bitwise")
    check(bool((dl_r.lowrank_residual != 0).any()) and bool(torch.isfinite(m_r).all()), "something is still owed")
    ph = dl_r.outer_phase_ms()
    check(CPU and ph == {} or set(ph) == {"pseudograd_ms", "allreduce_ms", "outer_update_ms"}
          and all(v >= 0 for v in ph.values()), f"outer phase spans {ph}")
    if not CPU:
        from nanodiloco_amd.parallel import rccl
        for c in list(rccl._COMMS.values()):  # a clean destroy: the drain and ncclCommDestroy report no error
            rc = rccl.lib().nd_comm_destroy2(c._h, 0)
            c._h = None
            check(rc == 0, f"communicator {c.key} destroyed cleanly (code {rc})")
        rccl._COMMS.clear()
    destroy_distributed()
    print("LOWRANK_RCCL_CHECK_PASSED", flush=True)


if __name__ == "__main__":
    main()
