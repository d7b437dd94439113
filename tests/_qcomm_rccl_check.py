"""Quantised outer transport on ONE GPU over the own RCCL communicator (run by tests/test_qcomm_gpu.py in
its own process, under a time limit; a one-rank process group must not leak into the other tests).

A one-rank ``nccl`` group with every collective forced on runs the real code: ``nd_comm_all_to_all`` (a self
copy through ncclSend / ncclRecv in one group), the in-place all-gather of the wire buffer, and a whole
``Diloco`` outer step with int8 and int4 transport.  With one rank the exchange is the identity, so the step
must equal, bit for bit, the same step over torch's ProcessGroupNCCL (``comm_impl="c10d"``), and lie within
the format's error bound of the fp32-transport step.  ``gloo`` as the first argument runs what does not need
a GPU on CPU (a rehearsal of the script itself)."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanodiloco_amd.config import LlamaConfig  # noqa: E402
from nanodiloco_amd.models import LlamaForCausalLM  # noqa: E402
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov  # noqa: E402
from nanodiloco_amd.parallel.comm import FlatCommunicator  # noqa: E402
from nanodiloco_amd.parallel.diloco import Diloco  # noqa: E402
from nanodiloco_amd.parallel.dist import DistEnv, destroy_distributed, init_distributed  # noqa: E402

BACKEND = sys.argv[1] if len(sys.argv) > 1 else "nccl"
CPU = BACKEND == "gloo"
CFG = dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_hidden_layers=3, vocab_size=1000,
           rms_norm_eps=1e-5)
LR, MU = 0.7, 0.9


def sync():
    if not CPU:
        torch.cuda.synchronize()


def check(cond, what):
    if not cond:
        raise SystemExit(f"FAIL: {what}")
    print(f"ok: {what}", flush=True)


def outer_run(env, comm_dtype, drift, steps=2):
    """`steps` outer steps of a small Llama whose weights moved by `drift` before each (no inner steps).
    Returns master, sync, shadow, the Diloco and how many collectives the own communicator issued for them."""
    model = LlamaForCausalLM(LlamaConfig(**CFG), env.device, torch.float32 if CPU else torch.bfloat16).init_weights(7)
    dl = Diloco(model, FlatAdamW(model.store, lr=1e-3), FlatOuterNesterov(model.store, lr=LR, momentum=MU),
                warmup_steps=1, total_steps=100, inner_steps=2, env=env, comm_dtype=comm_dtype, bucket_mb=0.25)
    rc = dl.outer_comm.rccl
    calls0 = rc.stats()["calls"] if rc is not None else 0
    for s in range(steps):
        model.store.master.add_(drift, alpha=1.0 / (s + 1))
        dl.outer_step(phases=(s == steps - 1))
    sync()
    grew = rc.stats()["calls"] - calls0 if rc is not None else 0
    return model.store.master.clone(), dl.sync.clone(), model.store.shadow.clone(), dl, grew


def main():
    env = init_distributed(BACKEND, device="cpu" if CPU else None, force_pg=True)
    dev = env.device
    check(dist.is_initialized() and env.force_collectives, f"one-rank {BACKEND} group, collectives forced on")

    # ---- all_to_all + all-gather of a uint8 wire buffer: one rank = a self copy
    if CPU:
        oc = FlatCommunicator(None, 1, bucket_mb=1.0, force=True)
    else:
        check(env.comm_impl == "rccl", f"own RCCL communicator selected ({env.comm_impl})")
        oc = FlatCommunicator(None, 1, bucket_mb=1.0, force=True, impl="rccl", device=dev, timeout_s=120.0)
        check(oc.rccl is not None and oc.rccl.size == 1, "own communicator initialised")
    calls0 = oc.rccl.stats()["calls"] if oc.rccl is not None else 0
    send = torch.randint(0, 256, ((1 << 20) + 4,), dtype=torch.uint8, device=dev)
    recv = torch.zeros_like(send)
    w = oc.all_to_all_async(send, recv)
    w.wait()
    same = torch.equal(send, recv)  # consumer on the compute stream, ordered after the wait only
    sync()
    check(same, "all_to_all over one rank copies send to recv")
    check(oc.stats.calls == 1 and oc.stats.bytes == send.numel(), "all_to_all counted in the FlatCommunicator's stats")
    if oc.rccl is not None:
        check(w.is_completed() and oc.rccl.error() == 0 and oc.rccl.stats()["calls"] == calls0 + 1,
              "all_to_all is one collective of the own communicator, completed without error")
    g = oc.all_gather_async(recv, 0)
    g.wait()
    sync()
    check(torch.equal(send, recv) and oc.stats.calls == 2, "in-place all-gather of a uint8 wire buffer")

    # ---- whole Diloco outer steps: own RCCL == c10d bitwise, within the format's bound of fp32 transport
    cc = env if CPU else DistEnv(device=dev, backend="nccl", force_collectives=True, comm_impl="c10d")
    n = LlamaForCausalLM(LlamaConfig(**CFG), "cpu").store.numel
    drift = (0.01 * torch.randn(n, generator=torch.Generator().manual_seed(3))).to(dev)
    m_f, _, _, _, _ = outer_run(env, torch.float32, drift, steps=1)
    for comm, qmax in (("int8", 127.0), ("int4", 7.0)):
        m_r, s_r, sh_r, dl_r, grew = outer_run(env, comm, drift)
        nb = dl_r.buckets_per_outer_step
        check(nb > 1 and dl_r.outer_comm.stats.calls == 2 * 2 * nb,
              f"{comm}: {nb} buckets, two collectives per bucket and outer step")
        if not CPU:
            check(dl_r.outer_comm.impl == "rccl" and grew == 2 * 2 * nb,
                  f"{comm}: rccl_calls grew by two collectives per bucket and outer step ({grew})")
        m_c, s_c, sh_c, dl_c, _ = outer_run(cc, comm, drift)
        check(CPU or dl_c.outer_comm.impl == "c10d", f"{comm}: the same steps over c10d")
        check(torch.equal(m_r, m_c) and torch.equal(s_r, s_c) and torch.equal(sh_r, sh_c),
              f"{comm}: own RCCL == c10d, bitwise (master, sync, shadow)")
        check(torch.equal(m_r, s_r) and torch.equal(sh_r, m_r.to(sh_r.dtype)), f"{comm}: master == sync, shadow = cast(master)")
        ph = dl_r.outer_phase_ms()
        check(CPU and ph == {} or set(ph) == {"pseudograd_ms", "allreduce_ms", "outer_update_ms"}
              and all(v >= 0 for v in ph.values()), f"{comm}: outer phase spans {ph}")
        # one step against fp32 transport: W = 1, so two roundings of at most scale/2 each, scale <= amax/QMAX,
        # times lr * (1 + mu); max|drift| over the whole vector bounds every block's amax
        m_1, _, _, dl_1, _ = outer_run(env, comm, drift, steps=1)
        amax = drift.abs().max().item() * (1 + 2.0 ** -20)
        bound = (amax / qmax / 2 + amax / qmax / 2) * LR * (1 + MU)
        err = (m_1 - m_f).abs().max().item()
        check(0 < err <= bound, f"{comm}: |quantised - fp32 transport| = {err:.3e} <= {bound:.3e}")
        check(dl_1.bytes_per_outer_step == sum(bk.send.numel() for bk in dl_1.transport._qplan) > 0,
              f"{comm}: wire bytes reported")
    if not CPU:
        from nanodiloco_amd.parallel import rccl
        for c in list(rccl._COMMS.values()):  # a clean destroy: the drain and ncclCommDestroy report no error
            rc = rccl.lib().nd_comm_destroy2(c._h, 0)
            c._h = None
            check(rc == 0, f"communicator {c.key} destroyed cleanly (code {rc})")
        rccl._COMMS.clear()
    destroy_distributed()
    print("QCOMM_RCCL_CHECK_PASSED", flush=True)


if __name__ == "__main__":
    main()
