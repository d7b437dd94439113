"""Error feedback of the quantised outer transport on ONE GPU over the own RCCL communicator (run by
tests/test_qef_gpu.py in its own process, under a time limit, like tests/_qcomm_rccl_check.py).

Two ``Diloco`` outer steps with ``error_feedback=True`` and every collective forced on.  Step 1 starts from zero
residuals, so it must equal the stateless run bit for bit; step 2 must equal, bit for bit, a manual composition of
``ops.pseudograd_q_ef -> ops.qreduce_ef -> ops.outer_nesterov_q`` on cloned buffers (with one rank the all-to-all
and the all-gather are the identity).  ``gloo`` as the first argument rehearses the script on CPU."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanodiloco_amd import ops  # noqa: E402
from nanodiloco_amd.config import LlamaConfig  # noqa: E402
from nanodiloco_amd.models import LlamaForCausalLM  # noqa: E402
from nanodiloco_amd.ops import qcomm  # noqa: E402
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov  # noqa: E402
from nanodiloco_amd.parallel.diloco import Diloco  # noqa: E402
from nanodiloco_amd.parallel.dist import destroy_distributed, init_distributed  # noqa: E402

BACKEND = sys.argv[1] if len(sys.argv) > 1 else "nccl"
CPU = BACKEND == "gloo"
CFG = dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_hidden_layers=3, vocab_size=1000,
           rms_norm_eps=1e-5)
LR, MU = 0.7, 0.9


def check(cond, what):
    if not cond:
        raise SystemExit(f"FAIL: {what}")
    print(f"ok: {what}", flush=True)


def make(env, comm, ef):
    model = LlamaForCausalLM(LlamaConfig(**CFG), env.device, torch.float32 if CPU else torch.bfloat16).init_weights(7)
    dl = Diloco(model, FlatAdamW(model.store, lr=1e-3), FlatOuterNesterov(model.store, lr=LR, momentum=MU),
                warmup_steps=1, total_steps=100, inner_steps=2, env=env, comm_dtype=comm, bucket_mb=0.25,
                error_feedback=ef)
    return model, dl


def main():
    env = init_distributed(BACKEND, device="cpu" if CPU else None, force_pg=True)
    dev = env.device
    check(dist.is_initialized() and env.force_collectives, f"one-rank {BACKEND} group, collectives forced on")
    n = LlamaForCausalLM(LlamaConfig(**CFG), "cpu").store.numel
    drifts = [(0.01 * torch.randn(n, generator=torch.Generator().manual_seed(3 + s))).to(dev) for s in range(2)]
    for comm in ("int8", "int4"):
        bits = int(comm[3:])
        m0, d0 = make(env, comm, False)
        m1, d1 = make(env, comm, True)
        check(d1.qef_send.numel() == n and d1.qef_reduce.numel() == sum(bk.c for bk in d1.transport._qplan)
              and len(d1.transport._qplan) > 1, f"{comm}: residual buffers cover the span and one chunk per bucket")
        for m, d in ((m0, d0), (m1, d1)):
            m.store.master.add_(drifts[0])
            d.outer_step()
        check(torch.equal(m0.store.master, m1.store.master) and torch.equal(d0.sync, d1.sync)
              and torch.equal(m0.store.shadow, m1.store.shadow),
              f"{comm}: step 1 (zero residuals) == the stateless step, bitwise")
        check(bool((d1.qef_send != 0).any()), f"{comm}: step 1 left a sender residual")
        check(d1.bytes_per_outer_step == d0.bytes_per_outer_step
              and d1.buckets_per_outer_step == d0.buckets_per_outer_step, f"{comm}: same bytes and buckets")
        # ---- step 2: Diloco against the ops composed by hand on clones
        st, opt = m1.store, d1.outer_optimizer
        st.master.add_(drifts[1])
        master, sync, mom = st.master.clone(), d1.sync.clone(), opt.momentum_buffer.clone()
        shadow = st.shadow.clone() if st.shadow.data_ptr() != st.master.data_ptr() else None
        e1, e2 = d1.qef_send.clone(), d1.qef_reduce.clone()
        off = 0
        for bk in d1.transport._qplan:
            pb = qcomm.chunk_bytes(bk.c, bits)
            send, red = (torch.zeros(pb, dtype=torch.uint8, device=dev) for _ in range(2))
            ops.pseudograd_q_ef(sync[bk.x:bk.y], master[bk.x:bk.y], e1[bk.x:bk.y], send, 1, bk.c, bits)
            ops.qreduce_ef(send, 1, bk.c, bits, e2[off:off + bk.c], red)
            ops.outer_nesterov_q(master[bk.x:bk.y], sync[bk.x:bk.y], red, 1, bk.c, bits, mom[bk.x:bk.y],
                                 shadow[bk.x:bk.y] if shadow is not None else None, 1.0, LR, MU, False)
            off += bk.c
        d1.outer_step()
        if not CPU:
            torch.cuda.synchronize()
        check(torch.equal(st.master, master) and torch.equal(d1.sync, sync)
              and torch.equal(opt.momentum_buffer, mom), f"{comm}: step 2 == the composed ops, bitwise")
        check(shadow is None or torch.equal(st.shadow, shadow), f"{comm}: step 2 shadow")
        check(torch.equal(d1.qef_send, e1) and torch.equal(d1.qef_reduce, e2), f"{comm}: step 2 residuals")
        # and the residual did something: the stateless run's second step differs
        m0.store.master.add_(drifts[1])
        d0.outer_step()
        check(not torch.equal(m0.store.master, st.master), f"{comm}: step 2 differs from the stateless step")
        if not CPU:
            check(d1.outer_comm.impl == "rccl", f"{comm}: own RCCL communicator")
    if not CPU:
        from nanodiloco_amd.parallel import rccl
        for c in list(rccl._COMMS.values()):
            rc = rccl.lib().nd_comm_destroy2(c._h, 0)
            c._h = None
            check(rc == 0, f"communicator {c.key} destroyed cleanly (code {rc})")
        rccl._COMMS.clear()
    destroy_distributed()
    print("QEF_RCCL_CHECK_PASSED", flush=True)


if __name__ == "__main__":
    main()
