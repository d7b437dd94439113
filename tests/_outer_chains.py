"""The per-rank chains of the outer-step transports, written once and run on the CPU (the ``*_e2e_cpu.py`` files,
test_diloco_cpu.py, test_streaming_cpu.py: gloo, the PyTorch path of ``ops``) and with several workers sharing one
GPU (tests/test_transports_multiworker_gpu.py: gloo, the HIP kernels).

Every chain takes ``(rank, world, ..., device="cpu", dtype=torch.float32, env=None)``: ``device="cuda"`` forces the
HIP backend, builds the model on ``env.device`` in ``dtype`` (bf16: a separate bf16 shadow, fp32: the shadow is the
master) and moves the drifts there.  ``env``: a process group that already exists (several chains in one child).

On ``"cuda"`` selection and quantisation stay in the CPU oracles (tests/_topk_oracle.py, _qoracle.py, _qef_checks.py:
the kernel-level GPU tests hold those stages to them bit for bit) and the final update goes through
``ops.outer_nesterov`` on the device under test; on ``"cpu"`` the chains that compared with ``torch.optim.SGD`` still
do."""
import json
import os

import numpy as np
import torch
import torch.distributed as dist

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.optim import FlatAdamW, FlatOuterNesterov
from nanodiloco_amd.parallel.diloco import Diloco
from nanodiloco_amd.parallel.dist import init_distributed
from nanodiloco_amd.parallel.transports import LowRankTransport, TopKTransport
from nanodiloco_amd.utils.checkpoint import load_checkpoint, save_checkpoint

from . import _lowrank_checks as lchk
from . import _qef_checks as qchk
from . import _qoracle as qo
from . import _topk_checks as tchk
from . import _topk_oracle as to

TINY = dict(hidden_size=32, intermediate_size=64, num_attention_heads=2, num_hidden_layers=1, vocab_size=50,
            rms_norm_eps=1e-5)
TINY4 = dict(TINY, num_hidden_layers=4)
LR, MU = 0.7, 0.9
SIGMA = 0.01
QEF_STEPS = 3
TOPK_BUCKET = (3 * 2 * 64 * 4 + 3 * 32) / (1 << 20)  # slots of three chunks of k = 64 (bf16): two buckets of TINY
H = 8  # inner steps per round of the streaming chains


# ------------------------------------------------------------------------------------------------ plumbing
def setup(device, inner_dp=1, env=None):
    """The process group (gloo) and, on ``"cuda"``, the HIP backend: an op that met a CPU tensor would raise."""
    env = env or init_distributed("gloo", inner_dp=inner_dp)
    if device == "cuda":
        ops.set_backend("hip")
        assert env.device.type == "cuda"
    return env


def model(cfg, seed, env, device, dtype):
    if device == "cpu":
        return LlamaForCausalLM(LlamaConfig.from_dict(cfg)).init_weights(seed)
    return LlamaForCausalLM(LlamaConfig.from_dict(cfg), env.device, dtype).init_weights(seed)


def diloco(m, env, inner_steps=4, total=8, **kw):
    return Diloco(m, FlatAdamW(m.store, lr=1e-3), FlatOuterNesterov(m.store, lr=LR, momentum=MU), 2, total, inner_steps,
                  env=env, **kw)


def drift(n, step, worker):
    return SIGMA * torch.randn(n, generator=torch.Generator().manual_seed(100 * step + worker))


def check_step(dl, spans=None):
    """What every transport owes after an outer step: replicas bit-identical, master == sync and the bf16 shadow
    the cast of the master, bitwise (``spans``: only there, for a streaming fragment)."""
    st = dl.store
    dl.check_replicas(tol=0.0)
    cut = (lambda t: t) if spans is None else (lambda t: torch.cat([t[a:b] for a, b in spans]))
    sync = dl.sync.to(st.device)
    assert torch.equal(cut(st.master), cut(sync)), "master != sync"
    assert torch.equal(cut(st.shadow), cut(st.master).to(st.shadow.dtype)), "shadow != cast(master)"


class Nesterov:
    """The oracle's outer update of a span from its summed pseudo-gradient: ``torch.optim.SGD`` on the CPU (what the
    CPU chains always compared with), ``ops.outer_nesterov`` on the device under test on ``"cuda"`` (SGD's roundings
    need not be the kernel's)."""

    def __init__(self, theta, device):
        self.theta, self.cuda = theta, device == "cuda"
        self.mom = torch.zeros_like(theta)
        self.steps, self.sgd = {}, {}

    def step(self, x, y, dsum, inv_w):
        """``dsum``: fp32 on the CPU.  theta[x:y] takes the step."""
        n = self.steps[x, y] = self.steps.get((x, y), 0) + 1
        if self.cuda:
            ops.outer_nesterov(self.theta[x:y].clone(), self.theta[x:y], dsum.to(self.theta.device), self.mom[x:y], None,
                               inv_w, LR, MU, n == 1)
            return
        if (x, y) not in self.sgd:
            p = torch.nn.Parameter(self.theta[x:y].clone())
            self.sgd[x, y] = (p, torch.optim.SGD([p], lr=LR, momentum=MU, nesterov=True))
        p, sgd = self.sgd[x, y]
        p.grad = dsum * inv_w
        sgd.step()
        self.theta[x:y] = p.detach()


# ------------------------------------------------------------------------------------------------ top-k
def topk_mk(comm=torch.float32, topk=7, inner_dp=1, seed=7, env=None, device="cpu", dtype=torch.float32, **kw):
    env = setup(device, inner_dp, env)
    m = model(TINY, seed, env, device, dtype)
    return env, m, diloco(m, env, comm_dtype=comm, topk=topk, **kw)


def _topk_diagnosis(dl, theta, slots, resid=None):
    """For a failed comparison: where the master differs, and which gathered slot is not the oracle's bytes."""
    bad = (dl.store.master != theta).nonzero().flatten()
    out = {"differing": int(bad.numel()), "first": int(bad[0]) if bad.numel() else None,
           "last": int(bad[-1]) if bad.numel() else None, "sync==master": bool(torch.equal(dl.sync, dl.store.master))}
    if resid is not None:
        rb = (dl.topk_residual.cpu() != torch.from_numpy(resid)).nonzero().flatten()
        out["own residual differs at"] = (int(rb.numel()), int(rb[0]), int(rb[-1])) if rb.numel() else None
    if slots is not None:
        wrong = []
        for b, bk in enumerate(dl.transport._plan):
            c0, c1 = bk.x // to.CHUNK, -(-bk.y // to.CHUNK)
            for j, (idx, val) in enumerate(slots):
                want = torch.from_numpy(to.pack(idx[c0:c1], val[c0:c1]))
                if not torch.equal(bk.gath[j * bk.slot:(j + 1) * bk.slot].cpu(), want):
                    wrong.append((b, j))
        out["(bucket, worker) slots that differ from the oracle's"] = wrong
    return out


def topk_chain(rank, world, comm, k, inner_dp, bucket_mb, device="cpu", dtype=torch.float32, env=None):
    """Two outer steps, a fresh drift per step and worker.  The oracle selects for every worker and shard, carries
    each residual, sums the slots in worker order and feeds ``ops.outer_nesterov``; master, sync, momentum and this
    rank's residual must equal it bit for bit."""
    bf16 = comm == torch.bfloat16
    env, m, dl = topk_mk(comm, k, inner_dp=inner_dp, bucket_mb=bucket_mb, env=env, device=device, dtype=dtype)
    assert isinstance(dl.transport, TopKTransport)
    st = m.store
    dev = st.device
    w = env.num_workers
    shards = dl.shards
    calls0 = dl.outer_comm.stats.calls
    theta, mom = st.master.clone(), torch.zeros_like(st.master)
    e = [[np.zeros(y - x, dtype=np.float32) for _ in range(w)] for x, y in shards]
    a, b = dl.my_shard
    mine = shards.index((a, b))
    assert dl.bytes_per_outer_step == sum(ops.topk_slot_bytes(bk.y - bk.x, k, comm) for bk in dl.transport._plan)
    assert all(bk.x % to.CHUNK == 0 for bk in dl.transport._plan)
    if bucket_mb >= 1:
        assert dl.buckets_per_outer_step == 1 and dl.bytes_per_outer_step == ops.topk_slot_bytes(b - a, k, comm)
    else:
        assert dl.buckets_per_outer_step > 1
    for s in range(2):
        drifts = [drift(st.numel, s, j) for j in range(w)]  # every GPU of a worker drifts identically
        st.master.add_(drifts[env.worker].to(dev))
        before = theta.to("cpu", copy=True)  # the oracle selects from host copies: nothing it reads was ever a device buffer
        for i, (x, y) in enumerate(shards):
            slots = []
            for j in range(w):
                local = (before + drifts[j])[x:y].numpy()
                idx, val, e[i][j], _ = to.select(before[x:y].numpy(), local, e[i][j], k, bf16)
                slots.append((idx, val))
            dsum = torch.from_numpy(to.dense_sum(slots, y - x)).to(dev)
            ops.outer_nesterov(theta[x:y].clone(), theta[x:y], dsum, mom[x:y], None, 1.0 / w, LR, MU, s == 0)
        # the step's inputs are the oracle's, bit for bit (the drift reached the device whole)
        assert torch.equal(dl.sync.cpu(), before) and torch.equal(st.master.cpu(), before + drifts[env.worker])
        dl.outer_step()
        assert torch.equal(st.master, theta), (s, (st.master - theta).abs().max().item(),
                                               _topk_diagnosis(dl, theta, slots if len(shards) == 1 else None,
                                                               e[mine][env.worker]))
        assert torch.equal(dl.sync, theta)
        assert torch.equal(dl.outer_optimizer.momentum_buffer[a:b], mom[a:b])
        assert tchk.same_bits(dl.topk_residual, e[mine][env.worker])
        dl.check_replicas(tol=0.0)
        check_step(dl)
    assert dl.outer_comm.stats.calls - calls0 == 2 * dl.buckets_per_outer_step
    return bool((dl.topk_residual != 0).any())


# ------------------------------------------------------------------------------------------------ int8 / int4
def q_mk(comm, inner_dp=1, seed=7, env=None, ef=False, device="cpu", dtype=torch.float32, **kw):
    env = setup(device, inner_dp, env)
    m = model(TINY, seed, env, device, dtype)
    return env, m, diloco(m, env, comm_dtype=comm, error_feedback=ef, **kw)


def qef_chain(rank, world, comm, inner_dp, device="cpu", dtype=torch.float32, env=None, ef=True, steps=QEF_STEPS,
              bucket_mb=128.0):
    """``steps`` outer steps, a fresh drift per step and worker; the master must equal an in-test chain that carries
    e1 per worker and e2 per chunk through the oracle of tests/_qef_checks.py, bucket by bucket of the transport's
    plan, and feeds the outer update (:class:`Nesterov`).  ``ef=False``: the stateless transport, whose oracle is the
    same chain with both residuals dropped after every step."""
    bits = int(comm[3:])
    env, m, dl = q_mk(comm, inner_dp=inner_dp, env=env, ef=ef, device=device, dtype=dtype, bucket_mb=bucket_mb)
    st = m.store
    dev = st.device
    w = env.num_workers
    _, m0, dl0 = q_mk(comm, env=env, device=device, dtype=dtype, bucket_mb=bucket_mb)  # stateless, for step 1
    shards = dl.shards
    plan = [(bk.x, bk.y) for bk in dl.transport._qplan]  # the same cut of every shard: the shards are equal
    assert (len(plan) == 1) == (bucket_mb >= 1)
    nes = Nesterov(st.master.clone(), device)  # the oracle's theta_sync
    theta = nes.theta
    e1 = [[[torch.zeros(y - x) for _ in range(w)] for x, y in plan] for _ in shards]
    e2 = [[[torch.zeros(qo.chunk(y - x, w)) for _ in range(w)] for x, y in plan] for _ in shards]
    for s in range(steps):
        drifts = [drift(st.numel, s, k) for k in range(w)]  # every GPU of a worker drifts identically
        st.master.add_(drifts[env.worker].to(dev))
        base = theta.cpu().clone()
        for i, (sx, _) in enumerate(shards):
            for j, (bx, by) in enumerate(plan):
                x, y = sx + bx, sx + by
                stage1 = []
                for k in range(w):
                    oc, os_, e1[i][j][k] = qchk.oracle_stage1(base[x:y], base[x:y] + drifts[k][x:y], e1[i][j][k], w, bits)
                    stage1.append((oc, os_))
                out = []
                for k in range(w):  # chunk k is reduced by worker k, which keeps e2 for it
                    codes = torch.stack([q[0][k] for q in stage1])
                    scales = torch.stack([q[1][k] for q in stage1])
                    rc, rs, e2[i][j][k] = qchk.oracle_stage2(codes, scales, e2[i][j][k], bits)
                    out.append(qo.dequant(rc, rs).view(-1))
                nes.step(x, y, torch.cat(out)[: y - x], 1.0 / w)
                if not ef:
                    e1[i][j] = [torch.zeros_like(t) for t in e1[i][j]]
                    e2[i][j] = [torch.zeros_like(t) for t in e2[i][j]]
        dl.outer_step()
        diff = (st.master - theta).abs().max().item()
        print(f"{comm} W={w} inner_dp={inner_dp} ef={ef} step {s + 1}: max |master - oracle| = {diff:.3e}")
        assert torch.equal(st.master, theta), (s, diff)
        assert torch.equal(dl.sync, st.master)
        dl.check_replicas(tol=0.0)
        check_step(dl)
        a, b = dl.my_shard
        i = shards.index((a, b))
        if device == "cuda":
            assert torch.equal(dl.outer_optimizer.momentum_buffer[a:b], nes.mom[a:b])
        if ef:
            assert qchk.same_bits(dl.qef_send, torch.cat([e1[i][j][env.worker] for j in range(len(plan))]))
            assert qchk.same_bits(dl.qef_reduce, torch.cat([e2[i][j][env.worker] for j in range(len(plan))]))
        if s == 0:
            m0.store.master.add_(drifts[env.worker].to(dev))
            dl0.outer_step()
            assert torch.equal(m0.store.master, st.master), "step 1 (zero residuals) must equal the stateless step"
            assert dl.bytes_per_outer_step == dl0.bytes_per_outer_step
            assert dl.buckets_per_outer_step == dl0.buckets_per_outer_step == len(plan)
            if bucket_mb >= 1:
                assert dl.buckets_per_outer_step == 1
                c = qo.chunk(b - a, w)
                assert dl.bytes_per_outer_step == w * (c * bits // 8 + c // 256 * 4)
    return bool((dl.qef_send != 0).any()) if ef else True


def qef_several_buckets(rank, world):
    """Three workers, buckets of 4 x 3 x 256 elements and a shorter last one (the flat size is a multiple of
    64 * 840, hence of 3 x 256: with three workers a last bucket is shorter, never padded -- padded chunks are the
    op-level sizes of tests/_qef_checks.py), the host-offloaded snapshot.  Against an fp32-transport run of the
    same drifts the difference after T steps is bounded by the delivered-sum bound (tests/_qef_checks.py:
    sum_w s1_w / 2 + s2 / 2 + slack, the sum of the residuals) times lr (1 + mu) / W, with the scales bounded as in
    tests/test_qcomm_e2e_cpu.py: |drift| < 6 sigma, so s1 <= amax / 127 for each of the three workers and
    s2 <= 3 amax / 127."""
    unit = 3 * 256
    env, m, dl = q_mk("int8", bucket_mb=4 * unit / (1 << 20), offload_snapshot=True, ef=True)
    st = m.store
    dev = st.device
    calls0 = dl.outer_comm.stats.calls
    a, b = dl.my_shard
    nb = -(-st.numel // (4 * unit))
    last = st.numel - (nb - 1) * 4 * unit
    assert dl.buckets_per_outer_step == nb > 3 and 0 < last < 4 * unit
    assert [bk.c for bk in dl.transport._qplan] == [4 * 256] * (nb - 1) + [last // 3]
    assert dl.bytes_per_outer_step == sum(3 * (bk.c + bk.c // 256 * 4) for bk in dl.transport._qplan)
    assert dl.qef_send.numel() == b - a == st.numel
    assert dl.qef_reduce.numel() == sum(bk.c for bk in dl.transport._qplan) == (nb - 1) * 4 * 256 + last // 3
    assert [v.numel() for v in dl.transport._qef_views] == [bk.c for bk in dl.transport._qplan]
    assert all(v.data_ptr() == dl.qef_reduce.data_ptr() + 4 * 4 * 256 * i
               for i, v in enumerate(dl.transport._qef_views))
    _, m2, dl2 = q_mk(torch.float32, env=env)
    amax = SIGMA * 6
    resid = 3 * amax / 127 / 2 + 3 * amax / 127 / 2 + QEF_STEPS * (3 + 1) * 2.0 ** -23 * (2 * 3 * amax)
    bound = resid * LR * (1 + MU) / 3
    for s in range(QEF_STEPS):
        for mm, dd in ((m, dl), (m2, dl2)):
            mm.store.master.add_(drift(st.numel, s, rank).to(dev))
            dd.outer_step()
        dl.check_replicas(tol=0.0)
        check_step(dl)
        assert torch.equal(dl.sync, st.master.cpu()) and dl.sync.device.type == "cpu"
        err = (st.master - m2.store.master).abs().max().item()
        print(f"step {s + 1}: max |error feedback - fp32 transport| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    assert dl.outer_comm.stats.calls - calls0 == QEF_STEPS * 2 * nb
    return True


def _q_oracle_step(base, deltas, bits):
    """quantise each rank's delta, sum in rank order, requantise, dequantise -> (d_sum, sum of the ranks'
    scales per element, the second scale per element), each of the span's length."""
    n, w = base.numel(), len(deltas)
    c = qo.chunk(n, w)
    qs = [qo.quant_span(d, w, bits) for d in deltas]
    out, s1, s2 = [], torch.zeros(w, c), torch.zeros(w, c)
    for k in range(w):  # chunk k is reduced by worker k
        codes = torch.stack([q[0][k] for q in qs])
        scales = torch.stack([q[1][k] for q in qs])
        rc, rs = qo.reduce_chunks(codes, scales, bits)
        out.append(qo.dequant(rc, rs).view(-1))
        s1[k] = scales.sum(dim=0).repeat_interleave(qo.QB)
        s2[k] = rs.view(-1).repeat_interleave(qo.QB)
    return torch.cat(out)[:n], s1.view(-1)[:n], s2.view(-1)[:n]


def q_drift(n, rank):
    return 0.01 * torch.randn(n, generator=torch.Generator().manual_seed(rank))


def q_random_drift(rank, world, comm, inner_dp, device="cpu", dtype=torch.float32, env=None):
    bits = int(comm[3:])
    env, m, dl = q_mk(comm, inner_dp=inner_dp, env=env, device=device, dtype=dtype)
    st = m.store
    dev = st.device
    base = st.master.cpu().clone()
    w = env.num_workers
    a, b = dl.my_shard
    # every GPU of a worker drifts identically; each rank can rebuild every worker's drift
    drifts = [q_drift(st.numel, k) for k in range(w)]
    st.master.add_(drifts[env.worker].to(dev))
    # in-test oracle, shard by shard (the two-level mode reduces shard i on the i-th GPU of every worker)
    nes = Nesterov(base.clone().to(dev), device)
    want = nes.theta
    bound = torch.zeros_like(base)
    for x, y in dl.shards:
        deltas = [base[x:y] - (base[x:y] + d[x:y]) for d in drifts]
        dsum, s1, s2 = _q_oracle_step(base[x:y], deltas, bits)
        nes.step(x, y, dsum, 1.0 / w)
        bound[x:y] = (s1 / 2 + s2 / 2) / w * LR * (1 + MU)
    dl.outer_step()
    diff = (st.master - want).abs().max().item()
    print(f"{comm} W={w} inner_dp={inner_dp}: max |master - oracle| = {diff:.3e}")
    assert torch.equal(st.master, want), diff
    assert torch.equal(dl.sync, st.master)
    dl.check_replicas(tol=0.0)
    check_step(dl)
    c = qo.chunk(b - a, w)
    assert dl.bytes_per_outer_step == w * (c * bits // 8 + c // 256 * 4)
    assert dl.buckets_per_outer_step == 1
    # against fp32 transport: the same step on a second instance
    _, m2, dl2 = q_mk(torch.float32, env=env, inner_dp=inner_dp, device=device, dtype=dtype)
    assert torch.equal(m2.store.master.cpu(), base)
    m2.store.master.add_(drifts[env.worker].to(dev))
    dl2.outer_step()
    err = (st.master - m2.store.master).abs().cpu()
    print(f"{comm}: max |quantised - fp32| = {err.max().item():.3e}, smallest bound {bound[bound > 0].min().item():.3e}")
    assert bool((err <= bound)[: st.num_params].all()), (err - bound).max()
    return True


def q_several_buckets(rank, world):
    """Three workers, a bucket size that cuts the span into many buckets with a padded last one, the
    host-offloaded snapshot: identical to the one-bucket plan's oracle only per bucket, so check the
    invariants -- replicas bit-identical, bytes, and agreement with fp32 transport within the format's bound
    (one scale per block bounds both roundings by amax / QMAX each)."""
    env, m, dl = q_mk("int8", bucket_mb=3 * 256 / (1 << 20), offload_snapshot=True)
    st = m.store
    dev = st.device
    calls0 = dl.outer_comm.stats.calls
    st.master.add_(q_drift(st.numel, rank).to(dev))
    assert dl.buckets_per_outer_step == -(-st.numel // (3 * 256)) and dl.buckets_per_outer_step > 3
    assert dl.bytes_per_outer_step == dl.buckets_per_outer_step * 3 * 260
    dl.outer_step(phases=True)
    dl.check_replicas(tol=0.0)
    check_step(dl)
    assert torch.equal(dl.sync, st.master.cpu()) and dl.sync.device.type == "cpu"
    _, m2, dl2 = q_mk(torch.float32, env=env)
    m2.store.master.add_(q_drift(st.numel, rank).to(dev))
    dl2.outer_step()
    amax = 0.01 * 6  # |drift| < 6 sigma
    assert (st.master - m2.store.master).abs().max().item() <= (3 * amax / 127 / 2 + 3 * amax / 127 / 2) / 3 * LR * (1 + MU)
    assert dl.outer_comm.stats.calls - calls0 == 2 * dl.buckets_per_outer_step
    return True


# ------------------------------------------------------------------------------------------------ low-rank
def lowrank_two_steps(rank, world, bucket_mb, device="cpu", dtype=torch.float32, env=None):
    """Every worker drifts on its own; after each outer step theta_sync and the master are the same bits everywhere,
    the residuals are each worker's own, and their mean is what the step did not deliver: with the first step's
    momentum (buf = d) theta moved by lr (1 + mu) d, so mean_w(acc_w) - mean_w(e_w) = d must reproduce it.  Q is the
    same bits on every rank, and with two workers (a two-addend sum has no order) both steps equal, bit for bit, an
    in-process replay of the four ``ops.lowrank_*`` entry points for both workers with the two wire buffers added
    where the all-reduce sits.  Returns ``(conservation error, its tolerance)`` of the first step."""
    env = setup(device, env=env)
    m = model(lchk.TINY, 7, env, device, dtype)
    dl = diloco(m, env, comm_dtype=torch.float32, lowrank=4, bucket_mb=bucket_mb)
    assert isinstance(dl.transport, LowRankTransport)
    st, plan = m.store, dl.transport.plan
    dev = st.device
    calls0 = dl.outer_comm.stats.calls
    mask, comp = lchk.covered(plan, st.numel)
    tmask = torch.from_numpy(mask)
    tcomp = torch.from_numpy(comp).to(dev)
    w1, w2 = dl.transport.wire1.numel(), dl.transport.wire2.numel()
    assert dl.bytes_per_outer_step == 4 * (w1 + w2)
    assert (dl.buckets_per_outer_step > 2) == (bucket_mb < 1)
    figures = None
    # the replay's state: theta, momentum and Q are shared, the residual is each worker's own
    r_theta, r_mom = dl.sync.clone(), torch.zeros_like(dl.sync)
    r_q0 = plan.init_q().to(dev)
    r_q = r_q0.clone()
    r_e = [torch.zeros_like(dl.sync) for _ in range(world)]
    for s in range(2):
        drifts = [(0.01 * torch.randn(st.numel, generator=torch.Generator().manual_seed(100 * s + j)) * tmask).to(dev)
                  for j in range(world)]
        theta = dl.sync.clone()
        st.master.add_(drifts[env.worker])
        if world == 2:
            local = [r_theta + d for d in drifts]
            wire1 = [torch.zeros(w1, device=dev) for _ in range(world)]
            wire2 = [torch.zeros(w2, device=dev) for _ in range(world)]
            for j in range(world):
                ops.lowrank_project(r_theta, local[j], r_e[j], r_q, wire1[j], plan)
            p_sum = wire1[0] + wire1[1]
            ops.lowrank_orthonormalize(p_sum, plan)
            for j in range(world):
                ops.lowrank_backproject(r_e[j], p_sum, wire2[j], plan)
            q_sum = wire2[0] + wire2[1]
            for j in range(world):  # the update of every worker is the same; the residual it leaves is its own
                last = j == world - 1
                ops.outer_nesterov_lowrank(local[j], r_theta if last else r_theta.clone(), r_e[j], p_sum, q_sum,
                                           r_q if last else r_q.clone(), r_q0, r_mom if last else r_mom.clone(), None,
                                           plan, 1.0 / world, LR, MU, s == 0)
        dl.outer_step()
        dl.check_replicas(tol=0.0)
        check_step(dl)
        assert torch.equal(st.master, dl.sync) and bool(torch.isfinite(st.master).all())
        e = dl.lowrank_residual
        assert bool(e[tcomp].any()) and not bool(e[~tcomp].any())
        qs = [torch.zeros_like(dl.lowrank_q) for _ in range(world)]
        dist.all_gather(qs, dl.lowrank_q)
        assert all(torch.equal(q, qs[0]) for q in qs), "lowrank_q differs between ranks"
        if world == 2:
            assert torch.equal(st.master, r_theta), (s, (st.master - r_theta).abs().max().item())
            assert torch.equal(dl.outer_optimizer.momentum_buffer, r_mom) and torch.equal(dl.lowrank_q, r_q)
            assert torch.equal(e, r_e[env.worker])
        if s == 0:
            es = [torch.zeros_like(e) for _ in range(world)]
            dist.all_gather(es, e)
            assert not torch.equal(es[0], es[1])
            acc = torch.stack([-d for d in drifts]).double().mean(0)  # sync - master of worker j is -drift_j
            d = acc - torch.stack(es).double().mean(0) * tcomp
            moved = (theta - dl.sync).double()
            # theta is rounded once where it is written (half an ulp of |theta|, taken as 2^-22 max|theta| with
            # room for the two fma), d and the residuals carry fp32 roundings relative to the step itself
            tol = 2.0 ** -22 * float(theta.abs().max()) + 1e-6 * float(moved.abs().max())
            err = float((moved - LR * (1 + MU) * d).abs().max())
            print(f"low-rank W={world} bucket_mb={bucket_mb} {device}: conservation error {err:.3e}, tolerance {tol:.3e}")
            figures = (err, tol)
            assert err <= tol, (err, tol)
    assert dl.outer_comm.stats.calls - calls0 == 2 * dl.buckets_per_outer_step
    return figures


# ------------------------------------------------------------------------------------------------ dense
def dense_mk(rank, overlap=False, comm=torch.float32, inner_dp=1, seed=None, device="cpu", dtype=torch.float32,
             env=None, **kw):
    env = setup(device, inner_dp, env)
    m = model(TINY, seed if seed is not None else 100 + rank, env, device, dtype)
    return env, m, diloco(m, env, comm_dtype=comm, overlap=overlap, **kw)


def _dense_oracle(dl, base, drifts):
    """Master, sync and momentum of the FIRST dense outer step from ``base``: every worker's pseudo-gradient
    (``ops.pseudograd`` bits, in the wire dtype), summed in worker order, through ``ops.outer_nesterov`` with 1/W."""
    total = None
    for d in drifts:
        delta = torch.zeros(base.numel(), dtype=dl.delta.dtype, device=base.device)
        ops.pseudograd(base, base + d, delta)
        total = delta if total is None else total.add_(delta)
    master, sync, mom = base + drifts[dl.env.worker], base.clone(), torch.zeros_like(base)
    ops.outer_nesterov(master, sync, total, mom, None, 1.0 / len(drifts), LR, MU, True)
    return master, sync, mom


def _dense_check(dl, base, drifts):
    """After the first dense step: the invariants, and with two workers (a two-addend sum has no order, whatever
    algorithm the all-reduce takes) the oracle's bits."""
    check_step(dl)
    if len(drifts) == 2:
        master, sync, mom = _dense_oracle(dl, base, drifts)
        assert torch.equal(dl.store.master, master), (dl.store.master - master).abs().max().item()
        a, b = dl.my_shard  # the momentum of the other shards lives on the other GPUs of the worker
        assert torch.equal(dl.sync, sync) and torch.equal(dl.outer_optimizer.momentum_buffer[a:b], mom[a:b])


def dense_matches_torch(rank, world, device="cpu", dtype=torch.float32, env=None, inner_dp=1, bucket_mb=128.0):
    """Full outer step == reference math: per-tensor all_reduce(AVG) + SGD-Nesterov on snapshot."""
    env, m, dl = dense_mk(rank, seed=7, device=device, dtype=dtype, env=env, inner_dp=inner_dp, bucket_mb=bucket_mb)
    st = m.store
    dev = st.device
    w = env.num_workers
    drifts = [0.01 * torch.randn(st.numel, generator=torch.Generator().manual_seed(k)) for k in range(w)]
    base = st.master.clone()
    st.master.add_(drifts[env.worker].to(dev))
    assert (dl.buckets_per_outer_step > 1) == (bucket_mb < 1)
    # reference (on the host: the sum of every RANK's delta over the world, so 1 / world)
    p = torch.nn.Parameter(base.cpu().clone())
    sgd = torch.optim.SGD([p], lr=LR, momentum=MU, nesterov=True)
    grad = base.cpu() - (base.cpu() + drifts[env.worker])
    dist.all_reduce(grad)
    p.grad = grad / world
    sgd.step()
    dl.outer_step()
    assert torch.allclose(st.master.cpu(), p.detach(), atol=1e-6)
    _dense_check(dl, base, [d.to(dev) for d in drifts])
    return True


def dense_bf16_comm(rank, world, device="cpu", dtype=torch.float32, env=None):
    env, m, dl = dense_mk(rank, comm=torch.bfloat16, seed=9, device=device, dtype=dtype, env=env)
    st = m.store
    base = st.master.clone()
    st.master.sub_(rank + 1.0)
    dl.outer_step()
    assert torch.allclose(st.master[: st.num_params], (base - 1.995)[: st.num_params], atol=2e-2)
    assert dl.bytes_per_outer_step == st.numel * 2
    _dense_check(dl, base, [torch.full_like(base, -(k + 1.0)) for k in range(world)])
    return True


def dense_bf16_random(rank, world, device="cpu", dtype=torch.float32, env=None, bucket_mb=128.0):
    """The bf16 wire with a drift that is not bf16-representable: every worker's delta is rounded on its own."""
    env, m, dl = dense_mk(rank, comm=torch.bfloat16, seed=9, device=device, dtype=dtype, env=env, bucket_mb=bucket_mb)
    st = m.store
    base = st.master.clone()
    drifts = [drift(st.numel, 0, k).to(st.device) for k in range(world)]
    st.master.add_(drifts[rank])
    dl.outer_step()
    assert dl.bytes_per_outer_step == st.numel * 2 and (dl.buckets_per_outer_step > 1) == (bucket_mb < 1)
    _dense_check(dl, base, drifts)
    # against the exact mean in float64, whatever order the all-reduce sums in: every worker's delta is rounded to
    # bf16 once (7 stored mantissa bits: 2^-8 relative) and each of the W - 1 partial sums once more, none larger than sum_k |d_k|; the first
    # step moves theta by lr (1 + mu) times the mean; 1e-6: the fp32 roundings, the bound of the fp32 chain
    d = torch.stack([-x.double() for x in drifts])
    want = base.double() - LR * (1 + MU) * d.mean(0)
    bound = LR * (1 + MU) / world * world * 2.0 ** -8 * d.abs().sum(0) + 1e-6
    err = (st.master.double() - want).abs()
    assert bool((err <= bound).all()), (err - bound).max().item()
    return True


def dense_two_level(rank, world, device="cpu", dtype=torch.float32, env=None):
    """4 ranks = 2 workers x 2-GPU inner DDP; sharded outer all-reduce + intra-worker all-gather."""
    env, m, dl = dense_mk(rank, inner_dp=2, seed=11, device=device, dtype=dtype, env=env)
    st = m.store
    base = st.master.clone()
    st.master.sub_(env.worker + 1.0)    # both GPUs of a worker drift identically
    dl.outer_step()
    assert torch.allclose(st.master[: st.num_params], (base - 1.995)[: st.num_params], atol=1e-5)
    assert dl.bytes_per_outer_step == st.numel // 2 * 4
    dl.check_replicas()
    _dense_check(dl, base, [torch.full_like(base, -(k + 1.0)) for k in range(env.num_workers)])
    return True


# ------------------------------------------------------------------------------------------------ streaming
def stream_model(seed=3, env=None, device="cpu", dtype=torch.float32):
    return model(TINY4, seed, env, device, dtype)


def stream_diloco(m, env=None, **kw):
    return diloco(m, env, inner_steps=H, total=4 * H, **kw)


def _cat(t, spans):
    return torch.cat([t[a:b] for a, b in spans])


class FragReplay:
    """In-process replay of the fragment syncs through ``ops.frag_pseudograd`` / ``ops.frag_outer_mix`` for every
    worker: theta_sync and the momentum are shared, every worker has its own local weights, and the packed wire
    buffers are added in worker order where the all-reduce sits (bitwise for two workers only)."""

    def __init__(self, dl, masters):
        self.dl, self.masters = dl, masters  # masters[k]: worker k's local weights, moved along by the caller
        self.sync, self.mom = dl.sync.clone(), torch.zeros_like(dl.sync)
        self.steps = [0] * len(dl.frag_tables)
        self.wire = None

    def send(self, p):
        table = self.dl.frag_tables[p]
        total = None
        for mk in self.masters:
            wire = torch.zeros(table.total, dtype=self.dl.delta.dtype, device=mk.device)
            ops.frag_pseudograd(self.sync, mk, table, wire)
            total = wire if total is None else total.add_(wire)
        self.wire = (p, total)

    def apply(self, alpha):
        p, total = self.wire
        table, n = self.dl.frag_tables[p], len(self.masters)
        for k, mk in enumerate(self.masters):
            last = k == n - 1
            ops.frag_outer_mix(mk, self.sync if last else self.sync.clone(), total, self.mom if last else self.mom.clone(),
                               None, table, 1.0 / n, LR, MU, self.steps[p] == 0, alpha)
        self.steps[p] += 1

    def check(self, p=None):
        dl = self.dl
        if len(self.masters) != 2:
            return
        assert torch.equal(dl.store.master, self.masters[dl.env.worker]), "master != the replayed fragment syncs"
        assert torch.equal(dl.sync, self.sync) and torch.equal(dl.outer_optimizer.momentum_buffer, self.mom)
        if p is not None:
            spans = dl.frag_tables[p].spans
            assert torch.equal(_cat(dl.store.shadow, spans), _cat(dl.store.master, spans).to(dl.store.shadow.dtype))


def stream_golden(rank, world, device="cpu", dtype=torch.float32, env=None, comm=torch.float32):
    env = setup(device, env=env)
    m = stream_model(100 + rank, env, device, dtype)  # the init broadcast makes the replicas identical
    dl = stream_diloco(m, env=env, fragments=2, comm_dtype=comm)
    st = m.store
    f0, f1 = (t.spans for t in dl.frag_tables)
    theta0 = st.master.clone()
    st.master.sub_(rank + 1.0)  # delta = r + 1, average 1.5
    local = st.master.clone()
    rep = FragReplay(dl, [theta0 - (k + 1.0) for k in range(world)])
    assert dl.stream_step(H // 2) == {"sent": 0, "applied": 0}
    rep.send(0), rep.apply(0.0), rep.check(0)
    step1 = _cat(st.master - theta0, f0)
    assert torch.allclose(step1, torch.full_like(step1, -1.995), atol=1e-5), step1[:4]
    assert torch.equal(_cat(st.master, f1), _cat(local, f1))            # fragment 1: bitwise untouched
    assert torch.equal(_cat(dl.sync, f1), _cat(theta0, f1))
    assert not dl.outer_optimizer.momentum_buffer[f1[0][0]:f1[0][1]].any()
    assert torch.equal(_cat(dl.sync, f0), _cat(st.master, f0))
    # second sync of fragment 0 with zero drift: its own momentum only (fragment 1 never synced in between)
    th1 = st.master.clone()
    assert dl.stream_step(H + H // 2) == {"sent": 0, "applied": 0}
    rep.send(0), rep.apply(0.0), rep.check(0)
    step2 = _cat(st.master - th1, f0)
    assert torch.allclose(step2, torch.full_like(step2, -0.8505), atol=1e-5), step2[:4]
    assert torch.equal(_cat(st.master, f1), _cat(local, f1))
    assert dl.frag_steps == [2, 0] and dl.outer_step_count == 0
    # fragment 1's first sync still takes the `first` branch with its own (zero) history
    assert dl.stream_step(2 * H) == {"sent": 1, "applied": 1}
    rep.send(1), rep.apply(0.0), rep.check(1)
    step3 = _cat(st.master - theta0, f1)
    assert torch.allclose(step3, torch.full_like(step3, -1.995), atol=1e-5)
    assert dl.frag_steps == [2, 1] and dl.outer_step_count == 1
    check_step(dl)  # every fragment has been synced with alpha = 0 and no drift since
    n = sum(b - a for a, b in f1)
    assert dl.bytes_per_outer_step == n * dl.delta.element_size() and dl.buckets_per_outer_step == 1
    return True


def stream_tau_alpha(rank, world, alpha, device="cpu", dtype=torch.float32, env=None, comm=torch.float32):
    env = setup(device, env=env)
    m = stream_model(5, env, device, dtype)
    dl = stream_diloco(m, env=env, fragments=2, stream_overlap=1, stream_alpha=alpha, comm_dtype=comm)
    st = m.store
    f0, f1 = (t.spans for t in dl.frag_tables)
    theta0 = st.master.clone()
    st.master.sub_(rank + 1.0)
    rep = FragReplay(dl, [theta0 - (k + 1.0) for k in range(world)])
    assert dl.stream_step(H // 2) == {"sent": 0, "applied": None}
    rep.send(0)
    assert torch.equal(st.master, theta0 - (rank + 1.0))                 # nothing applied yet
    st.master.add_(0.25)                                                 # local progress inside the window
    for mk in rep.masters:
        mk.add_(0.25)
    local_now = st.master.clone()
    assert dl.stream_step(H // 2 + 1) == {"sent": None, "applied": 0}
    rep.apply(alpha), rep.check(0)
    theta_new = _cat(theta0, f0) - 1.995
    assert torch.allclose(_cat(dl.sync, f0), theta_new, atol=1e-5)
    if alpha:
        expect = alpha * _cat(local_now, f0) + (1 - alpha) * _cat(dl.sync, f0)
        assert torch.allclose(_cat(st.master, f0), expect, atol=1e-5)
        assert not torch.equal(_cat(st.master, f0), _cat(dl.sync, f0))
    else:  # the local progress on the fragment is discarded
        assert torch.equal(_cat(st.master, f0), _cat(dl.sync, f0))
    gathered = [torch.zeros_like(dl.sync) for _ in range(world)]
    dist.all_gather(gathered, dl.sync)
    assert all(torch.equal(g, gathered[0]) for g in gathered)            # theta_new identical on every rank
    assert torch.equal(_cat(st.master, f1), _cat(local_now, f1))         # the other fragment: unchanged
    assert torch.equal(_cat(dl.sync, f1), _cat(theta0, f1))
    dl.check_replicas()  # local weights legitimately differ; theta_sync must not
    dl.flush_fragments()
    for p in range(2):
        rep.send(p), rep.apply(0.0)
    rep.check()
    assert torch.equal(st.master, dl.sync)
    dl.check_replicas()
    check_step(dl)
    return True


# ------------------------------------------------------------------------------------------------ checkpoints
QEF_BUCKET = 2048 / (1 << 20)  # 2048 (int8) / 4096 (int4) elements per bucket: the two plans differ


def real_step(m, dl, s):
    """one outer step after a drift of the parameters alone: a checkpoint stores the model by parameter, so the
    alignment padding of the flat vector (which training never moves) comes back as it was initialised"""
    st = m.store
    real = torch.zeros(st.numel, dtype=torch.bool)
    for name in st.names:
        real[st.offsets[name]:st.offsets[name] + st.master_view(name).numel()] = True
    st.master.add_((drift(st.numel, s, dl.env.worker) * real).to(st.device))
    dl.outer_step()


def qef_checkpoints(rank, world, tmp):
    mk = q_mk
    env, m, dl = mk("int8", bucket_mb=QEF_BUCKET, ef=True)
    assert len(dl.transport._qplan) > 2
    real_step(m, dl, 0)
    save_checkpoint(os.path.join(tmp, "ef"), m, dl, env, 4)
    send1, red1 = dl.qef_send.clone(), dl.qef_reduce.clone()
    assert bool((send1 != 0).any()) and bool((red1 != 0).any())
    real_step(m, dl, 1)
    with open(os.path.join(tmp, "ef", "trainer_state.json")) as f:
        meta = json.load(f)["comm_error_feedback"]
    assert meta == {"bits": 8, "num_workers": 2, "plan": [[bk.x, bk.y, bk.c] for bk in dl.transport._qplan]}
    # save after step 1, load into a fresh instance, step 2: the uninterrupted run, bitwise
    _, m2, dl2 = mk("int8", env=env, bucket_mb=QEF_BUCKET, seed=8, ef=True)
    load_checkpoint(os.path.join(tmp, "ef"), m2, dl2, env)
    assert torch.equal(dl2.qef_send, send1) and torch.equal(dl2.qef_reduce, red1)
    real_step(m2, dl2, 1)
    assert torch.equal(m2.store.master, m.store.master) and torch.equal(dl2.sync, dl.sync)
    assert torch.equal(dl2.qef_send, dl.qef_send) and torch.equal(dl2.qef_reduce, dl.qef_reduce)
    # a stateless checkpoint, resumed with the flag on: zero residuals, the run goes on
    _, m3, dl3 = mk("int8", env=env, bucket_mb=QEF_BUCKET, ef=False)
    real_step(m3, dl3, 0)
    save_checkpoint(os.path.join(tmp, "plain"), m3, dl3, env, 4)
    with open(os.path.join(tmp, "plain", "trainer_state.json")) as f:
        assert "comm_error_feedback" not in json.load(f)
    _, m4, dl4 = mk("int8", env=env, bucket_mb=QEF_BUCKET, seed=9, ef=True)
    dl4.qef_send.fill_(1.0)  # whatever was there is dropped
    dl4.qef_reduce.fill_(1.0)
    load_checkpoint(os.path.join(tmp, "plain"), m4, dl4, env)
    assert not bool(dl4.qef_send.any()) and not bool(dl4.qef_reduce.any())
    real_step(m4, dl4, 1)
    dl4.check_replicas(tol=0.0)
    assert bool(torch.isfinite(m4.store.master).all()) and bool((dl4.qef_send != 0).any())
    # a checkpoint with residuals, resumed without the flag: ignored, the stateless run of that state
    _, m5, dl5 = mk("int8", env=env, bucket_mb=QEF_BUCKET, ef=False, seed=10)
    load_checkpoint(os.path.join(tmp, "ef"), m5, dl5, env)
    assert dl5.error_feedback_state() is None and not hasattr(dl5, "qef_send")
    real_step(m5, dl5, 1)
    dl5.check_replicas(tol=0.0)
    assert bool(torch.isfinite(m5.store.master).all()) and not torch.equal(m5.store.master, m.store.master)
    # int8 -> int4: qef.send is per element and stays; qef.reduce follows the plan, which differs: zero
    _, m6, dl6 = mk("int4", env=env, bucket_mb=QEF_BUCKET, seed=11, ef=True)
    assert [[bk.x, bk.y, bk.c] for bk in dl6.transport._qplan] != meta["plan"]
    dl6.qef_reduce.fill_(1.0)
    load_checkpoint(os.path.join(tmp, "ef"), m6, dl6, env)
    assert torch.equal(dl6.qef_send, send1) and not bool(dl6.qef_reduce.any())
    real_step(m6, dl6, 1)
    dl6.check_replicas(tol=0.0)
    return True


RESIDUALS = {"qef": ("qef_send", "qef_reduce"), "topk": ("topk_residual",), "lowrank": ("lowrank_residual", "lowrank_q")}


def resume_roundtrip(rank, world, tmp, kind, device="cpu", dtype=torch.float32, env=None):
    """Two outer steps, a checkpoint (``save_checkpoint``), a fresh ``Diloco`` of another seed that loads it
    (``load_checkpoint``), a third step on both: master, sync, momentum and the transport's residuals are the same
    bits -- the residuals live where the model does, so on ``"cuda"`` they come back onto the device."""
    env = setup(device, env=env)
    cfg = lchk.TINY if kind == "lowrank" else TINY
    kw = {"qef": dict(comm_dtype="int8", error_feedback=True, bucket_mb=8192 / (1 << 20)),  # two buckets each
          "topk": dict(comm_dtype=torch.bfloat16, topk=64, bucket_mb=TOPK_BUCKET),
          "lowrank": dict(comm_dtype=torch.float32, lowrank=4)}[kind]
    made = []
    for seed in (7, 8):
        m = model(cfg, seed, env, device, dtype)
        made.append((m, diloco(m, env, **kw)))
    (m, dl), (m2, dl2) = made
    assert dl.buckets_per_outer_step > 1 or kind == "lowrank"  # (no launcher sees the buckets of an all-reduce)
    for s in range(2):
        real_step(m, dl, s)
    path = os.path.join(tmp, kind)
    save_checkpoint(path, m, dl, env, 8)
    saved = [getattr(dl, name).clone() for name in RESIDUALS[kind]]
    assert all(bool((t != 0).any()) for t in saved)
    load_checkpoint(path, m2, dl2, env)
    for name, t in zip(RESIDUALS[kind], saved):
        got = getattr(dl2, name)
        assert got.device == m2.store.device and torch.equal(got, t), name
    assert torch.equal(m2.store.master, m.store.master) and torch.equal(dl2.sync, dl.sync)
    for mm, dd in made:
        real_step(mm, dd, 2)
        check_step(dd)
    assert torch.equal(m2.store.master, m.store.master) and torch.equal(dl2.sync, dl.sync)
    assert torch.equal(dl2.outer_optimizer.momentum_buffer, dl.outer_optimizer.momentum_buffer)
    for name, t in zip(RESIDUALS[kind], saved):
        assert torch.equal(getattr(dl2, name), getattr(dl, name)), name
        assert not torch.equal(getattr(dl, name), t), f"{name}: the third step changed nothing"
    return True
