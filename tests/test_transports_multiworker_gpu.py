"""Every outer transport's ``step()`` with SEVERAL workers on the HIP kernels.

Only one GPU is visible to the tests, so W workers are W processes that share it over gloo (tests/_mp.run_ranks, as
tests/test_multirank_gpu.py does with torchrun).  That is what only W > 1 or
``inner_dp`` produces and the PyTorch path cannot object to: worker slices ``gath[r * pb:(r + 1) * pb]`` at ``r > 0``
(byte offsets that are a multiple of 4 but not of 16), bucket starts ``bk.x > 0``, shard starts ``a > 0``, residual
views, ``sh_full[ga:gb]`` of a separate bf16 shadow, ``inv_w < 1`` and the reducer's error-feedback stage for chunk
``r``.

Three process groups: W = 2, W = 3 and 4 ranks as two workers of two shards (``inner_dp = 2``; streaming and low-rank
refuse that).  The child of each runs its chains (tests/_outer_chains.py, the chains of the CPU tests) one after
another in the same group, under a launcher spy: every chain states which ``nd_*`` entry points had to run how often,
and no launcher may answer with an error code.  What is bitwise and what is bounded: docs/PARITY.md."""
import collections
import time

import pytest
import torch
import torch.distributed as dist

from nanodiloco_amd.parallel.comm import FlatCommunicator, PendingAllReduce, _DoneWork, plan_buckets

from . import _model_oracle as mo
from . import _outer_chains as oc
from ._mp import run_ranks

pytestmark = pytest.mark.gpu
LIMIT = 180  # seconds per group; a group takes a few tens of seconds
BF16, F32 = torch.bfloat16, torch.float32
# The quantised and dense small-bucket variants cut the tiny model's span in TWO buckets (bk.x > 0), not in the many of
# the CPU tests: the W processes share one GPU, and every collective costs each of them a device synchronisation (a few
# tenths of a second), so a chain's time is its number of collectives.  For the same reason the many-bucket chains of
# the CPU tests that are bounded against fp32, not bitwise, stay on the CPU.  Top-k and low-rank take the CPU tests' own.
TOPK_BUCKET = oc.TOPK_BUCKET  # tests/test_topk_e2e_cpu.py: three chunks of k = 64 per slot
LOWRANK_BUCKET = 0.01  # tests/test_lowrank_e2e_cpu.py: several buckets per all-reduce
HALF = 8192  # elements per bucket
C10D = "c10d on device: "  # a chain whose collectives are FlatCommunicator's own, on device tensors


def _two(elem_bits):
    return HALF * elem_bits / 8 / (1 << 20)


@pytest.fixture(autouse=True)
def _gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class _HostStaged(FlatCommunicator):
    """The three asynchronous collectives of ``FlatCommunicator`` staged through the host, for the children of this
    file only.  gloo does take device tensors (the ``C10D`` chains of the two-worker group run on them), but with
    several asynchronous device collectives in flight each one takes about a second (measured: 72 s for three steps of
    seven buckets, 1.4 s for the same chain with one bucket), and that is gloo's time, not the kernels'.  The launchers
    meet the same pointers, offsets and buffers; the calls and bytes are counted as the parent counts them."""

    def _count(self, nbytes):
        self.stats.calls += 1
        self.stats.bytes += nbytes

    def all_reduce_async(self, flat, ranges=None):
        if ranges is None:
            ranges = plan_buckets(0, flat.numel(), flat.element_size(), self.bucket_bytes)
        for a, b in ranges:
            if self.enabled:
                host = flat[a:b].cpu()
                dist.all_reduce(host, op=dist.ReduceOp.SUM, group=self.group)
                flat[a:b].copy_(host)
                self._count((b - a) * flat.element_size())
        return PendingAllReduce([None] * len(ranges), list(ranges), flat)

    def all_to_all_async(self, send, recv):
        if send.numel() % max(1, self.size) or recv.numel() != send.numel():
            raise ValueError("all_to_all: send / recv must match and divide by the group size")
        if not self.enabled:
            return super().all_to_all_async(send, recv)
        host = torch.empty(send.numel(), dtype=send.dtype)
        dist.all_to_all_single(host, send.cpu(), group=self.group)
        recv.copy_(host)
        self._count(send.numel() * send.element_size())
        return _DoneWork()

    def all_gather_async(self, out, my_index):
        if out.numel() % max(1, self.size):
            raise ValueError("all_gather: numel not divisible by the group size")
        if not self.enabled:
            return super().all_gather_async(out, my_index)
        n = out.numel() // self.size
        host = torch.empty(out.numel(), dtype=out.dtype)
        dist.all_gather_into_tensor(host, out[my_index * n:(my_index + 1) * n].cpu(), group=self.group)
        out.copy_(host)
        self._count(n * out.element_size())
        return _DoneWork()


class _Spy(mo.LauncherSpy):
    """The launcher spy, which also keeps every non-zero answer of a launcher (``errors``)."""

    def __init__(self, lib):
        super().__init__(lib)
        self.errors = collections.Counter()

    def __getattr__(self, name):
        counted = super().__getattr__(name)
        launcher = not (name.endswith("_splits") or "_set" in name or name in self._NOT_LAUNCHERS)

        def checked(*args):
            rc = counted(*args)
            if launcher and rc != 0:
                self.errors[name, rc] += 1
            return rc

        return checked


# what a quantised chain launches: the instance under test for ``steps`` steps plus the stateless twin's one step
def _q(ef, steps):
    e = "_ef" if ef else ""
    want = {"nd_pseudograd_q" + e: steps, "nd_qreduce" + e: steps, "nd_outer_nesterov_q": steps + 1}
    want["nd_pseudograd_q"] = want.get("nd_pseudograd_q", 0) + 1
    want["nd_qreduce"] = want.get("nd_qreduce", 0) + 1
    return want


def _q_chain(comm, inner_dp, ef, bucket_mb=128.0, dtype=BF16):
    """(label, chain, args, kwargs, launches, exact): stateless two steps, with error feedback three."""
    steps = 3 if ef else 2
    return (f"{comm}{' ef' if ef else ''} bucket_mb={bucket_mb:g} {dtype}", oc.qef_chain, (comm, inner_dp),
            dict(ef=ef, steps=steps, bucket_mb=bucket_mb, dtype=dtype), _q(ef, steps), bucket_mb >= 1)


TOPK = {"nd_pseudograd_topk": 2, "nd_outer_nesterov_topk": 2}
LOWRANK = ("nd_lowrank_project", "nd_lowrank_orthonormalize", "nd_lowrank_backproject", "nd_outer_nesterov_lowrank")
FRAG = ("nd_frag_pseudograd", "nd_frag_outer_mix")


def _lowrank(world):
    """two steps of the transport; with two workers the replay adds one launch per worker and step (the
    orthonormalisation: one per step)"""
    replay = {2: (4, 2, 4, 4)}.get(world, (0, 0, 0, 0))
    return {name: 2 + extra for name, extra in zip(LOWRANK, replay)}


def _cases(group, world, tmp):
    """The chains of one group: (label, chain, args, kwargs, launcher -> launches, exact counts?)."""
    # dense: the transport's launch, and with two workers the oracle's (one pseudo-gradient per worker, one update)
    dense = lambda n: {"nd_pseudograd": n, "nd_outer_nesterov": 2 if n > 1 else 1}  # noqa: E731
    if group == "two_level":  # 4 ranks: two workers of two shards
        return [
            ("dense two-level", oc.dense_two_level, (), {}, dense(3), False),
            ("dense fp32 random", oc.dense_matches_torch, (), dict(inner_dp=2), dense(3), False),
            ("dense fp32 random, buckets, fp32 model", oc.dense_matches_torch, (),
             dict(inner_dp=2, bucket_mb=_two(32), dtype=F32), dense(3), False),
            ("int8 one step", oc.q_random_drift, ("int8", 2), {}, {"nd_pseudograd_q": 1, "nd_qreduce": 1,
                                                                    "nd_outer_nesterov_q": 1}, True),
            ("int4 one step", oc.q_random_drift, ("int4", 2), {}, {"nd_pseudograd_q": 1, "nd_qreduce": 1,
                                                                    "nd_outer_nesterov_q": 1}, True),
            _q_chain("int8", 2, False), _q_chain("int4", 2, False), _q_chain("int8", 2, True), _q_chain("int4", 2, True),
            _q_chain("int4", 2, True, _two(4)), _q_chain("int8", 2, True, _two(8), F32),
            ("top-k bf16 k=7", oc.topk_chain, (BF16, 7, 2, 128.0), {}, TOPK, True),
            ("top-k fp32 k=64, fp32 model", oc.topk_chain, (F32, 64, 2, 128.0), dict(dtype=F32), TOPK, True),
        ]
    cases = [
        # ---- dense: two addends have no order, so W = 2 is bitwise (the chains compare when world == 2)
        ("dense fp32 random", oc.dense_matches_torch, (), {}, dense(1 + (world if world == 2 else 0)), False),
        ("dense fp32 random, buckets, fp32 model", oc.dense_matches_torch, (), dict(bucket_mb=_two(32), dtype=F32),
         dense(1 + (world if world == 2 else 0)), False),
        ("dense bf16 random, buckets", oc.dense_bf16_random, (), dict(bucket_mb=_two(16)),
         dense(1 + (world if world == 2 else 0)), False),
        # ---- int8 / int4: the reduction is the kernel's own, in rank order, so W = 3 is bitwise too
        _q_chain("int8", 1, False), _q_chain("int4", 1, False), _q_chain("int8", 1, True), _q_chain("int4", 1, True),
        _q_chain("int8", 1, True, _two(8)), _q_chain("int4", 1, False, _two(4)),
        _q_chain("int8", 1, True, dtype=F32),
        # ---- top-k
        ("top-k fp32 k=7", oc.topk_chain, (F32, 7, 1, 128.0), {}, TOPK, True),
        ("top-k bf16 k=64", oc.topk_chain, (BF16, 64, 1, 128.0), {}, TOPK, True),
        ("top-k bf16 k=64, buckets", oc.topk_chain, (BF16, 64, 1, TOPK_BUCKET), {}, TOPK, False),
        ("top-k fp32 k=64", oc.topk_chain, (F32, 64, 1, 128.0), {}, TOPK, True),
        ("top-k bf16 k=7", oc.topk_chain, (BF16, 7, 1, 128.0), {}, TOPK, True),
        ("top-k fp32 k=7, fp32 model", oc.topk_chain, (F32, 7, 1, 128.0), dict(dtype=F32), TOPK, True),
        # ---- low-rank
        ("low-rank R=4", oc.lowrank_two_steps, (128.0,), {}, _lowrank(world), True),
        ("low-rank R=4, buckets", oc.lowrank_two_steps, (LOWRANK_BUCKET,), {}, _lowrank(world), True),
        ("low-rank R=4, fp32 model", oc.lowrank_two_steps, (128.0,), dict(dtype=F32), _lowrank(world), True),
    ]
    if world == 3:
        return cases
    # ---- W = 2 only: the golden values of the dense and streaming chains are two workers', and so is the replay
    frag = {name: 3 + 3 * world for name in FRAG}  # three fragment syncs, replayed for every worker
    cases += [("dense bf16", oc.dense_bf16_comm, (), {}, dense(3), False)]
    cases += [(f"streaming golden {comm} wire {dtype} model", oc.stream_golden, (), dict(comm=comm, dtype=dtype), frag, True)
              for comm, dtype in ((F32, BF16), (BF16, BF16), (F32, F32))]
    cases += [(f"streaming tau=1 alpha={alpha} {comm} wire", oc.stream_tau_alpha, (alpha,), dict(comm=comm), frag, True)
              for alpha in (0.0, 0.5) for comm in (F32, BF16)]
    # ---- FlatCommunicator's own asynchronous c10d collectives on device tensors, one chain per transport
    cases += [(C10D + label, chain, args, kw, launches, exact) for label, chain, args, kw, launches, exact in (
        cases[0], _q_chain("int8", 1, True), _q_chain("int4", 1, False),
        ("top-k bf16 k=64", oc.topk_chain, (BF16, 64, 1, 128.0), {}, TOPK, True),
        ("low-rank R=4", oc.lowrank_two_steps, (128.0,), {}, _lowrank(world), True),
        (f"streaming tau=1 alpha=0.5 {BF16} wire", oc.stream_tau_alpha, (0.5,), dict(comm=BF16), frag, True))]
    # ---- checkpoints of device-resident residuals
    cases += [(f"resume {kind}", oc.resume_roundtrip, (tmp, kind), {}, launches, False)
              for kind, launches in (("qef", {"nd_pseudograd_q_ef": 4, "nd_qreduce_ef": 4}),
                                     ("topk", {"nd_pseudograd_topk": 4}), ("lowrank", {"nd_lowrank_project": 4}))]
    return cases


def _child(rank, world, group, tmp):
    """All chains of one group, one after another in one process group.  Returns ``[(label, seconds, result)]``."""
    from nanodiloco_amd.ops import _ext
    from nanodiloco_amd.parallel import diloco
    # the oracles are small CPU tensors: W processes with a thread pool each, sized by the machine, only fight
    torch.set_num_threads(2)
    env = oc.setup("cuda", inner_dp=2 if group == "two_level" else 1)
    t_start = time.perf_counter()
    spy = _Spy(_ext.lib())
    out = []
    for label, chain, args, kw, launches, exact in _cases(group, world, tmp):
        t0 = time.perf_counter()
        before = collections.Counter(spy.calls)
        # this child only: a spawned process that ends with its chains
        diloco.FlatCommunicator = FlatCommunicator if label.startswith(C10D) else _HostStaged
        with _ext.using(spy):
            res = chain(rank, world, *args, device="cuda", env=env, **{"dtype": BF16, **kw})
        torch.cuda.synchronize()
        ran = {name: spy.calls[name] - before[name] for name in launches}
        short = {n: (ran[n], want) for n, want in launches.items() if (ran[n] != want if exact else ran[n] < want)}
        assert not short, (f"[{group}: {label}] launches (got, {'exactly' if exact else 'at least'}): {short}; "
                           f"all: {dict(spy.calls - before)}")
        assert not spy.refused and not spy.errors, (label, dict(spy.refused), dict(spy.errors))
        out.append((label, round(time.perf_counter() - t0, 3), res))
        if rank == 0:
            print(f"[multiworker] {group} +{time.perf_counter() - t_start:6.1f} s  done: {label}", flush=True)
    return out


_failed = []  # a group that failed: no GPU work follows a failed rank, in the groups after it either


def _run(group, world, tmp_path):
    assert not _failed, f"group {_failed[0]} failed before this one: nothing more is started on the GPU"
    _failed.append(group)
    t0 = time.perf_counter()
    ranks = run_ranks(_child, world, group, str(tmp_path), limit=LIMIT)
    _failed.pop()
    wall = time.perf_counter() - t0
    print(f"[multiworker] group {group} ({world} ranks): {wall:.1f} s wall, {len(ranks[0])} chains")
    for label, secs, res in ranks[0]:
        print(f"[multiworker]   {secs:7.3f} s  {label}: {res}")
    for label, _, res in (c for r in ranks for c in r):
        assert res is not None and res is not False, label
    return ranks


def test_two_workers(tmp_path):
    _run("w2", 2, tmp_path)


def test_three_workers(tmp_path):
    _run("w3", 3, tmp_path)


def test_two_workers_of_two_shards(tmp_path):
    _run("two_level", 4, tmp_path)
