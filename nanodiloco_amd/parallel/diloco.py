"""DiLoCo: H local AdamW steps per worker, then an outer Nesterov step on the averaged
pseudo-gradient.  Capability parity with ``class Diloco`` (REF/nanodiloco/diloco/diloco.py:7-74):

  reference                                      here
  ---------------------------------------------  ------------------------------------------------
  per-tensor broadcast from rank 0 (:21-22)      one bucketed flat broadcast of the fp32 master
  CPU snapshot, pageable, per tensor (:27-32)    device-resident flat fp32 ``sync`` (288 GB HBM);
                                                 ``offload_snapshot=True`` keeps it in pinned host
  per-tensor H2D, sub, all_reduce(AVG), reset    ``nd_pseudograd`` -> bucketed async all-reduce(SUM)
  then SGD-Nesterov step + zero_grad (:46-53)    on RCCL's stream -> per-bucket fused
                                                 ``nd_outer_nesterov`` (1/W, momentum, Nesterov,
                                                 theta, sync, bf16 shadow in one pass), overlapping
                                                 the reduction of the next bucket
  clip + AdamW + scheduler + zero_grad (:56-60)  fused clip+AdamW kernels + host cosine schedule
  avg_sync_time always 0 (:62-64, dead)          real: wall time of every outer step (host) and
                                                 device time of its collectives (HIP events)

Extensions (north star).  How the pseudo-gradient travels is one of five transports
(``parallel/transports.py``, whose classes document the protocols); :func:`_check_options` has every rule
about which options go together:
* ``comm_dtype`` fp32 / bf16 (half the bytes / outer step), ``overlap=True`` (the DELAYED outer update: one
  burst, applied one step late; ``overlap=False`` is bit-faithful to the reference order):
  :class:`~.transports.DenseTransport`;
* ``comm_dtype="int8"`` / ``"int4"`` (``torch.int8`` = ``"int8"``), ``error_feedback=True``:
  :class:`~.transports.QuantisedTransport`;
* ``fragments=P`` with ``fragment_pattern``, ``stream_overlap``, ``stream_alpha`` (Streaming DiLoCo), driven by
  :meth:`Diloco.stream_step`: :class:`~.transports.StreamingTransport`;
* ``topk=K`` (--comm-topk; ``comm_dtype`` fp32 / bf16 is then the dtype of the values sent): the K largest entries
  of every 4096-element chunk travel, the rest waits in an fp32 residual: :class:`~.transports.TopKTransport`;
* ``lowrank=R`` (--comm-rank; PowerSGD): every large enough matrix travels as two all-reducible factors of R columns,
  what they did not carry waits in an fp32 residual: :class:`~.transports.LowRankTransport`;
* ``inner_dp > 1`` (two-level): the W/K workers' outer all-reduce is sharded over the K GPUs of a
  worker (each reduces 1/K of the pseudo-gradient over its outer group, then the worker
  all-gathers the updated weights), so cross-worker bytes per GPU drop by K.
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from ..models.llama import LlamaForCausalLM
from ..optim import FlatAdamW, FlatMuon, FlatOuterNesterov
from ..utils.schedule import CosineWarmupSchedule
from .comm import FlatCommunicator
from .dist import DistEnv
from .fragments import PATTERNS
from ..ops.sparse_comm import CHUNK as TOPK_CHUNK
from ..ops.lowrank_comm import MAX_RANK as LOWRANK_MAX
from .transports import DenseTransport, LowRankTransport, QuantisedTransport, StepTimer, StreamingTransport, \
    TopKTransport
from .transports import quantised_bits  # also the name existing imports of it use


def _check_options(flat_store: bool, comm_dtype=torch.float32, overlap=False, offload_snapshot=False, inner_dp=1,
                   error_feedback=False, fragments=0, fragment_pattern="strided", stream_overlap=0, stream_alpha=0.0,
                   num_layers=0, inner_steps=0, topk=0, lowrank=0) -> int:
    """Every rule about which options go together, checked before a transport exists.  Returns the bits of
    the quantised transport (0: fp32 / bf16)."""
    if lowrank:
        _check_lowrank(flat_store, comm_dtype, overlap, error_feedback, fragments, topk, inner_dp, lowrank)
    if topk:
        _check_topk(flat_store, comm_dtype, overlap, error_feedback, fragments, topk)
    if not flat_store:
        if fragments:
            raise ValueError("Streaming DiLoCo (fragments > 0) needs the flat-store Llama of Diloco: "
                             "ModuleDiloco does not take the streaming options")
        if error_feedback:
            raise ValueError("error_feedback belongs to the quantised transport (comm_dtype int8 / int4), which "
                             "needs the flat-store Llama of Diloco: ModuleDiloco does not take it")
        return 0
    qbits = quantised_bits(comm_dtype)
    if qbits and overlap:
        raise ValueError("quantised transport (comm_dtype int8 / int4) does not support overlap=True yet: the "
                         "delayed application and its pending-state checkpoint need the fp32 / bf16 path")
    if error_feedback and not qbits:
        raise ValueError("error_feedback=True (--comm-error-feedback) needs the quantised transport: comm_dtype "
                         f"'int8' or 'int4', not {comm_dtype}")
    if not fragments:
        return qbits
    P, H, tau, alpha = fragments, inner_steps, stream_overlap, stream_alpha
    if fragment_pattern not in PATTERNS:
        raise ValueError(f"fragment_pattern must be one of {PATTERNS}, not {fragment_pattern!r}")
    if not 1 <= P <= min(num_layers, H):
        raise ValueError(f"fragments must be in [1, min(num_layers={num_layers}, inner_steps={H})], got {P}")
    if not 0 <= tau < H // P:
        raise ValueError(f"stream_overlap must be in [0, inner_steps // fragments = {H // P}), got {tau}: a "
                         f"fragment must be applied before the next one is sent")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"stream_alpha must be in [0, 1], got {alpha}")
    for on, what in ((overlap, "overlap=True (--overlap-outer)"),
                     (bool(qbits), "quantised transport (comm_dtype int8 / int4)"),
                     (offload_snapshot, "offload_snapshot=True (--offload-snapshot)"),
                     (inner_dp > 1, "inner_dp > 1 (--inner-dp)")):
        if on:
            raise ValueError(f"Streaming DiLoCo (fragments > 0) is not supported together with {what}")
    return qbits


def _check_topk(flat_store: bool, comm_dtype, overlap, error_feedback, fragments, topk) -> None:
    """The rules of the top-k sparse transport (``topk`` > 0, --comm-topk)."""
    if not flat_store:
        raise ValueError("top-k sparse transport (topk > 0, --comm-topk) needs the flat-store Llama of Diloco: "
                         "ModuleDiloco does not take it")
    if not 1 <= int(topk) <= TOPK_CHUNK:
        raise ValueError(f"topk (--comm-topk) must be in [1, {TOPK_CHUNK}] entries per chunk of {TOPK_CHUNK}, got {topk}")
    if comm_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"top-k sparse transport (topk > 0, --comm-topk) sends fp32 or bf16 values, not comm_dtype "
                         f"{comm_dtype}: int8 / int4 block quantisation is another transport")
    for on, what in ((error_feedback, "error_feedback=True (--comm-error-feedback): top-k always carries its own "
                                      "residual, and that flag belongs to the quantised transport"),
                     (overlap, "overlap=True (--overlap-outer)"),
                     (bool(fragments), "Streaming DiLoCo (fragments > 0, --streaming-fragments)")):
        if on:
            raise ValueError(f"top-k sparse transport (topk > 0, --comm-topk) is not supported together with {what}")


def _check_lowrank(flat_store: bool, comm_dtype, overlap, error_feedback, fragments, topk, inner_dp, lowrank) -> None:
    """The rules of the low-rank transport (``lowrank`` > 0, --comm-rank)."""
    if not flat_store:
        raise ValueError("low-rank transport (lowrank > 0, --comm-rank) needs the flat-store Llama of Diloco: "
                         "ModuleDiloco does not take it")
    if not 1 <= int(lowrank) <= LOWRANK_MAX:
        raise ValueError(f"lowrank (--comm-rank) must be in [1, {LOWRANK_MAX}] columns per factor, got {lowrank}")
    if comm_dtype != torch.float32:
        raise ValueError(f"low-rank transport (lowrank > 0, --comm-rank) sends fp32 factors, not comm_dtype "
                         f"{comm_dtype}: bf16 or quantised factors are not implemented")
    for on, what in ((error_feedback, "error_feedback=True (--comm-error-feedback): low-rank always carries its own "
                                      "residual, and that flag belongs to the quantised transport"),
                     (bool(topk), "the top-k sparse transport (topk > 0, --comm-topk)"),
                     (overlap, "overlap=True (--overlap-outer)"),
                     (bool(fragments), "Streaming DiLoCo (fragments > 0, --streaming-fragments)"),
                     (inner_dp > 1, "inner_dp > 1 (--inner-dp): the shards of a worker cut matrices")):
        if on:
            raise ValueError(f"low-rank transport (lowrank > 0, --comm-rank) is not supported together with {what}")


class Diloco:
    """Flagship DiLoCo on the flat-store Llama.  Any other ``nn.Module`` (with plain torch optimizers)
    is dispatched to :class:`~nanodiloco_amd.parallel.module_diloco.ModuleDiloco`, which has the
    reference's generic ``model.parameters()`` / ``param_groups`` contract."""

    def __new__(cls, model, *args, **kwargs):
        if not isinstance(model, LlamaForCausalLM):
            from .module_diloco import ModuleDiloco
            _check_options(False, fragments=kwargs.get("fragments"), error_feedback=kwargs.pop("error_feedback", False),
                           topk=kwargs.pop("topk", 0), lowrank=kwargs.pop("lowrank", 0))
            return ModuleDiloco(model, *args, **kwargs)
        return super().__new__(cls)

    def __init__(self, model: LlamaForCausalLM, inner_optimizer: Union[FlatAdamW, FlatMuon],
                 outer_optimizer: FlatOuterNesterov,
                 warmup_steps: int, total_steps: int, inner_steps: int = 100, outer_steps: Optional[int] = None,
                 env: Optional[DistEnv] = None, comm_dtype: torch.dtype = torch.float32, bucket_mb: float = 128.0,
                 overlap: bool = False, offload_snapshot: bool = False, debug_checks: bool = False,
                 broadcast_init: bool = True, fragments: int = 0, fragment_pattern: str = "strided",
                 stream_overlap: int = 0, stream_alpha: float = 0.0, error_feedback: bool = False, topk: int = 0,
                 lowrank: int = 0):
        self.model = model
        self.store = model.store
        self.inner_optimizer = inner_optimizer
        self.outer_optimizer = outer_optimizer
        self.inner_steps = inner_steps
        self.outer_steps = outer_steps if outer_steps is not None else max(1, total_steps // max(1, inner_steps))
        self.env = env or DistEnv(device=self.store.device)
        self.scheduler = CosineWarmupSchedule(inner_optimizer.lr, warmup_steps, total_steps)
        self.error_feedback = bool(error_feedback)
        self.comm_dtype = comm_dtype
        self.overlap = overlap
        self.offload_snapshot = offload_snapshot
        self.debug_checks = debug_checks
        self.fragments = int(fragments)
        self.fragment_pattern = fragment_pattern
        self.stream_overlap = int(stream_overlap)
        self.stream_alpha = float(stream_alpha)
        self.topk = int(topk)
        self.lowrank = int(lowrank)
        qbits = _check_options(True, comm_dtype, overlap, offload_snapshot, self.env.inner_dp, error_feedback,
                               self.fragments, fragment_pattern, self.stream_overlap, self.stream_alpha,
                               model.config.num_hidden_layers, inner_steps, self.topk, self.lowrank)
        e = self.env
        f = e.force_collectives
        kw = dict(impl=e.comm_impl, device=e.device, timeout_s=e.timeout_s)
        self.outer_comm = FlatCommunicator(e.outer_group, e.num_workers, bucket_mb, force=f, **kw)
        self.inner_comm = FlatCommunicator(e.inner_group, e.inner_dp, bucket_mb, force=f and e.force_inner_ddp, **kw)
        self.world_comm = FlatCommunicator(e.world_group, e.world_size, bucket_mb, force=f, **kw)
        n = self.store.numel
        # shard of the flat vector this GPU reduces over the outer group (two-level mode)
        k = e.inner_dp
        if n % (k * 64):
            raise ValueError("flat size must be divisible by 64*inner_dp (ParamStore pads to 64)")
        self.shards = [(i * n // k, (i + 1) * n // k) for i in range(k)]
        self.my_shard = self.shards[e.inner_rank]

        # ---- replicate the init (reference: 57 per-tensor broadcasts)
        if broadcast_init and e.is_distributed:
            self.world_comm.broadcast(self.store.master, 0)
            self.store.sync_shadow()
        # ---- last-synced snapshot
        if offload_snapshot:
            self.sync = self.store.new_flat(device="cpu", pin=True)
            self.sync.copy_(self.store.master)
        else:
            self.sync = self.store.master.clone()
        self.timer = StepTimer(self.store.device)
        self.local_step = 0
        self.outer_step_count = 0
        # ---- the one place that tells the transports apart
        if self.lowrank:
            self.transport = LowRankTransport(self, self.lowrank)
        elif self.topk:
            self.transport = TopKTransport(self, self.topk, comm_dtype)
        elif qbits:
            self.transport = QuantisedTransport(self, qbits, self.error_feedback)
        elif fragments:
            self.transport = StreamingTransport(self, comm_dtype, self.fragments, fragment_pattern,
                                                self.stream_overlap, self.stream_alpha)
        else:
            self.transport = DenseTransport(self, comm_dtype, overlap)

    # ------------------------------------------------------------------ reference API
    def __call__(self, *args, **kwargs):
        return self.model(*args, **kwargs)

    def train(self):
        self.model.train()

    def eval(self):
        self.model.eval()

    @property
    def avg_sync_time(self) -> float:
        """Mean wall seconds per outer step (host view, includes the device wait when not overlapped)."""
        return self.timer.wall / self.timer.calls if self.timer.calls > 0 else 0.0

    @property
    def bytes_per_outer_step(self) -> int:
        """Pseudo-gradient payload each GPU contributes to the outer all-reduce."""
        return self.transport.bytes_per_step if self.outer_comm.enabled else 0

    def comm_ms(self) -> float:
        """Device time of the last outer step (HIP events on the compute stream, from the pseudo-
        gradient kernel to the last outer-Nesterov / all-gather: i.e. everything the outer step
        costs the compute stream, collectives included; syncs on the end event)."""
        if not self.timer.events:
            return 0.0
        s, e = self.timer.events[-1]
        e.synchronize()
        return s.elapsed_time(e)

    @property
    def buckets_per_outer_step(self) -> int:
        """Number of all-reduce calls one outer step issues (the reference issues one per tensor)."""
        return self.transport.buckets_per_step if self.outer_comm.enabled else 0

    def current_lr(self) -> float:
        return self.scheduler.lr()

    _TRANSPORT_NAMES = ("delta", "qbits", "qef_send", "qef_reduce", "error_feedback_state", "frag_tables", "frag_steps",
                        "fragment_sync_count", "topk_residual", "lowrank_residual", "lowrank_q")

    def __getattr__(self, name):
        """Read-only forwards of the active transport's public state (absent where that transport has none)."""
        if name in Diloco._TRANSPORT_NAMES and "transport" in self.__dict__:
            return getattr(self.transport, name)
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    # ------------------------------------------------------------------ inner step
    def inner_step(self):
        """clip(1.0) + AdamW at the scheduled lr, advance the schedule, zero grads."""
        lr = self.scheduler.lr()
        self.inner_optimizer.step(lr)
        if getattr(self.model, "fp8", None) is not None:
            self.model.fp8.recipe.update()  # fp8 delayed scaling: roll amax history once per inner step
        self.scheduler.step()
        self.store.zero_grad()
        self.local_step += 1
        if self.overlap:  # overlapped outer step from the previous boundary
            self.transport.finalize()
        if self.debug_checks and self.env.inner_dp > 1:
            self.check_inner_replicas()

    # ------------------------------------------------------------------ outer step
    def outer_step(self, phases: bool = False):
        """One outer step.  ``phases=True`` (diagnostics, e.g. bench.py --full after its timed window) runs it
        serialized -- every bucket's all-reduce completes before the first Nesterov update -- and
        records HIP events between the phases, so :meth:`outer_phase_ms` can split the step into
        pseudo-gradient / collective / outer-update time; the default pipelines buckets instead."""
        self.transport.step(phases)

    def outer_phase_ms(self) -> dict:
        """Device time of the last ``outer_step(phases=True)``: pseudo-gradient kernel, bucketed
        all-reduce (from the compute stream's view: issue to last bucket done), outer Nesterov update
        (+ the two-level all-gathers).  Empty if no phased step ran."""
        m = self.timer.phase_marks
        if not m:
            return {}
        m[-1].synchronize()
        return {"pseudograd_ms": m[0].elapsed_time(m[1]), "allreduce_ms": m[1].elapsed_time(m[2]),
                "outer_update_ms": m[2].elapsed_time(m[3])}

    def _after_update(self, sync, sh_full, ev0, t_from):
        """What follows the per-bucket updates of an outer step, whatever the transport."""
        opt, master = self.outer_optimizer, self.store.master
        opt.step_count += 1
        self.store.version += 1
        # own RCCL: a watchdog abort still completes the collective's event, so the update above may have
        # consumed a partial reduction -- fail before anything builds on it (c10d raises in Work.wait)
        self.outer_comm.check("the outer update")
        if self.env.inner_dp > 1:
            # every GPU of the worker updated its shard; replicate master and snapshot
            self.inner_comm.all_gather_flat(master, self.shards, self.env.inner_rank)
            self.inner_comm.all_gather_flat(sync, self.shards, self.env.inner_rank)
            if sh_full is not None:
                for j, (x, y) in enumerate(self.shards):
                    if j != self.env.inner_rank:
                        sh_full[x:y].copy_(master[x:y])
        if self.offload_snapshot:
            self.sync.copy_(sync, non_blocking=True)
        self.timer.stop(ev0, t_from)
        if self.debug_checks:
            self.check_replicas()

    def stream_step(self, t: int) -> Optional[dict]:
        """Streaming mode (:meth:`.transports.StreamingTransport.stream_step`): call after inner step ``t``."""
        return self.transport.stream_step(t)

    def flush_fragments(self):
        """End of a streaming run (:meth:`.transports.StreamingTransport.flush`); nothing to do otherwise."""
        self.transport.flush()

    def _sync_on_device(self) -> torch.Tensor:
        if not self.offload_snapshot:
            return self.sync
        dev = self.store.master.new_empty(self.store.numel)
        dev.copy_(self.sync, non_blocking=True)
        return dev

    def finalize(self):
        """Apply a still-pending overlapped outer step or fragment (end of training / before checkpoint)."""
        self.transport.finalize()

    # ------------------------------------------------------------------ debug
    @staticmethod
    def _checksum_spread(x: torch.Tensor, group) -> torch.Tensor:
        """MAX-MIN over ``group`` of two order-sensitive fp64 checksums of ``x``."""
        import torch.distributed as dist
        xd = x.double()
        w = torch.arange(1, x.numel() + 1, device=x.device, dtype=torch.float64).remainder(7)
        v = torch.stack([xd.sum(), (xd * w).sum()])
        mx, mn = v.clone(), v.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=group)
        dist.all_reduce(mn, op=dist.ReduceOp.MIN, group=group)
        return (mx - mn).abs()

    @torch.no_grad()
    def check_replicas(self, tol: float = 0.0):
        """Replica-consistency assertions, run after every outer step with
        ``debug_checks``:

        * theta_sync is identical on every rank of the job;
        * the GPUs of one DiLoCo worker (inner DDP) hold identical master weights;
        * without the overlapped outer step, the master weights equal theta_sync everywhere.
        (In the overlapped mode, and in the streaming mode until ``flush_fragments``, the local weights
        legitimately differ across workers by each worker's in-flight inner progress.)"""
        if not self.env.is_distributed:
            return
        spread = self._checksum_spread(self.sync.to(self.store.device), None)
        if spread.max().item() > tol:
            raise RuntimeError(f"DiLoCo replicas diverged: theta_sync checksum spread {spread.tolist()}")
        self.check_inner_replicas(tol)
        if not self.transport.local_weights_differ:
            spread = self._checksum_spread(self.store.master, None)
            if spread.max().item() > tol:
                raise RuntimeError(f"DiLoCo replicas diverged: master checksum spread {spread.tolist()}")

    @torch.no_grad()
    def check_inner_replicas(self, tol: float = 0.0):
        """The K GPUs of one DiLoCo worker apply the same all-reduced gradient every inner step, so
        their master weights must stay bit-identical (run after every inner step with
        ``debug_checks`` when ``inner_dp > 1``)."""
        if self.env.inner_dp <= 1:
            return
        spread = self._checksum_spread(self.store.master, self.env.inner_group)
        if spread.max().item() > tol:
            raise RuntimeError(f"inner-DDP replicas diverged inside worker {self.env.worker}: "
                               f"master checksum spread {spread.tolist()}")

    # ------------------------------------------------------------------ checkpoint state
    def state_dict(self):
        """The state that does not depend on the transport (the rest: ``transport.rank_state`` / ``shared_state``)."""
        self.finalize()
        return {
            "sync": self.sync,
            "outer": self.outer_optimizer.state_dict(),
            "inner": self.inner_optimizer.state_dict(),
            "scheduler": self.scheduler.state_dict(),
            "local_step": self.local_step,
            "outer_step_count": self.outer_step_count,
        }

    def load_state_dict(self, d):
        """Restore the outer state (``inner`` is optional: the checkpoint keeps AdamW state per rank)."""
        self.sync.copy_(d["sync"])
        self.outer_optimizer.load_state_dict(d["outer"])
        if "inner" in d:
            self.inner_optimizer.load_state_dict(d["inner"])
        self.scheduler.load_state_dict(d["scheduler"])
        self.local_step = int(d["local_step"])
        self.outer_step_count = int(d["outer_step_count"])
