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

Extensions (north star):
* ``comm_dtype=bf16``: pseudo-gradients travel in bf16 (half the bytes / outer step);
* ``comm_dtype="int8"`` / ``"int4"`` (``torch.int8`` = ``"int8"``): block-quantised transport, a quarter /
  an eighth of the fp32 bytes.  Integers with per-block scales cannot be all-reduced, so the step becomes
  ``nd_pseudograd_q`` -> all-to-all -> ``nd_qreduce`` -> all-gather -> ``nd_outer_nesterov_q`` per bucket
  (a quantised reduce-scatter + all-gather, docs/DESIGN.md §4).  Stateless by default; ``error_feedback=True``
  keeps two fp32 residuals per GPU -- ``qef_send`` (what this worker's codes did not deliver, one element per
  element of the owned span) and ``qef_reduce`` (the same for the chunk it requantises, per bucket) -- adds them
  before the next step's quantisation (``nd_pseudograd_q_ef`` / ``nd_qreduce_ef``) and stores them in the
  per-rank checkpoint files.  Not with ``overlap=True`` yet;
* ``overlap=True``: the all-reduce is launched at the boundary and overlaps the next inner step;
  it is applied one step late as theta <- theta_outer + (theta_local_now - theta_local_boundary)
  (the DELAYED outer update: one burst, one step late).  ``overlap=False`` is bit-faithful to the reference order;
* ``fragments=P`` (Streaming DiLoCo, Douillard et al. 2025; ``parallel/fragments.py``, docs/DESIGN.md §4): the
  model is cut into P fragments of whole layers, fragment p is sent after inner step t when
  ``t % H == ((p+1)*H // P) % H`` (peak bytes 1/P of the burst), its all-reduce overlaps ``stream_overlap`` = tau
  inner steps, and the result is merged into the drifting local weights as
  ``(1 - alpha) * theta_new + alpha * theta_local`` (``stream_alpha``).  One ``nd_frag_pseudograd`` and one
  ``nd_frag_outer_mix`` launch per fragment sync (csrc/stream_outer.hip), each fragment with its own momentum
  history and ``first`` flag.  Driven by :meth:`Diloco.stream_step`; not with ``overlap``, the quantised
  transports, ``offload_snapshot`` or ``inner_dp > 1``;
* ``inner_dp > 1`` (two-level): the W/K workers' outer all-reduce is sharded over the K GPUs of a
  worker (each reduces 1/K of the pseudo-gradient over its outer group, then the worker
  all-gathers the updated weights), so cross-worker bytes per GPU drop by K.
"""
from __future__ import annotations

import time
from typing import Optional

import torch

from .. import ops
from ..models.llama import LlamaForCausalLM
from ..optim import FlatAdamW, FlatOuterNesterov
from ..utils.schedule import CosineWarmupSchedule
from .comm import FlatCommunicator, PendingAllReduce, plan_buckets
from .dist import DistEnv
from .fragments import PATTERNS, fragment_due, plan_fragments
from ..ops import qcomm


def quantised_bits(comm_dtype) -> int:
    """8 / 4 for the block-quantised transports (``"int8"`` or ``torch.int8``, ``"int4"``), 0 for a plain
    torch dtype (fp32 / bf16 all-reduce)."""
    if isinstance(comm_dtype, str):
        if comm_dtype in ("int8", "int4"):
            return int(comm_dtype[3:])
        raise ValueError(f"comm_dtype must be a torch dtype, 'int8' or 'int4', not {comm_dtype!r}")
    return 8 if comm_dtype == torch.int8 else 0


class _QBucket:
    """One bucket of the quantised outer step: elements [x, y) of the owned span, W chunks of c elements."""

    __slots__ = ("x", "y", "c", "send", "recv", "gath")

    def __init__(self, x, y, c, send, recv, gath):
        self.x, self.y, self.c, self.send, self.recv, self.gath = x, y, c, send, recv, gath


class Diloco:
    """Flagship DiLoCo on the flat-store Llama.  Any other ``nn.Module`` (with plain torch optimizers)
    is dispatched to :class:`~nanodiloco_amd.parallel.module_diloco.ModuleDiloco`, which has the
    reference's generic ``model.parameters()`` / ``param_groups`` contract."""

    def __new__(cls, model, *args, **kwargs):
        if not isinstance(model, LlamaForCausalLM):
            from .module_diloco import ModuleDiloco
            if kwargs.get("fragments"):
                raise ValueError("Streaming DiLoCo (fragments > 0) needs the flat-store Llama of Diloco: "
                                 "ModuleDiloco does not take the streaming options")
            if kwargs.pop("error_feedback", False):
                raise ValueError("error_feedback belongs to the quantised transport (comm_dtype int8 / int4), which "
                                 "needs the flat-store Llama of Diloco: ModuleDiloco does not take it")
            return ModuleDiloco(model, *args, **kwargs)
        return super().__new__(cls)

    def __init__(self, model: LlamaForCausalLM, inner_optimizer: FlatAdamW, outer_optimizer: FlatOuterNesterov,
                 warmup_steps: int, total_steps: int, inner_steps: int = 100, outer_steps: Optional[int] = None,
                 env: Optional[DistEnv] = None, comm_dtype: torch.dtype = torch.float32, bucket_mb: float = 128.0,
                 overlap: bool = False, offload_snapshot: bool = False, debug_checks: bool = False,
                 broadcast_init: bool = True, fragments: int = 0, fragment_pattern: str = "strided",
                 stream_overlap: int = 0, stream_alpha: float = 0.0, error_feedback: bool = False):
        self.model = model
        self.store = model.store
        self.inner_optimizer = inner_optimizer
        self.outer_optimizer = outer_optimizer
        self.inner_steps = inner_steps
        self.outer_steps = outer_steps if outer_steps is not None else max(1, total_steps // max(1, inner_steps))
        self.env = env or DistEnv(device=self.store.device)
        self.scheduler = CosineWarmupSchedule(inner_optimizer.lr, warmup_steps, total_steps)
        self.qbits = quantised_bits(comm_dtype)  # 0: fp32 / bf16 transport
        if self.qbits and overlap:
            raise ValueError("quantised transport (comm_dtype int8 / int4) does not support overlap=True yet: the "
                             "delayed application and its pending-state checkpoint need the fp32 / bf16 path")
        if error_feedback and not self.qbits:
            raise ValueError("error_feedback=True (--comm-error-feedback) needs the quantised transport: comm_dtype "
                             f"'int8' or 'int4', not {comm_dtype}")
        self.error_feedback = bool(error_feedback)
        self.comm_dtype = comm_dtype
        self.overlap = overlap
        self.offload_snapshot = offload_snapshot
        self.debug_checks = debug_checks
        self.fragments = int(fragments)
        self.fragment_pattern = fragment_pattern
        self.stream_overlap = int(stream_overlap)
        self.stream_alpha = float(stream_alpha)
        if self.fragments:
            self._check_streaming(model.config.num_hidden_layers)
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
        a, b = self.my_shard
        if self.qbits:
            # the fp32 pseudo-gradient is never materialised: it is quantised in registers into the wire buffers
            self.delta = torch.zeros(0, dtype=torch.float32, device=self.store.device)
            self._qplan = self._plan_quantised(b - a)
            if self.error_feedback:
                # fp32 residuals, zero at the start: one element per owned element, and one chunk per bucket (a
                # single allocation, bucket i's view at _qef_views[i]) for the chunk this worker requantises
                dev = self.store.device
                self.qef_send = torch.zeros(b - a, dtype=torch.float32, device=dev)
                self.qef_reduce = torch.zeros(sum(bk.c for bk in self._qplan), dtype=torch.float32, device=dev)
                self._qef_views = list(self.qef_reduce.split([bk.c for bk in self._qplan]))
        elif self.fragments:
            # ONE wire buffer, sized to the largest fragment: at most one fragment is ever in flight
            plan = plan_fragments(self.store, model.config.num_hidden_layers, self.fragments, fragment_pattern)
            self.frag_tables = [ops.SpanTable(sp, self.store.device) for sp in plan]
            self.delta = torch.zeros(max(t.total for t in self.frag_tables), dtype=comm_dtype,
                                     device=self.store.device)
        else:
            self.delta = torch.zeros(b - a, dtype=comm_dtype, device=self.store.device)
        self.drift_base = torch.zeros(b - a, dtype=torch.float32, device=self.store.device) if overlap else None
        self._pending = None
        self._sync_time = 0.0
        self._sync_calls = 0
        self._comm_events = []
        self.local_step = 0
        self.outer_step_count = 0
        # streaming state: per-fragment step counters (the `first` flag and the momentum history are per
        # fragment), the fragment in flight, the last one sent (for the byte / bucket properties)
        self.frag_steps = [0] * self.fragments
        self.fragment_sync_count = 0
        self._stream_pending = None
        self._last_frag = None
        self._flushed = True  # no fragment sent yet: local weights == theta_sync on every worker

    def _check_streaming(self, num_layers: int):
        P, H, tau, alpha = self.fragments, self.inner_steps, self.stream_overlap, self.stream_alpha
        if self.fragment_pattern not in PATTERNS:
            raise ValueError(f"fragment_pattern must be one of {PATTERNS}, not {self.fragment_pattern!r}")
        if not 1 <= P <= min(num_layers, H):
            raise ValueError(f"fragments must be in [1, min(num_layers={num_layers}, inner_steps={H})], got {P}")
        if not 0 <= tau < H // P:
            raise ValueError(f"stream_overlap must be in [0, inner_steps // fragments = {H // P}), got {tau}: a "
                             f"fragment must be applied before the next one is sent")
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"stream_alpha must be in [0, 1], got {alpha}")
        for on, what in ((self.overlap, "overlap=True (--overlap-outer)"),
                         (bool(self.qbits), "quantised transport (comm_dtype int8 / int4)"),
                         (self.offload_snapshot, "offload_snapshot=True (--offload-snapshot)"),
                         (self.env.inner_dp > 1, "inner_dp > 1 (--inner-dp)")):
            if on:
                raise ValueError(f"Streaming DiLoCo (fragments > 0) is not supported together with {what}")

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
        return self._sync_time / self._sync_calls if self._sync_calls > 0 else 0.0

    @property
    def bytes_per_outer_step(self) -> int:
        """Pseudo-gradient payload each GPU contributes to the outer all-reduce."""
        if self.qbits:  # phase-1 (all-to-all) wire bytes: codes + scales of every chunk, padding included
            return sum(bk.send.numel() for bk in self._qplan) if self.outer_comm.enabled else 0
        if self.fragments:  # the fragment sent last: the PEAK of a streaming run is what gets logged
            n = self.frag_tables[self._last_frag].total if self._last_frag is not None else 0
            return n * self.delta.element_size() if self.outer_comm.enabled else 0
        a, b = self.my_shard
        return (b - a) * torch.tensor([], dtype=self.comm_dtype).element_size() if self.outer_comm.enabled else 0

    def comm_ms(self) -> float:
        """Device time of the last outer step (HIP events on the compute stream, from the pseudo-
        gradient kernel to the last outer-Nesterov / all-gather: i.e. everything the outer step
        costs the compute stream, collectives included; syncs on the end event)."""
        if not self._comm_events:
            return 0.0
        s, e = self._comm_events[-1]
        e.synchronize()
        return s.elapsed_time(e)

    @property
    def buckets_per_outer_step(self) -> int:
        """Number of all-reduce calls one outer step issues (the reference issues one per tensor)."""
        if not self.outer_comm.enabled:
            return 0
        if self.qbits:  # each bucket issues two collectives: an all-to-all and an all-gather
            return len(self._qplan)
        if self.fragments:
            n = self.frag_tables[self._last_frag].total if self._last_frag is not None else 0
            return len(plan_buckets(0, n, self.delta.element_size(), self.outer_comm.bucket_bytes))
        a, b = self.my_shard
        return len(plan_buckets(0, b - a, self.delta.element_size(), self.outer_comm.bucket_bytes))

    def current_lr(self) -> float:
        return self.scheduler.lr()

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
        if self._pending is not None:  # overlapped outer step from the previous boundary
            self._finish_outer()
        if self.debug_checks and self.env.inner_dp > 1:
            self.check_inner_replicas()

    # ------------------------------------------------------------------ outer step
    def outer_step(self, phases: bool = False):
        """One outer step.  ``phases=True`` (diagnostics, e.g. bench.py --full after its timed window) runs it
        serialized -- every bucket's all-reduce completes before the first Nesterov update -- and
        records HIP events between the phases, so :meth:`outer_phase_ms` can split the step into
        pseudo-gradient / collective / outer-update time; the default pipelines buckets instead."""
        if self.fragments:
            raise RuntimeError("streaming mode (fragments > 0): call stream_step(t) after every inner step and "
                               "flush_fragments() at the end instead of outer_step()")
        t0 = time.perf_counter()
        cuda = self.store.device.type == "cuda"
        ev0 = torch.cuda.Event(enable_timing=True) if cuda else None
        if ev0 is not None:
            ev0.record()
        master = self.store.master
        sync = self._sync_on_device()
        a, b = self.my_shard
        if self.qbits:
            return self._outer_step_quantised(sync, ev0, t0, phases and cuda)
        ops.pseudograd(sync[a:b], master[a:b], self.delta)
        if self.overlap:
            # fp32 drift base: with bf16 transport, re-applying the local progress from the rounded
            # delta would carry its bf16 rounding error into the weights every outer step
            if self.delta.dtype == torch.float32:
                self.drift_base.copy_(self.delta)
            else:
                ops.pseudograd(sync[a:b], master[a:b], self.drift_base)
        marks = None
        if phases and cuda and not self.overlap:
            marks = [ev0, torch.cuda.Event(enable_timing=True)]
            marks[1].record()
        pend = self.outer_comm.all_reduce_async(self.delta)
        if marks is not None:
            pend.wait_all()  # serialized: the compute stream waits for every bucket here
            marks.append(torch.cuda.Event(enable_timing=True))
            marks[2].record()
        self._pending = (pend, sync, ev0, t0)
        self.outer_step_count += 1
        if not self.overlap:
            self._finish_outer()
            if marks is not None:
                marks.append(self._comm_events[-1][1])
                self._phase_marks = marks
        else:
            self._sync_time += time.perf_counter() - t0

    def outer_phase_ms(self) -> dict:
        """Device time of the last ``outer_step(phases=True)``: pseudo-gradient kernel, bucketed
        all-reduce (from the compute stream's view: issue to last bucket done), outer Nesterov update
        (+ the two-level all-gathers).  Empty if no phased step ran."""
        m = getattr(self, "_phase_marks", None)
        if not m:
            return {}
        m[-1].synchronize()
        return {"pseudograd_ms": m[0].elapsed_time(m[1]), "allreduce_ms": m[1].elapsed_time(m[2]),
                "outer_update_ms": m[2].elapsed_time(m[3])}

    def _finish_outer(self):
        pend, sync, ev0, t0 = self._pending
        t1 = time.perf_counter()
        self._pending = None
        a, b = self.my_shard
        opt = self.outer_optimizer
        first = opt.step_count == 0
        master, shadow, mom = self.store.master, self.store.shadow, opt.momentum_buffer
        inv_w = 1.0 / max(1, self.env.num_workers)
        sh_full = shadow if shadow.data_ptr() != master.data_ptr() else None
        for i, (x, y) in enumerate(pend.ranges):
            pend.wait(i)  # compute stream waits for bucket i only
            ga, gb = a + x, a + y
            ops.outer_nesterov(master[ga:gb], sync[ga:gb], self.delta[x:y], mom[ga:gb],
                               sh_full[ga:gb] if sh_full is not None else None, inv_w, opt.lr, opt.momentum,
                               first, drift_base=self.drift_base[x:y] if self.overlap else None)
        self._after_update(sync, sh_full, ev0, t1 if self.overlap else t0)

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
        if ev0 is not None:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record()
            self._comm_events = [(ev0, ev1)]
        self._sync_time += time.perf_counter() - t_from
        self._sync_calls += 1
        if self.debug_checks:
            self.check_replicas()

    # ------------------------------------------------------------------ quantised transport
    def _plan_quantised(self, length: int) -> list:
        """Buckets of the span this GPU owns, in elements: each a multiple of W*256 (W chunks of whole
        quantisation blocks) except the last, which is padded in its wire buffers.  Per bucket three
        persistent uint8 wire buffers of W chunks: ``send`` (this worker's quantised delta, chunk w for worker
        w), ``recv`` (chunk ``worker`` of every worker) and ``gath`` (the reduced chunks of all workers)."""
        w = max(1, self.env.num_workers)
        bits, unit = self.qbits, w * qcomm.QBLOCK
        per = max(unit, (self.outer_comm.bucket_bytes * 8 // bits) // unit * unit)
        dev = self.store.device
        plan = []
        for x, y in plan_buckets(0, length, 1, per, align=unit):
            c = qcomm.chunk_elems(y - x, w)
            nbytes = w * qcomm.chunk_bytes(c, bits)
            plan.append(_QBucket(x, y, c, *(torch.zeros(nbytes, dtype=torch.uint8, device=dev) for _ in range(3))))
        return plan

    def _outer_step_quantised(self, sync, ev0, t0, phases: bool):
        """int8 / int4 transport: per bucket quantise -> all-to-all -> dequantise, sum, requantise ->
        all-gather -> update.  Every bucket's quantise + all-to-all is issued first, then each bucket is
        reduced and its all-gather issued, then each bucket is updated while the next one is still being
        gathered; the host never blocks (GPU).  EVERY worker, the owner of a chunk included, updates from
        the gathered bytes, so theta_sync and the master stay bit-identical across workers.  With
        ``error_feedback`` the two quantising ops are their ``_ef`` forms, which carry ``qef_send`` /
        ``qef_reduce``; nothing else in the step changes."""
        e, opt, bits = self.env, self.outer_optimizer, self.qbits
        w, r = max(1, e.num_workers), e.worker
        a, _ = self.my_shard
        master, shadow, mom = self.store.master, self.store.shadow, opt.momentum_buffer
        sh_full = shadow if shadow.data_ptr() != master.data_ptr() else None
        first = opt.step_count == 0
        inv_w = 1.0 / w
        comm = self.outer_comm
        ef = self.error_feedback

        def mark():
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            return ev

        exchanged = []
        for bk in self._qplan:
            ga, gb = a + bk.x, a + bk.y
            if ef:
                ops.pseudograd_q_ef(sync[ga:gb], master[ga:gb], self.qef_send[bk.x:bk.y], bk.send, w, bk.c, bits)
            else:
                ops.pseudograd_q(sync[ga:gb], master[ga:gb], bk.send, w, bk.c, bits)
            exchanged.append(comm.all_to_all_async(bk.send, bk.recv))
        marks = [ev0, mark()] if phases else None
        gathered = []
        for i, (bk, work) in enumerate(zip(self._qplan, exchanged)):
            work.wait()
            pb = bk.send.numel() // w
            if ef:
                ops.qreduce_ef(bk.recv, w, bk.c, bits, self._qef_views[i], bk.gath[r * pb:(r + 1) * pb])
            else:
                ops.qreduce(bk.recv, w, bk.c, bits, bk.gath[r * pb:(r + 1) * pb])
            gathered.append(comm.all_gather_async(bk.gath, r))
        if phases:
            for work in gathered:
                work.wait()  # serialized: the compute stream waits for every bucket here
            marks.append(mark())
        self.outer_step_count += 1
        for bk, work in zip(self._qplan, gathered):
            work.wait()
            ga, gb = a + bk.x, a + bk.y
            ops.outer_nesterov_q(master[ga:gb], sync[ga:gb], bk.gath, w, bk.c, bits, mom[ga:gb],
                                 sh_full[ga:gb] if sh_full is not None else None, inv_w, opt.lr, opt.momentum, first)
        self._after_update(sync, sh_full, ev0, t0)
        if phases:
            marks.append(self._comm_events[-1][1])
            self._phase_marks = marks

    def error_feedback_state(self) -> Optional[dict]:
        """The residuals of the quantised transport for a checkpoint (per rank): ``send`` / ``reduce`` and what
        they are indexed by -- ``bits``, ``num_workers`` and the bucket ``plan`` ``[[x, y, c], ...]``.  None
        without ``error_feedback``."""
        if not self.error_feedback:
            return None
        return {"send": self.qef_send, "reduce": self.qef_reduce, "bits": self.qbits,
                "num_workers": max(1, self.env.num_workers), "plan": [[bk.x, bk.y, bk.c] for bk in self._qplan]}

    def load_error_feedback_state(self, send: Optional[torch.Tensor], reduce: Optional[torch.Tensor],
                                  meta: Optional[dict]) -> list:
        """Restore the residuals saved by :meth:`error_feedback_state`; returns the lines worth logging.

        * no saved residuals (a stateless checkpoint, or a worker the checkpoint did not have): both start at zero;
        * ``send`` is indexed by element of the owned span: restored whenever its length matches, also across
          int8 <-> int4 (it is an fp32 amount still owed, whatever step size it was measured with);
        * ``reduce`` is indexed by bucket and chunk: restored only when the saved ``plan`` and ``num_workers``
          equal this run's, else zero (an elastic resume always changes the plan);
        * without ``error_feedback`` saved residuals are ignored.

        A dropped residual costs at most half a quantisation step per element, once: it is the part of earlier
        pseudo-gradients that would have been delivered later, and nothing else depends on it."""
        if not self.error_feedback:
            return ["checkpoint holds error-feedback residuals; this run has no --comm-error-feedback: ignored"] \
                if send is not None or reduce is not None else []
        notes = []
        self.qef_send.zero_()
        self.qef_reduce.zero_()
        if send is None and reduce is None:
            return ["no error-feedback residuals in the checkpoint for this rank: starting from zero"]
        if send is not None and send.numel() == self.qef_send.numel():
            self.qef_send.copy_(send)
        elif send is not None:
            notes.append(f"qef.send has {send.numel()} elements, this rank owns {self.qef_send.numel()}: starting "
                         f"from zero")
        mine = self.error_feedback_state()
        same = meta is not None and int(meta.get("num_workers", -1)) == mine["num_workers"] \
            and [list(map(int, p)) for p in meta.get("plan", [])] == mine["plan"]
        if reduce is not None and same and reduce.numel() == self.qef_reduce.numel():
            self.qef_reduce.copy_(reduce)
        elif reduce is not None:
            notes.append("qef.reduce was saved for another bucket plan or worker count: starting from zero")
        return notes

    # ------------------------------------------------------------------ streaming DiLoCo
    def stream_step(self, t: int) -> Optional[dict]:
        """Streaming mode: call after inner step ``t`` (1-based).  Applies the fragment whose overlap window ends
        here (sent after step ``t - tau``), then sends the fragment that is due after step ``t`` (and, with
        ``tau = 0``, applies it in the same call).  Returns ``{"sent": p or None, "applied": p or None}`` when
        anything happened, else None."""
        if not self.fragments:
            raise RuntimeError("stream_step needs fragments > 0")
        applied = sent = None
        if self._stream_pending is not None and t >= self._stream_pending["apply_step"]:
            applied = self._apply_fragment(self.stream_alpha)
        p = fragment_due(t, self.inner_steps, self.fragments)
        if p is not None:
            self._send_fragment(p, t + self.stream_overlap)
            sent = p
            if self.stream_overlap == 0:
                applied = self._apply_fragment(self.stream_alpha)
        if sent is None and applied is None:
            return None
        return {"sent": sent, "applied": applied}

    def _send_fragment(self, p: int, apply_step: int):
        if self._stream_pending is not None:  # tau < H // P keeps the windows apart
            raise RuntimeError(f"fragment {self._stream_pending['fragment']} is still in flight")
        t0 = time.perf_counter()
        cuda = self.store.device.type == "cuda"
        ev0 = torch.cuda.Event(enable_timing=True) if cuda else None
        if ev0 is not None:
            ev0.record()
        table = self.frag_tables[p]
        wire = self.delta[:table.total]
        ops.frag_pseudograd(self.sync, self.store.master, table, wire)
        pend = self.outer_comm.all_reduce_async(wire)
        self._stream_pending = {"fragment": p, "apply_step": apply_step, "pend": pend, "ev0": ev0}
        self._last_frag = p
        self._flushed = False
        self.fragment_sync_count += 1
        self._sync_time += time.perf_counter() - t0

    def _apply_fragment(self, alpha: float, count_round: bool = True) -> int:
        t0 = time.perf_counter()
        st, self._stream_pending = self._stream_pending, None
        p, pend, ev0 = st["fragment"], st["pend"], st["ev0"]
        if ev0 is not None and self.stream_overlap > 0:
            # the window in between belongs to the inner steps: time the apply alone
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record()
        pend.wait_all()  # the compute stream waits for this fragment's buckets
        opt, store = self.outer_optimizer, self.store
        table = self.frag_tables[p]
        ops.frag_outer_mix(store.master, self.sync, self.delta[:table.total], opt.momentum_buffer, store.shadow,
                           table, 1.0 / max(1, self.env.num_workers), opt.lr, opt.momentum, self.frag_steps[p] == 0,
                           alpha)
        self.frag_steps[p] += 1
        self.outer_comm.check("the fragment update")
        store.version += 1
        if count_round and p == self.fragments - 1:  # a round is complete
            self.outer_step_count += 1
            opt.step_count += 1
        if ev0 is not None:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record()
            self._comm_events = [(ev0, ev1)]
        self._sync_time += time.perf_counter() - t0
        self._sync_calls += 1
        if self.debug_checks:
            self.check_replicas()
        return p

    def flush_fragments(self):
        """End of a streaming run: apply a pending fragment, then send and apply every fragment once with
        tau = 0 and alpha = 0, so ``master == sync`` and all replicas are identical (an export-ready model).
        The extra syncs do not count as outer steps."""
        if not self.fragments:
            return
        if self._stream_pending is not None:
            self._apply_fragment(self.stream_alpha)
        for p in range(self.fragments):
            self._send_fragment(p, 0)
            self._apply_fragment(0.0, count_round=False)
        self._flushed = True

    @property
    def streaming_local_weights(self) -> bool:
        """Streaming mode between the first send and :meth:`flush_fragments`: every worker's local weights
        carry its own inner progress (checkpoints keep them per rank and are not export-ready)."""
        return bool(self.fragments) and not self._flushed

    def pending_stream_state(self) -> Optional[dict]:
        """The fragment in flight (a checkpoint inside its overlap window): the compute stream waits for its
        all-reduce and the reduced packed buffer is returned WITHOUT applying it; None when nothing is pending."""
        if self._stream_pending is None:
            return None
        st = self._stream_pending
        st["pend"].wait_all()
        return {"delta": self.delta[:self.frag_tables[st["fragment"]].total], "fragment": st["fragment"],
                "apply_step": st["apply_step"]}

    def restore_pending_stream(self, delta: torch.Tensor, fragment: int, apply_step: int):
        """Re-arm the fragment saved by :meth:`pending_stream_state` (its all-reduce already done)."""
        table = self.frag_tables[fragment]
        wire = self.delta[:table.total]
        wire.copy_(delta)
        ranges = plan_buckets(0, table.total, wire.element_size(), self.outer_comm.bucket_bytes)
        self._stream_pending = {"fragment": int(fragment), "apply_step": int(apply_step),
                                "pend": PendingAllReduce([None] * len(ranges), ranges, wire), "ev0": None}
        self._last_frag = int(fragment)
        self._flushed = False

    def streaming_config(self) -> Optional[dict]:
        if not self.fragments:
            return None
        return {"fragments": self.fragments, "pattern": self.fragment_pattern, "overlap": self.stream_overlap,
                "alpha": self.stream_alpha}

    def _sync_on_device(self) -> torch.Tensor:
        if not self.offload_snapshot:
            return self.sync
        dev = self.store.master.new_empty(self.store.numel)
        dev.copy_(self.sync, non_blocking=True)
        return dev

    def finalize(self):
        """Apply a still-pending overlapped outer step (end of training / before checkpoint)."""
        if self._pending is not None:
            self._finish_outer()
        if self._stream_pending is not None:
            self._apply_fragment(self.stream_alpha)

    def pending_outer_state(self) -> Optional[dict]:
        """An overlapped outer step that is still in flight (a checkpoint between the boundary and its
        one-step-late application): the compute stream waits for its all-reduce, and the reduced
        pseudo-gradient plus this rank's drift base are returned WITHOUT applying the step, so a run
        resumed from the checkpoint applies it at the same point as the uninterrupted run.  None when
        nothing is pending (always, without ``overlap``)."""
        if self._pending is None:
            return None
        self._pending[0].wait_all()
        return {"delta": self.delta, "drift_base": self.drift_base}

    def restore_pending_outer(self, delta: torch.Tensor, drift_base: torch.Tensor):
        """Re-arm the pending outer step saved by :meth:`pending_outer_state` (its all-reduce already
        done): the next :meth:`inner_step` applies it."""
        if not self.overlap:
            raise RuntimeError("checkpoint holds a pending overlapped outer step: resume with --overlap-outer")
        self.delta.copy_(delta)
        self.drift_base.copy_(drift_base)
        ranges = plan_buckets(0, self.delta.numel(), self.delta.element_size(), self.outer_comm.bucket_bytes)
        self._pending = (PendingAllReduce([None] * len(ranges), ranges, self.delta), self._sync_on_device(), None,
                         time.perf_counter())

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
        if not self.overlap and self._pending is None and not self.streaming_local_weights:
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
        self.finalize()
        return {
            "sync": self.sync,
            "outer": self.outer_optimizer.state_dict(),
            "inner": self.inner_optimizer.state_dict(),
            "scheduler": self.scheduler.state_dict(),
            "local_step": self.local_step,
            "outer_step_count": self.outer_step_count,
            "frag_steps": list(self.frag_steps),
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
        if self.fragments and "frag_steps" in d:
            self.frag_steps = [int(x) for x in d["frag_steps"]]
