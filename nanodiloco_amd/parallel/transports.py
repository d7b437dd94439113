"""The five ways :class:`~nanodiloco_amd.parallel.diloco.Diloco` moves its pseudo-gradient.  Each transport owns
its wire buffers, its protocol and the part of a checkpoint that only it understands; ``Diloco`` builds exactly
one (``Diloco.transport``) and keeps what does not depend on it: the snapshot, the counters, the communicators,
``_after_update`` and the :class:`StepTimer`.

What ``Diloco`` and ``utils/checkpoint.py`` ask of a transport: ``bytes_per_step`` / ``buckets_per_step``,
``finalize()``, ``local_weights_differ``, and for checkpoints ``rank_state() -> (tensors, scalars)`` (this rank's
files), ``shared_state() -> (trainer_state.json entries, config.json flags)`` and ``load_state(per, scal, shared)
-> lines to log`` (``per`` / ``scal``: this rank's OWN files, empty for a worker the checkpoint did not have).
A transport may also have ``shared_tensors()``, saved once for all workers.  Dense, quantised, top-k and low-rank run
``step(phases)``; streaming runs ``stream_step(t)`` and ``flush()``.
"""
from __future__ import annotations

import time
from typing import Optional

import torch

from .. import ops
from ..ops import lowrank_comm, qcomm, sparse_comm
from .comm import PendingAllReduce, plan_buckets
from .fragments import fragment_due, plan_fragments

_EF_IGNORED = "checkpoint holds error-feedback residuals; this run has no --comm-error-feedback: ignored"
_TOPK_IGNORED = "checkpoint holds a top-k residual (topk.residual); this run has no --comm-topk: ignored"
_LOWRANK_IGNORED = ("checkpoint holds low-rank transport state (lowrank.residual, lowrank.q); this run has no "
                    "--comm-rank: ignored")


def quantised_bits(comm_dtype) -> int:
    """8 / 4 for the block-quantised transports (``"int8"`` or ``torch.int8``, ``"int4"``), 0 for a plain
    torch dtype (fp32 / bf16 all-reduce)."""
    if isinstance(comm_dtype, str):
        if comm_dtype in ("int8", "int4"):
            return int(comm_dtype[3:])
        raise ValueError(f"comm_dtype must be a torch dtype, 'int8' or 'int4', not {comm_dtype!r}")
    return 8 if comm_dtype == torch.int8 else 0


class StepTimer:
    """Wall time (host) and device time (HIP events on the compute stream) of the outer steps.  A step is
    ``ev0, t0 = start()`` ... ``stop(ev0, t0)``; one that ends in a later call adds the host time of its first
    part with ``pause(t0)``.  ``start(phases=True)`` also collects a mark per ``phase()`` for ``outer_phase_ms``."""

    def __init__(self, device):
        self.cuda = device.type == "cuda"
        self.wall, self.calls = 0.0, 0
        self.events = []  # [(start, end)] of the last finished step
        self.phase_marks = None
        self._marks = None

    def mark(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def start(self, phases: bool = False):
        t0 = time.perf_counter()
        ev0 = self.mark() if self.cuda else None
        self._marks = [ev0] if phases and self.cuda else None
        return ev0, t0

    @property
    def phased(self) -> bool:
        return self._marks is not None

    def phase(self):
        if self._marks is not None:
            self._marks.append(self.mark())

    def pause(self, t0: float):
        self.wall += time.perf_counter() - t0

    def stop(self, ev0, t_from: float):
        if ev0 is not None:
            self.events = [(ev0, self.mark())]
            if self._marks is not None:
                self.phase_marks, self._marks = self._marks + [self.events[-1][1]], None
        self.wall += time.perf_counter() - t_from
        self.calls += 1


class Transport:
    """The answers of a transport with no state of its own between steps (also what ``ModuleDiloco`` gives)."""

    local_weights_differ = False  # do the workers' master weights legitimately differ right now?
    qbits = 0  # 8 / 4: the quantised transport

    def error_feedback_state(self):
        return None

    def __init__(self, diloco=None):
        self.d = diloco

    def finalize(self):
        pass

    def flush(self):
        pass

    def stream_step(self, t: int):
        raise RuntimeError("stream_step needs fragments > 0")

    def rank_state(self):
        return {}, {}

    def shared_state(self):
        return {"pending_outer": False}, {}

    def shared_tensors(self):
        """Tensors that are identical on every worker and belong to this transport: rank 0 writes them next to
        theta_sync (``diloco_state.safetensors``), and ``load_state`` finds them in ``shared`` under their names."""
        return {}

    def load_state(self, per, scal, shared) -> list:
        if shared.get("pending_outer"):
            raise RuntimeError("checkpoint holds a pending overlapped outer step: resume with --overlap-outer")
        if self.d is not None and self.d.env.rank != 0:
            return []
        return ([_EF_IGNORED] if "qef.send" in per or "qef.reduce" in per else []) + \
            ([_TOPK_IGNORED] if "topk.residual" in per else []) + \
            ([_LOWRANK_IGNORED] if "lowrank.residual" in per else [])


class DenseTransport(Transport):
    """fp32 / bf16: ``nd_pseudograd`` -> bucketed async all-reduce(SUM) -> per-bucket fused ``nd_outer_nesterov``,
    which overlaps the reduction of the next bucket.  With ``overlap`` the all-reduce is launched at the boundary,
    overlaps the next inner step and is applied one step late as theta <- theta_outer + (theta_local_now -
    theta_local_boundary); until then the step is ``_pending`` and a checkpoint keeps it so (``outer.delta``,
    ``outer.drift_base`` and each rank's local ``master``)."""

    def __init__(self, diloco, comm_dtype, overlap: bool):
        super().__init__(diloco)
        a, b = diloco.my_shard
        dev = diloco.store.device
        self.overlap = overlap
        self.delta = torch.zeros(b - a, dtype=comm_dtype, device=dev)
        self.drift_base = torch.zeros(b - a, dtype=torch.float32, device=dev) if overlap else None
        self._pending = None

    @property
    def bytes_per_step(self) -> int:
        return self.delta.numel() * self.delta.element_size()

    @property
    def buckets_per_step(self) -> int:
        return len(plan_buckets(0, self.delta.numel(), self.delta.element_size(), self.d.outer_comm.bucket_bytes))

    @property
    def local_weights_differ(self) -> bool:
        return self.overlap or self._pending is not None

    def step(self, phases: bool):
        d, timer = self.d, self.d.timer
        ev0, t0 = timer.start(phases and not self.overlap)
        master = d.store.master
        sync = d._sync_on_device()
        a, b = d.my_shard
        ops.pseudograd(sync[a:b], master[a:b], self.delta)
        if self.overlap:
            # fp32 drift base: with bf16 transport, re-applying the local progress from the rounded
            # delta would carry its bf16 rounding error into the weights every outer step
            if self.delta.dtype == torch.float32:
                self.drift_base.copy_(self.delta)
            else:
                ops.pseudograd(sync[a:b], master[a:b], self.drift_base)
        timer.phase()
        pend = d.outer_comm.all_reduce_async(self.delta)
        if timer.phased:
            pend.wait_all()  # serialized: the compute stream waits for every bucket here
            timer.phase()
        self._pending = (pend, sync, ev0, t0)
        d.outer_step_count += 1
        if not self.overlap:
            self.finalize()
        else:
            timer.pause(t0)

    def finalize(self):
        """Apply the pending step: at once without ``overlap``, else after the next inner step (or at the end)."""
        if self._pending is None:
            return
        d = self.d
        pend, sync, ev0, t0 = self._pending
        t1 = time.perf_counter()
        self._pending = None
        a, b = d.my_shard
        opt = d.outer_optimizer
        first = opt.step_count == 0
        master, mom = d.store.master, opt.momentum_buffer
        inv_w = 1.0 / max(1, d.env.num_workers)
        sh_full = d.store.separate_shadow
        for i, (x, y) in enumerate(pend.ranges):
            pend.wait(i)  # compute stream waits for bucket i only
            ga, gb = a + x, a + y
            ops.outer_nesterov(master[ga:gb], sync[ga:gb], self.delta[x:y], mom[ga:gb],
                               sh_full[ga:gb] if sh_full is not None else None, inv_w, opt.lr, opt.momentum,
                               first, drift_base=self.drift_base[x:y] if self.overlap else None)
        d._after_update(sync, sh_full, ev0, t1 if self.overlap else t0)  # overlapped: wall time from the apply

    def rank_state(self):
        """An overlapped outer step that is still in flight (a checkpoint between the boundary and its
        one-step-late application): the compute stream waits for its all-reduce, and the reduced pseudo-gradient,
        this rank's drift base and its local weights (until the step lands every worker carries its own inner
        progress since the boundary; model.safetensors holds rank 0's) are saved WITHOUT applying the step, so a
        run resumed from the checkpoint applies it at the same point as the uninterrupted run."""
        if self._pending is None:
            return {}, {}
        self._pending[0].wait_all()
        return {"outer.delta": self.delta, "outer.drift_base": self.drift_base, "master": self.d.store.master}, {}

    def shared_state(self):
        pending = self._pending is not None
        return {"pending_outer": pending}, ({"nanodiloco_pending_outer_step": True} if pending else {})

    def load_state(self, per, scal, shared) -> list:
        """Re-arm the pending step saved by :meth:`rank_state` (its all-reduce already done): the next
        ``Diloco.inner_step`` applies it."""
        if not (shared.get("pending_outer") and self.overlap):
            return super().load_state(per, scal, shared)
        self.d.store.master.copy_(per["master"])
        self.delta.copy_(per["outer.delta"])
        self.drift_base.copy_(per["outer.drift_base"])
        self._pending = (PendingAllReduce.finished(self.delta, self.d.outer_comm.bucket_bytes),
                         self.d._sync_on_device(), None, time.perf_counter())
        return []


class _QBucket:
    """One bucket of the quantised outer step: elements [x, y) of the owned span, W chunks of c elements."""

    __slots__ = ("x", "y", "c", "send", "recv", "gath")

    def __init__(self, x, y, c, send, recv, gath):
        self.x, self.y, self.c, self.send, self.recv, self.gath = x, y, c, send, recv, gath


class QuantisedTransport(Transport):
    """int8 / int4 block-quantised codes, a quarter / an eighth of the fp32 bytes.  Integers with per-block scales
    cannot be all-reduced, so the step is ``nd_pseudograd_q`` -> all-to-all -> ``nd_qreduce`` -> all-gather ->
    ``nd_outer_nesterov_q`` per bucket (a quantised reduce-scatter + all-gather, docs/DESIGN.md §4); the fp32
    pseudo-gradient is never materialised, it is quantised in registers into the wire buffers.  Stateless by
    default; ``error_feedback`` keeps two fp32 residuals per GPU -- ``qef_send`` (what this worker's codes did not
    deliver, one element per element of the owned span) and ``qef_reduce`` (the same for the chunk it requantises,
    per bucket) -- adds them before the next step's quantisation (``nd_pseudograd_q_ef`` / ``nd_qreduce_ef``) and
    stores them in the per-rank checkpoint files (``qef.send``, ``qef.reduce``).  Not with ``overlap`` yet."""

    def __init__(self, diloco, bits: int, error_feedback: bool):
        super().__init__(diloco)
        self.qbits, self.error_feedback = bits, error_feedback
        a, b = diloco.my_shard
        self._qplan = self._plan_quantised(b - a)
        if error_feedback:
            # fp32 residuals, zero at the start: one element per owned element, and one chunk per bucket (a
            # single allocation, bucket i's view at _qef_views[i]) for the chunk this worker requantises
            dev = diloco.store.device
            self.qef_send = torch.zeros(b - a, dtype=torch.float32, device=dev)
            self.qef_reduce = torch.zeros(sum(bk.c for bk in self._qplan), dtype=torch.float32, device=dev)
            self._qef_views = list(self.qef_reduce.split([bk.c for bk in self._qplan]))

    @property
    def bytes_per_step(self) -> int:
        """phase-1 (all-to-all) wire bytes: codes + scales of every chunk, padding included"""
        return sum(bk.send.numel() for bk in self._qplan)

    @property
    def buckets_per_step(self) -> int:
        return len(self._qplan)  # each bucket issues two collectives: an all-to-all and an all-gather

    def _plan_quantised(self, length: int) -> list:
        """Buckets of the span this GPU owns, in elements: each a multiple of W*256 (W chunks of whole
        quantisation blocks) except the last, which is padded in its wire buffers.  Per bucket three
        persistent uint8 wire buffers of W chunks: ``send`` (this worker's quantised delta, chunk w for worker
        w), ``recv`` (chunk ``worker`` of every worker) and ``gath`` (the reduced chunks of all workers)."""
        d = self.d
        w = max(1, d.env.num_workers)
        bits, unit = self.qbits, w * qcomm.QBLOCK
        per = max(unit, (d.outer_comm.bucket_bytes * 8 // bits) // unit * unit)
        dev = d.store.device
        plan = []
        for x, y in plan_buckets(0, length, 1, per, align=unit):
            c = qcomm.chunk_elems(y - x, w)
            nbytes = w * qcomm.chunk_bytes(c, bits)
            plan.append(_QBucket(x, y, c, *(torch.zeros(nbytes, dtype=torch.uint8, device=dev) for _ in range(3))))
        return plan

    def step(self, phases: bool):
        """Per bucket quantise -> all-to-all -> dequantise, sum, requantise -> all-gather -> update.  Every
        bucket's quantise + all-to-all is issued first, then each bucket is reduced and its all-gather issued,
        then each bucket is updated while the next one is still being gathered; the host never blocks (GPU).
        EVERY worker, the owner of a chunk included, updates from the gathered bytes, so theta_sync and the
        master stay bit-identical across workers.  With ``error_feedback`` the two quantising ops are their
        ``_ef`` forms, which carry ``qef_send`` / ``qef_reduce``; nothing else in the step changes."""
        d, timer = self.d, self.d.timer
        ev0, t0 = timer.start(phases)
        sync = d._sync_on_device()
        e, opt, bits = d.env, d.outer_optimizer, self.qbits
        w, r = max(1, e.num_workers), e.worker
        a, _ = d.my_shard
        master, mom = d.store.master, opt.momentum_buffer
        sh_full = d.store.separate_shadow
        first = opt.step_count == 0
        inv_w = 1.0 / w
        comm = d.outer_comm
        ef = self.error_feedback
        exchanged = []
        for bk in self._qplan:
            ga, gb = a + bk.x, a + bk.y
            if ef:
                ops.pseudograd_q_ef(sync[ga:gb], master[ga:gb], self.qef_send[bk.x:bk.y], bk.send, w, bk.c, bits)
            else:
                ops.pseudograd_q(sync[ga:gb], master[ga:gb], bk.send, w, bk.c, bits)
            exchanged.append(comm.all_to_all_async(bk.send, bk.recv))
        timer.phase()
        gathered = []
        for i, (bk, work) in enumerate(zip(self._qplan, exchanged)):
            work.wait()
            pb = bk.send.numel() // w
            if ef:
                ops.qreduce_ef(bk.recv, w, bk.c, bits, self._qef_views[i], bk.gath[r * pb:(r + 1) * pb])
            else:
                ops.qreduce(bk.recv, w, bk.c, bits, bk.gath[r * pb:(r + 1) * pb])
            gathered.append(comm.all_gather_async(bk.gath, r))
        if timer.phased:
            for work in gathered:
                work.wait()  # serialized: the compute stream waits for every bucket here
            timer.phase()
        d.outer_step_count += 1
        for bk, work in zip(self._qplan, gathered):
            work.wait()
            ga, gb = a + bk.x, a + bk.y
            ops.outer_nesterov_q(master[ga:gb], sync[ga:gb], bk.gath, w, bk.c, bits, mom[ga:gb],
                                 sh_full[ga:gb] if sh_full is not None else None, inv_w, opt.lr, opt.momentum, first)
        d._after_update(sync, sh_full, ev0, t0)

    def error_feedback_state(self) -> Optional[dict]:
        """The residuals of the quantised transport for a checkpoint (per rank): ``send`` / ``reduce`` and what
        they are indexed by -- ``bits``, ``num_workers`` and the bucket ``plan`` ``[[x, y, c], ...]``.  None
        without ``error_feedback``."""
        if not self.error_feedback:
            return None
        return {"send": self.qef_send, "reduce": self.qef_reduce, "bits": self.qbits,
                "num_workers": max(1, self.d.env.num_workers), "plan": [[bk.x, bk.y, bk.c] for bk in self._qplan]}

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
            return [_EF_IGNORED] if send is not None or reduce is not None else []
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

    def rank_state(self):
        qef = self.error_feedback_state()
        return ({"qef.send": qef["send"], "qef.reduce": qef["reduce"]} if qef else {}), {}

    def shared_state(self):
        qef = self.error_feedback_state()
        feedback = {"comm_error_feedback": {k: qef[k] for k in ("bits", "num_workers", "plan")}} if qef else {}
        return {"pending_outer": False, **feedback}, {}

    def load_state(self, per, scal, shared) -> list:
        # refuses a pending overlapped step; a top-k or low-rank residual is not this transport's
        other = super().load_state({k: v for k, v in per.items() if k.startswith(("topk.", "lowrank."))}, scal, shared)
        send, reduce, saved = per.get("qef.send"), per.get("qef.reduce"), shared.get("comm_error_feedback")
        had = saved is not None or send is not None
        if not (had or self.error_feedback):
            return other
        lines = self.load_error_feedback_state(send, reduce, saved)
        # every rank that lost residuals the checkpoint had says so; the rest is rank 0's to log
        return other + (lines if self.d.env.rank == 0 or (self.error_feedback and had and send is None) else [])


class _TopKBucket:
    """One bucket of the top-k outer step: elements [x, y) of the owned span (whole chunks, except at the span's
    end), W slots of ``slot`` bytes back to back in ``gath``."""

    __slots__ = ("x", "y", "slot", "gath")

    def __init__(self, x, y, slot, gath):
        self.x, self.y, self.slot, self.gath = x, y, slot, gath


class TopKTransport(Transport):
    """Top-k sparse transport with error feedback (``ops/sparse_comm.py``, docs/DESIGN.md §4): of every chunk of 4096
    elements of the span this GPU owns, only the ``k`` entries of ``(sync - master) + e`` with the largest magnitude
    travel, as ``uint16`` indices with fp32 or bf16 values; ``e`` (fp32, one element per owned element, zero at the
    start) keeps what did not.  Indices differ per worker, so nothing can be reduced on the way: the step is
    ``nd_pseudograd_topk`` -> all-gather of the W slots -> ``nd_outer_nesterov_topk`` per bucket, and EVERY worker,
    the sender included, updates from the gathered bytes in worker order, so theta_sync and the master stay
    bit-identical across workers.  The residual is this rank's checkpoint state (``topk.residual``)."""

    def __init__(self, diloco, k: int, value_dtype):
        super().__init__(diloco)
        self.k, self.value_dtype = int(k), value_dtype
        a, b = diloco.my_shard
        self.residual = torch.zeros(b - a, dtype=torch.float32, device=diloco.store.device)
        self._plan = self._plan_buckets(b - a)

    @property
    def topk_residual(self) -> torch.Tensor:
        return self.residual

    @property
    def bytes_per_step(self) -> int:
        """this worker's slots (what it contributes to the all-gathers), padding included"""
        return sum(bk.slot for bk in self._plan)

    @property
    def buckets_per_step(self) -> int:
        return len(self._plan)

    def _plan_buckets(self, length: int) -> list:
        """Runs of whole chunks whose W slots fit ``bucket_bytes`` (at least one chunk), each with one persistent
        uint8 ``gath`` buffer of W slots."""
        d = self.d
        w = max(1, d.env.num_workers)
        vs = 4 if self.value_dtype == torch.float32 else 2
        # 32: the two paddings of a slot
        chunks = max(1, (d.outer_comm.bucket_bytes // w - 32) // (self.k * (2 + vs)))
        dev = d.store.device
        plan = []
        for x, y in plan_buckets(0, length, 1, chunks * sparse_comm.CHUNK, align=sparse_comm.CHUNK):
            slot = sparse_comm.topk_slot_bytes(y - x, self.k, self.value_dtype)
            plan.append(_TopKBucket(x, y, slot, torch.zeros(w * slot, dtype=torch.uint8, device=dev)))
        return plan

    def step(self, phases: bool):
        """Every bucket's select + all-gather is issued first, then each bucket is updated while the later ones
        are still being gathered; the host never blocks (GPU)."""
        d, timer = self.d, self.d.timer
        ev0, t0 = timer.start(phases)
        sync = d._sync_on_device()
        e, opt = d.env, d.outer_optimizer
        w, r = max(1, e.num_workers), e.worker
        a, _ = d.my_shard
        master, mom = d.store.master, opt.momentum_buffer
        sh_full = d.store.separate_shadow
        first = opt.step_count == 0
        comm = d.outer_comm
        gathered = []
        for bk in self._plan:
            ga, gb = a + bk.x, a + bk.y
            ops.pseudograd_topk(sync[ga:gb], master[ga:gb], self.residual[bk.x:bk.y],
                                bk.gath[r * bk.slot:(r + 1) * bk.slot], self.k, self.value_dtype)
            gathered.append(comm.all_gather_async(bk.gath, r))
        timer.phase()
        if timer.phased:
            for work in gathered:
                work.wait()  # serialized: the compute stream waits for every bucket here
            timer.phase()
        d.outer_step_count += 1
        for bk, work in zip(self._plan, gathered):
            work.wait()
            ga, gb = a + bk.x, a + bk.y
            ops.outer_nesterov_topk(master[ga:gb], sync[ga:gb], bk.gath, w, self.k, self.value_dtype, mom[ga:gb],
                                    sh_full[ga:gb] if sh_full is not None else None, 1.0 / w, opt.lr, opt.momentum,
                                    first)
        d._after_update(sync, sh_full, ev0, t0)

    def rank_state(self):
        return {"topk.residual": self.residual}, {}

    def shared_state(self):
        name = "fp32" if self.value_dtype == torch.float32 else "bf16"
        return {"pending_outer": False,
                "comm_topk": {"k": self.k, "chunk": sparse_comm.CHUNK, "value_dtype": name}}, {}

    def load_state(self, per, scal, shared) -> list:
        """The residual is an fp32 amount still owed, indexed by element of the owned span: restored whenever its
        length matches -- k, the value dtype and the number of workers may differ --, else zero.  A rank without
        one (a checkpoint of another transport, a worker the checkpoint did not have) starts at zero."""
        lines = super().load_state({k: v for k, v in per.items() if k.startswith(("qef.", "lowrank."))}, scal, shared)
        saved = per.get("topk.residual")
        self.residual.zero_()
        if saved is None:
            if shared.get("comm_topk") is not None:  # the checkpoint had residuals, this rank has none in it
                lines.append("no top-k residual in the checkpoint for this rank: starting from zero")
        elif saved.numel() == self.residual.numel():
            self.residual.copy_(saved)
        else:
            lines.append(f"topk.residual has {saved.numel()} elements, this rank owns {self.residual.numel()}: "
                         f"starting from zero")
        return lines


class LowRankTransport(Transport):
    """Low-rank (PowerSGD) transport with error feedback (``ops/lowrank_comm.py``, docs/DESIGN.md §4): every 2-D
    tensor [m, n] with ``min(m, n) >= 4 R`` and ``n % 4 == 0`` travels as two factors P [m, R] and Q [n, R], the rest
    (norm weights, small or odd matrices) as plain fp32.  The factors are linear in the pseudo-gradient, so both are
    all-reduced and the bytes sent and received do not depend on the number of workers.  The step is
    ``nd_lowrank_project`` -> all-reduce of ``[dense | all P]`` -> ``nd_lowrank_orthonormalize`` ->
    ``nd_lowrank_backproject`` -> all-reduce of ``[all Q]`` -> ``nd_outer_nesterov_lowrank``; everything after an
    all-reduce is computed by deterministic kernels from identical bytes, so theta_sync and the master stay
    bit-identical across workers.  ``residual`` (fp32, one element per element, zero on the dense spans) is this
    rank's checkpoint state (``lowrank.residual``); ``q`` is identical on every worker and is saved once
    (``lowrank.q``); Q0 is regenerated from a constant seed and never saved."""

    def __init__(self, diloco, rank: int):
        super().__init__(diloco)
        store = diloco.store
        dev = store.device
        self.rank = int(rank)
        self.plan = lowrank_comm.LowRankPlan.from_store(store, self.rank)
        if not len(self.plan):
            raise ValueError(f"low-rank transport (lowrank > 0, --comm-rank): no tensor of this model is a matrix "
                             f"with min(m, n) >= 4 * {self.rank} and n % 4 == 0, so there is nothing to compress")
        self.residual = torch.zeros(store.numel, dtype=torch.float32, device=dev)
        self.q0 = self.plan.init_q().to(dev)
        self.q = self.q0.clone()
        w1, w2 = lowrank_comm.lowrank_wire_elems(self.plan)
        self.wire1 = torch.zeros(w1, dtype=torch.float32, device=dev)
        self.wire2 = torch.zeros(w2, dtype=torch.float32, device=dev)

    @property
    def lowrank_residual(self) -> torch.Tensor:
        return self.residual

    @property
    def lowrank_q(self) -> torch.Tensor:
        return self.q

    @property
    def bytes_per_step(self) -> int:
        """both rounds: ``[dense | all P]`` and ``[all Q]``, fp32"""
        return 4 * (self.wire1.numel() + self.wire2.numel())

    @property
    def buckets_per_step(self) -> int:
        bb = self.d.outer_comm.bucket_bytes
        return len(plan_buckets(0, self.wire1.numel(), 4, bb)) + len(plan_buckets(0, self.wire2.numel(), 4, bb))

    def step(self, phases: bool):
        """Two all-reduce rounds, each waited for before the kernel that reads it (the rounds do not overlap each
        other yet).  With ``phases`` the collective span also holds the orthonormalisation and the back-projection
        that sit between the two rounds."""
        d, timer = self.d, self.d.timer
        ev0, t0 = timer.start(phases)
        sync = d._sync_on_device()
        opt = d.outer_optimizer
        master, mom = d.store.master, opt.momentum_buffer
        sh_full = d.store.separate_shadow
        ops.lowrank_project(sync, master, self.residual, self.q, self.wire1, self.plan)
        timer.phase()
        d.outer_comm.all_reduce_async(self.wire1).wait_all()
        ops.lowrank_orthonormalize(self.wire1, self.plan)
        ops.lowrank_backproject(self.residual, self.wire1, self.wire2, self.plan)
        d.outer_comm.all_reduce_async(self.wire2).wait_all()
        timer.phase()
        d.outer_step_count += 1
        ops.outer_nesterov_lowrank(master, sync, self.residual, self.wire1, self.wire2, self.q, self.q0, mom, sh_full,
                                   self.plan, 1.0 / max(1, d.env.num_workers), opt.lr, opt.momentum,
                                   opt.step_count == 0)
        d._after_update(sync, sh_full, ev0, t0)

    def rank_state(self):
        return {"lowrank.residual": self.residual}, {}

    def shared_state(self):
        return {"pending_outer": False, "comm_lowrank": {"rank": self.rank, "seed": lowrank_comm.Q_SEED}}, {}

    def shared_tensors(self):
        return {"lowrank.q": self.q}

    def load_state(self, per, scal, shared) -> list:
        """The residual is an fp32 amount still owed, indexed by element: restored whenever its length matches --
        the rank may differ --, else zero.  Q is restored when the saved rank, seed and length equal this run's (the
        table follows from the model and the rank), else it starts from Q0 again.  Q is the same on every worker, so
        what concerns it is rank 0's to log."""
        lines = super().load_state({k: v for k, v in per.items() if k.startswith(("qef.", "topk."))}, scal, shared)
        meta, first = shared.get("comm_lowrank"), self.d.env.rank == 0
        same = meta is not None and int(meta.get("rank", -1)) == self.rank \
            and int(meta.get("seed", -1)) == lowrank_comm.Q_SEED
        saved = per.get("lowrank.residual")
        self.residual.zero_()
        if saved is None:
            if meta is not None:  # the checkpoint had residuals, this rank has none in it
                lines.append("no low-rank residual in the checkpoint for this rank: starting from zero")
        elif saved.numel() == self.residual.numel():
            self.residual.copy_(saved)
            if not same and first:
                lines.append(f"lowrank.residual was left by rank {meta.get('rank') if meta else '?'}, this run has "
                             f"rank {self.rank}: kept, it is an amount still owed")
        else:
            lines.append(f"lowrank.residual has {saved.numel()} elements, this rank owns {self.residual.numel()}: "
                         f"starting from zero")
        qs = shared.get("lowrank.q")
        self.q.copy_(self.q0)
        if same and qs is not None and qs.numel() == self.q.numel():
            self.q.copy_(qs)
        elif meta is not None and first:
            lines.append(f"lowrank.q was saved for rank {meta.get('rank')}, this run has rank {self.rank}: "
                         f"re-seeded from the constant seed")
        return lines


class StreamingTransport(Transport):
    """Streaming DiLoCo (Douillard et al. 2025; ``parallel/fragments.py``, docs/DESIGN.md §4): the model is cut
    into P fragments of whole layers, fragment p is sent after inner step t when ``t % H == ((p+1)*H // P) % H``
    (peak bytes 1/P of the burst), its all-reduce overlaps ``stream_overlap`` = tau inner steps, and the result is
    merged into the drifting local weights as ``(1 - alpha) * theta_new + alpha * theta_local`` (``stream_alpha``).
    One ``nd_frag_pseudograd`` and one ``nd_frag_outer_mix`` launch per fragment sync (csrc/stream_outer.hip), each
    fragment with its own momentum history and ``first`` flag (``frag_steps``).  ONE wire buffer, sized to the
    largest fragment: at most one fragment is ever in flight.  A checkpoint keeps every rank's local ``master``
    and, inside an overlap window, the reduced ``stream.delta`` with its fragment and apply step."""

    def __init__(self, diloco, comm_dtype, fragments: int, pattern: str, overlap: int, alpha: float):
        super().__init__(diloco)
        self.fragments, self.pattern, self.overlap, self.alpha = fragments, pattern, overlap, alpha
        store = diloco.store
        plan = plan_fragments(store, diloco.model.config.num_hidden_layers, fragments, pattern)
        self.frag_tables = [ops.SpanTable(sp, store.device) for sp in plan]
        self.delta = torch.zeros(max(t.total for t in self.frag_tables), dtype=comm_dtype, device=store.device)
        self.frag_steps = [0] * fragments
        self.fragment_sync_count = 0
        self._stream_pending = None  # the fragment in flight
        self._last_frag = None  # the last one sent (for the byte / bucket properties)
        self._flushed = True  # no fragment sent yet: local weights == theta_sync on every worker

    @property
    def bytes_per_step(self) -> int:
        """of the fragment sent last: the PEAK of a streaming run is what gets logged"""
        n = self.frag_tables[self._last_frag].total if self._last_frag is not None else 0
        return n * self.delta.element_size()

    @property
    def buckets_per_step(self) -> int:
        n = self.frag_tables[self._last_frag].total if self._last_frag is not None else 0
        return len(plan_buckets(0, n, self.delta.element_size(), self.d.outer_comm.bucket_bytes))

    def step(self, phases: bool):
        raise RuntimeError("streaming mode (fragments > 0): call stream_step(t) after every inner step and "
                           "flush_fragments() at the end instead of outer_step()")

    def stream_step(self, t: int) -> Optional[dict]:
        """Call after inner step ``t`` (1-based).  Applies the fragment whose overlap window ends
        here (sent after step ``t - tau``), then sends the fragment that is due after step ``t`` (and, with
        ``tau = 0``, applies it in the same call).  Returns ``{"sent": p or None, "applied": p or None}`` when
        anything happened, else None."""
        applied = sent = None
        if self._stream_pending is not None and t >= self._stream_pending["apply_step"]:
            applied = self._apply_fragment(self.alpha)
        p = fragment_due(t, self.d.inner_steps, self.fragments)
        if p is not None:
            self._send_fragment(p, t + self.overlap)
            sent = p
            if self.overlap == 0:
                applied = self._apply_fragment(self.alpha)
        if sent is None and applied is None:
            return None
        return {"sent": sent, "applied": applied}

    def _send_fragment(self, p: int, apply_step: int):
        if self._stream_pending is not None:  # tau < H // P keeps the windows apart
            raise RuntimeError(f"fragment {self._stream_pending['fragment']} is still in flight")
        d = self.d
        ev0, t0 = d.timer.start()
        table = self.frag_tables[p]
        wire = self.delta[:table.total]
        ops.frag_pseudograd(d.sync, d.store.master, table, wire)
        pend = d.outer_comm.all_reduce_async(wire)
        self._stream_pending = {"fragment": p, "apply_step": apply_step, "pend": pend, "ev0": ev0}
        self._last_frag = p
        self._flushed = False
        self.fragment_sync_count += 1
        d.timer.pause(t0)

    def _apply_fragment(self, alpha: float, count_round: bool = True) -> int:
        t0 = time.perf_counter()
        d = self.d
        st, self._stream_pending = self._stream_pending, None
        p, pend, ev0 = st["fragment"], st["pend"], st["ev0"]
        if ev0 is not None and self.overlap > 0:
            ev0 = d.timer.mark()  # the window in between belongs to the inner steps: time the apply alone
        pend.wait_all()  # the compute stream waits for this fragment's buckets
        opt, store = d.outer_optimizer, d.store
        table = self.frag_tables[p]
        ops.frag_outer_mix(store.master, d.sync, self.delta[:table.total], opt.momentum_buffer, store.shadow,
                           table, 1.0 / max(1, d.env.num_workers), opt.lr, opt.momentum, self.frag_steps[p] == 0,
                           alpha)
        self.frag_steps[p] += 1
        d.outer_comm.check("the fragment update")
        store.version += 1
        if count_round and p == self.fragments - 1:  # a round is complete
            d.outer_step_count += 1
            opt.step_count += 1
        d.timer.stop(ev0, t0)
        if d.debug_checks:
            d.check_replicas()
        return p

    def finalize(self):
        if self._stream_pending is not None:
            self._apply_fragment(self.alpha)

    def flush(self):
        """End of a streaming run: apply a pending fragment, then send and apply every fragment once with
        tau = 0 and alpha = 0, so ``master == sync`` and all replicas are identical (an export-ready model).
        The extra syncs do not count as outer steps."""
        self.finalize()
        for p in range(self.fragments):
            self._send_fragment(p, 0)
            self._apply_fragment(0.0, count_round=False)
        self._flushed = True

    @property
    def streaming_local_weights(self) -> bool:
        """Between the first send and :meth:`flush`: every worker's local weights carry its own inner
        progress (checkpoints keep them per rank and are not export-ready)."""
        return not self._flushed

    local_weights_differ = streaming_local_weights

    def streaming_config(self) -> dict:
        return {"fragments": self.fragments, "pattern": self.pattern, "overlap": self.overlap, "alpha": self.alpha}

    def rank_state(self):
        """Every rank's local weights (they differ per worker until the flush) and, inside an overlap window, the
        fragment in flight: the compute stream waits for its all-reduce and the reduced packed buffer is saved
        WITHOUT applying it."""
        st = self._stream_pending
        if st is None:
            return {"master": self.d.store.master}, {}
        st["pend"].wait_all()
        return {"master": self.d.store.master, "stream.delta": self.delta[:self.frag_tables[st["fragment"]].total]}, \
            {"stream_pending_fragment": st["fragment"], "stream_apply_step": st["apply_step"]}

    def shared_state(self):
        st, local = self._stream_pending, self.streaming_local_weights
        streaming = {**self.streaming_config(), "frag_steps": list(self.frag_steps),
                     "fragment_sync_count": self.fragment_sync_count, "local_weights": local,
                     "pending_fragment": st["fragment"] if st else None,
                     "pending_apply_step": st["apply_step"] if st else None}
        # rank 0's local weights, fragments at different sync ages: not the synced model
        return {"pending_outer": False, "streaming": streaming}, \
            ({"nanodiloco_streaming_local_weights": True} if local else {})

    def load_state(self, per, scal, shared) -> list:
        streamed = shared["streaming"]  # load_checkpoint has compared the options
        self.d.store.master.copy_(per["master"])
        self.frag_steps = [int(x) for x in streamed["frag_steps"]]
        self.fragment_sync_count = int(streamed.get("fragment_sync_count", 0))
        self._flushed = not streamed.get("local_weights", True)
        if "stream.delta" in per:  # re-arm the fragment in flight (its all-reduce already done)
            p = self._last_frag = int(scal["stream_pending_fragment"])
            wire = self.delta[:self.frag_tables[p].total]
            wire.copy_(per["stream.delta"])
            self._stream_pending = {"fragment": p, "apply_step": int(scal["stream_apply_step"]), "ev0": None,
                                    "pend": PendingAllReduce.finished(wire, self.d.outer_comm.bucket_bytes)}
        return []
