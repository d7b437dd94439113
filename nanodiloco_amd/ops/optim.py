"""Flat-buffer optimizer kernels: clip + AdamW (inner, K12-K14) and the DiLoCo outer step (K15-K17).

Inner step (reference: ``clip_grad_norm_(1.0)`` then ``AdamW.step()``,
REF/nanodiloco/diloco/diloco.py:56-60):
  ``nd_sumsq_partial``  per-block sum of squares of the flat fp32 grad
  ``nd_adamw_step``     every block re-reduces the (<=1024) partials -> global norm -> clip
                        coefficient, then one fused pass: decoupled weight decay, m/v update,
                        bias-corrected step, fp32 master write AND bf16 shadow write-out.
  Two launches total, no host sync (lr / bias corrections are kernel arguments).

Outer step (reference: per-tensor pseudo-grad + all_reduce(AVG) + SGD-Nesterov + CPU snapshot,
REF/nanodiloco/diloco/diloco.py:34-54):
  ``nd_pseudograd``     delta = theta_sync - theta_local   (fp32 or bf16 wire dtype)
  -- all-reduce(SUM) of delta, bucketed, on the comm stream --
  ``nd_outer_nesterov`` one pass per bucket: buf = m*buf + delta/W (buf = delta/W on the first
                        outer step), theta = theta_sync - lr*(delta/W + m*buf), theta_sync = theta,
                        shadow = bf16(theta); optional "drift" term for the delayed (overlapped)
                        mode (see parallel/diloco.py).
  ``nd_frag_pseudograd`` / ``nd_frag_outer_mix``  the same two steps for one FRAGMENT of Streaming DiLoCo: a
                        list of 64-aligned spans of the flat vector packed into one wire buffer, one launch
                        each, plus the merge master = theta + alpha*(master - theta) (csrc/stream_outer.hip).

Every function has a PyTorch implementation with identical math (CPU path + test oracle).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

from . import _ext

SUMSQ_BLOCKS = 1024


def global_grad_norm(grad: torch.Tensor) -> torch.Tensor:
    if _ext.use_hip(grad):
        part = torch.empty(SUMSQ_BLOCKS, dtype=torch.float32, device=grad.device)
        _ext.check(_ext.lib().nd_sumsq_partial(_ext.ptr(grad), grad.numel(), _ext.ptr(part), SUMSQ_BLOCKS,
                                               _ext.stream_ptr(grad.device)), "nd_sumsq_partial")
        return part.sum().sqrt()
    return grad.float().norm()


def adamw_step(master: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
               shadow: Optional[torch.Tensor], step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
               weight_decay: float = 0.01, max_norm: Optional[float] = 1.0,
               norm_out: Optional[torch.Tensor] = None, skip_nonfinite: bool = False,
               skipped: Optional[torch.Tensor] = None) -> None:
    """Clip-by-global-norm + AdamW (torch.optim.AdamW semantics) over flat fp32 buffers.

    ``step`` is the 1-based AdamW step count (bias correction).  If ``norm_out`` is given, the
    pre-clip global grad norm is written to it (device scalar, for logging without a sync).
    ``skip_nonfinite``: if the global grad norm is NaN/Inf the update is skipped on the device (no
    host sync) and ``skipped`` (int32 device scalar) is incremented.
    """
    b1, b2 = betas
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    if _ext.use_hip(master):
        n = master.numel()
        part = torch.empty(SUMSQ_BLOCKS, dtype=torch.float32, device=master.device)
        L = _ext.lib()
        s = _ext.stream_ptr(master.device)
        need_norm = max_norm is not None or norm_out is not None or skip_nonfinite
        if need_norm:
            _ext.check(L.nd_sumsq_partial(_ext.ptr(grad), n, _ext.ptr(part), SUMSQ_BLOCKS, s), "nd_sumsq_partial")
        sh = shadow if (shadow is not None and shadow.data_ptr() != master.data_ptr()) else None
        _ext.check(L.nd_adamw_step(_ext.ptr(master), _ext.ptr(grad), _ext.ptr(exp_avg), _ext.ptr(exp_avg_sq),
                                   _ext.ptr(sh), _ext.dtcode(sh) if sh is not None else 0, n,
                                   _ext.ptr(part) if need_norm else 0,
                                   SUMSQ_BLOCKS, float(lr), float(b1), float(b2), float(eps), float(weight_decay),
                                   float(bc1), float(bc2), float(max_norm if max_norm is not None else -1.0),
                                   _ext.ptr(norm_out), 1 if skip_nonfinite else 0, _ext.ptr(skipped), s),
                   "nd_adamw_step")
        return
    # ---- torch reference (same op order as torch.optim.AdamW single-tensor path)
    g = grad
    if max_norm is not None or norm_out is not None or skip_nonfinite:
        total = grad.norm()
        if norm_out is not None:
            norm_out.copy_(total.reshape(norm_out.shape))
        if skip_nonfinite and not bool(torch.isfinite(total)):
            if skipped is not None:
                skipped += 1
            return
        if max_norm is not None:
            coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
            g = grad * coef
    _adamw_update_torch(master, g, exp_avg, exp_avg_sq, lr, b1, b2, eps, weight_decay, bc1, bc2)
    if shadow is not None and shadow.data_ptr() != master.data_ptr():
        shadow.copy_(master)


def _adamw_update_torch(master, g, exp_avg, exp_avg_sq, lr, b1, b2, eps, weight_decay, bc1, bc2) -> None:
    """The element-wise part of ``adamw_step``'s PyTorch form on an already clipped gradient (also run span by
    span by ``ops.muon.adamw_step_spans``)."""
    master.mul_(1.0 - lr * weight_decay)
    exp_avg.lerp_(g, 1.0 - b1)
    exp_avg_sq.mul_(b2).addcmul_(g, g, value=1.0 - b2)
    step_size = lr / bc1
    denom = (exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(eps)
    master.addcdiv_(exp_avg, denom, value=-step_size)


def pseudograd(sync: torch.Tensor, master: torch.Tensor, out: torch.Tensor) -> None:
    """out = sync - master (out may be fp32 or bf16)."""
    if _ext.use_hip(master):
        _ext.check(_ext.lib().nd_pseudograd(_ext.ptr(sync), _ext.ptr(master), _ext.ptr(out), _ext.dtcode(out),
                                            master.numel(), _ext.stream_ptr(master.device)), "nd_pseudograd")
        return
    torch.sub(sync, master, out=out) if out.dtype == torch.float32 else out.copy_(sync - master)


def outer_nesterov(master: torch.Tensor, sync: torch.Tensor, delta_sum: torch.Tensor, mom: torch.Tensor,
                   shadow: Optional[torch.Tensor], inv_world: float, lr: float, momentum: float, first: bool,
                   drift_base: Optional[torch.Tensor] = None) -> None:
    """Outer SGD-Nesterov step on one (bucket) range; see module docstring.

    ``drift_base`` (fp32, optional): the pre-reduce local pseudo-gradient.  When given, the local
    progress made since the outer boundary (``master - (sync - drift_base)``) is re-applied on top
    of the new outer weights (overlapped / one-step-delayed mode).
    """
    if _ext.use_hip(master):
        sh = shadow if (shadow is not None and shadow.data_ptr() != master.data_ptr()) else None
        _ext.check(_ext.lib().nd_outer_nesterov(
            _ext.ptr(master), _ext.ptr(sync), _ext.ptr(delta_sum), _ext.dtcode(delta_sum), _ext.ptr(mom),
            _ext.ptr(sh), _ext.dtcode(sh) if sh is not None else 0, master.numel(), float(inv_world), float(lr),
            float(momentum), 1 if first else 0, _ext.ptr(drift_base), 0, _ext.stream_ptr(master.device)),
            "nd_outer_nesterov")
        return
    new = _nesterov_torch(sync, delta_sum, mom, inv_world, lr, momentum, first)
    if drift_base is not None:
        master.add_(drift_base).sub_(sync).add_(new)  # new + (local - (sync_old - drift_base))
    else:
        master.copy_(new)
    sync.copy_(new)
    if shadow is not None and shadow.data_ptr() != master.data_ptr():
        shadow.copy_(master)


def _nesterov_torch(sync, delta_sum, mom, inv_world, lr, momentum, first, fused_step: bool = False) -> torch.Tensor:
    """PyTorch form of ``outer_update`` (csrc/outer_update.h): updates ``mom`` in place, returns the new theta.
    ``fused_step``: theta as ONE ``add(alpha=-lr)`` (a single rounding, what the kernel's fused multiply-add and
    ``outer_nesterov_q`` do) instead of ``outer_nesterov``'s historical ``sync - lr * upd`` (two roundings)."""
    d = delta_sum.float() * inv_world
    if first:
        mom.copy_(d)
    else:
        mom.mul_(momentum).add_(d)
    upd = d.add(mom, alpha=momentum)
    return sync.add(upd, alpha=-lr) if fused_step else sync - lr * upd


# ---------------------------------------------------------------------------------------------------------
# Streaming DiLoCo: the outer step of one fragment (a list of spans of the flat vector), csrc/stream_outer.hip
FRAG_ALIGN = 64


class SpanTable:
    """Validated span list of one fragment plus its device table.

    ``spans``: ``[(start, end), ...]`` in elements of the flat vector, in increasing order.  Every start and end
    must be a multiple of 64 (so the packed offsets are too and the kernels' 16-byte accesses stay aligned), and
    spans must be non-empty and disjoint: anything else raises ``ValueError`` here, before any launch.  The
    device table (``int64``: S rows ``(start, end)``, then the S+1 packed offsets) is built once per device."""

    def __init__(self, spans: Sequence[Tuple[int, int]], device=None):
        self.spans = [(int(a), int(b)) for a, b in spans]
        if not self.spans:
            raise ValueError("span table is empty")
        prev_end = 0
        self.offsets = [0]
        for a, b in self.spans:
            if a % FRAG_ALIGN or b % FRAG_ALIGN:
                raise ValueError(f"span [{a}, {b}) is misaligned: starts and ends must be multiples of {FRAG_ALIGN}")
            if a < 0 or b <= a:
                raise ValueError(f"span [{a}, {b}) is empty or negative")
            if a < prev_end:
                raise ValueError(f"span [{a}, {b}) overlaps or precedes the span ending at {prev_end}")
            prev_end = b
            self.offsets.append(self.offsets[-1] + (b - a))
        self.total = self.offsets[-1]
        self.end = prev_end
        self._dev = {}
        if device is not None:
            self.device_table(torch.device(device))

    def __len__(self):
        return len(self.spans)

    def device_table(self, device: torch.device) -> torch.Tensor:
        t = self._dev.get(device)
        if t is None:
            flat = [x for ab in self.spans for x in ab] + self.offsets
            t = torch.tensor(flat, dtype=torch.int64, device=device)
            self._dev[device] = t
        return t

    def packed(self):
        """``(start, end, packed_offset)`` per span."""
        return [(a, b, o) for (a, b), o in zip(self.spans, self.offsets)]


def _span_table(spans, n_flat: int, n_packed: int) -> SpanTable:
    table = spans if isinstance(spans, SpanTable) else SpanTable(spans)
    if table.end > n_flat:
        raise ValueError(f"span table ends at {table.end}, the flat buffers hold {n_flat} elements")
    if table.total > n_packed:
        raise ValueError(f"span table packs {table.total} elements, the wire buffer holds {n_packed}")
    return table


def frag_pseudograd(sync: torch.Tensor, master: torch.Tensor, spans, out: torch.Tensor) -> None:
    """``out[:total] = cat(sync[a:b] - master[a:b] for every span)``: the packed pseudo-gradient of one fragment
    (``out`` fp32 or bf16), one launch for all spans.  ``spans``: a :class:`SpanTable` or a span list."""
    table = _span_table(spans, min(sync.numel(), master.numel()), out.numel())
    if _ext.use_hip(master):
        _ext.check(_ext.lib().nd_frag_pseudograd(
            _ext.ptr(sync), _ext.ptr(master), _ext.ptr(table.device_table(master.device)), len(table), table.total,
            _ext.ptr(out), _ext.dtcode(out), _ext.stream_ptr(master.device)), "nd_frag_pseudograd")
        return
    for a, b, o in table.packed():
        pseudograd(sync[a:b], master[a:b], out[o:o + b - a])


def frag_outer_mix(master: torch.Tensor, sync: torch.Tensor, delta_packed: torch.Tensor, mom: torch.Tensor,
                   shadow: Optional[torch.Tensor], spans, inv_world: float, lr: float, momentum: float, first: bool,
                   alpha: float = 0.0) -> None:
    """Outer SGD-Nesterov step of one fragment from its packed, all-reduced pseudo-gradient, scattered back
    through the span table in one launch; then the Streaming DiLoCo merge of the local weights::

        theta = outer_update(delta / W)         (sync = theta, mom updated: exactly ``outer_nesterov``)
        master = theta + alpha * (master - theta)   (one fused rounding; alpha = 0: master = theta, not read)
        shadow = bf16(master)

    Elements outside the spans are never written."""
    n_flat = min(master.numel(), sync.numel(), mom.numel())
    sh = shadow if (shadow is not None and shadow.data_ptr() != master.data_ptr()) else None
    if sh is not None:
        n_flat = min(n_flat, sh.numel())
    table = _span_table(spans, n_flat, delta_packed.numel())
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], got {alpha}")
    if _ext.use_hip(master):
        _ext.check(_ext.lib().nd_frag_outer_mix(
            _ext.ptr(master), _ext.ptr(sync), _ext.ptr(delta_packed), _ext.dtcode(delta_packed), _ext.ptr(mom),
            _ext.ptr(sh), _ext.dtcode(sh) if sh is not None else 0, _ext.ptr(table.device_table(master.device)),
            len(table), table.total, float(inv_world), float(lr), float(momentum), 1 if first else 0, float(alpha),
            _ext.stream_ptr(master.device)), "nd_frag_outer_mix")
        return
    # on the GPU this path is the kernel's twin (--ops torch), so theta takes the kernel's single rounding; on the
    # CPU it keeps outer_nesterov's order, so that one fragment over the whole vector IS the classic outer step
    for a, b, o in table.packed():
        new = _nesterov_torch(sync[a:b], delta_packed[o:o + b - a], mom[a:b], inv_world, lr, momentum, first,
                              fused_step=master.is_cuda)
        if alpha == 0.0:
            master[a:b].copy_(new)
        else:
            master[a:b].sub_(new).mul_(alpha).add_(new)  # theta + alpha * (local - theta)
        sync[a:b].copy_(new)
        if sh is not None:
            sh[a:b].copy_(master[a:b])
