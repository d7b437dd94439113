"""Fused lm_head + cross-entropy with the backward computed during the forward (K9).

The reference materialises fp32 logits ``[N, V]`` and their gradient (1.05 GB each per 8k-token
micro-batch; 33.5 GB at 262k tokens).  Here the N rows are processed in
chunks; for each chunk:

  1. ``logits = y_c @ W^T``            (the plain projection GEMM, ops.linear.mm_nt: the selected
                                       --proj-gemm kernel; compute dtype)
  2. ``nd_ce_fwd_bwd``                 one HIP kernel, one row per workgroup: online max/sum-exp over V,
                                       per-row loss summed into a device scalar, and the logits
                                       buffer overwritten IN PLACE by ``dlogits = (softmax - onehot) * s``
  3. ``dy_c = dlogits @ W``            (dgrad, kept for backward)
  4. ``gW += dlogits^T @ y_c``         (wgrad, fp32 accumulate into the flat grad buffer)

so only one chunk of logits ever exists and nothing [N, V]-sized survives the forward.
``s = loss_scale / n_valid`` is read from device memory (no host sync).

z-loss (``z_loss`` = z_coef > 0, --z-loss; docs/DESIGN.md "z-loss"): the objective gains
``z_coef * mean(lse^2)`` over the valid rows, lse = logsumexp(logits).  Nothing [N, V]-sized exists for an
autograd-side term to attach to, so the term lives in the CE kernels: ``nd_ce_z_fwd_bwd`` /
``nd_ce_z_fwd_bwd_q8`` are step 2 with ``dlogits = s * (softmax * (1 + 2 z_coef lse) - onehot)`` -- one more
scalar per row -- and accumulate ``sum lse^2`` apart from the cross-entropy sum.  The returned loss is then
the objective, cross-entropy + weighted z term; ``lm_head_ce_parts`` also gives the two parts as detached
device scalars (no host sync).  With ``z_loss == 0.0`` the entry points called, the launches and every bit are
those of the z-free path.

Logit soft-capping (``softcap`` = C > 0, --logit-softcap; docs/DESIGN.md "Logit soft-capping"): the model's logits are
``C * tanh(logits / C)``.  For the same reason the cap lives in the CE kernels: ``nd_ce_cap_fwd_bwd`` /
``nd_ce_cap_fwd_bwd_q8`` are step 2 on the capped logits, formed in fp32 from the stored ones, with
``dlogits = s * (softmax * g - onehot) * (1 - tanh^2)`` (g = 1 without z-loss), and ``nd_ce_loss_cap`` is the loss-only
kernel on them.  With ``softcap == 0.0`` the entry points called, the launches and every bit are those of the cap-free
path.  ``logit_softcap`` caps a logits tensor the model hands out, in place.

fp8 (``f8`` = the model's ``Fp8Linears``, BASELINE config 5): the three GEMMs run on the own fp8 kernels --
logits = e4m3 y8 . W8^T, the CE kernel writes the dlogits straight as e5m2 (delayed scaling, slot "x.lm";
``nd_ce_fwd_bwd_q8``, bitwise the bf16 dlogits + separate cast that the first step, which has no scale yet,
still takes; with z-loss the same pair is ``nd_ce_z_fwd_bwd_q8`` / ``nd_ce_z_fwd_bwd``), dy = dlogits8 . (W^T)8^T and
gW += dlogits8^T y8 (wgrad8_pp_kernel).  The returned loss is the unscaled mean over valid tokens
(ignore_index=-100), matching ``HF/loss/loss_utils.py:32-71``.

Contract: the weight gradient is produced in the forward, assuming the loss is back-propagated
with unit upstream gradient (``loss.backward()``); ``loss_scale`` is how callers scale it
(e.g. 1/grad_accum).  It scales the gradient of the whole objective -- with z-loss
``loss_scale * (sum CE + z_coef * sum lse^2) / n_valid`` -- and never the returned loss or its parts.
The activation gradient is additionally multiplied by the upstream gradient, so ``dy`` is correct for
any upstream value.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import torch

from . import _ext
from .determinism import deterministic
from .linear import mm_nt, wgrad_accumulate

IGNORE_INDEX = -100
_HIP_INVALID_VALUE = 1  # hipErrorInvalidValue: a launcher refused the shape (caller takes the general path)


# logits chunk budget (ND_CE_CHUNK_MB, default 4 GiB: a whole 64k-token micro-batch of a 32k
# vocabulary in bf16 -- one GEMM triple per micro-batch; +0.35 % over 1 GiB chunks, profiles/r2_ce_chunk_ab.md)
_CHUNK_BYTES = int(float(os.environ.get("ND_CE_CHUNK_MB", "4096")) * (1 << 20))


def _chunk_rows(V: int, elem: int, budget_bytes: int = 0) -> int:
    return max(256, ((budget_bytes or _CHUNK_BYTES) // (V * elem)) // 256 * 256)


def _chunks(n: int, V: int, elem: int, chunk_rows: int):
    """The [start, end) row chunks of the lm head: ``chunk_rows`` as given, else the logits budget."""
    chunk = chunk_rows or _chunk_rows(V, elem)
    if not chunk_rows and n > chunk:  # equal-sized chunks: one GEMM shape, one tuned kernel
        nch = -(-n // chunk)
        chunk = (-(-n // nch) + 255) // 256 * 256
    return [(s, min(n, s + chunk)) for s in range(0, n, chunk)]


class LMHeadLoss(NamedTuple):
    """``loss``: the objective (differentiable); ``ce_loss``: its cross-entropy part; ``z_loss``: the weighted z
    term ``z_coef * mean(lse^2)`` -- both detached device scalars, ``z_loss`` None when z-loss is off (then
    ``ce_loss`` is ``loss``, detached)."""
    loss: torch.Tensor
    ce_loss: torch.Tensor
    z_loss: Optional[torch.Tensor]


class LMHeadCEFn(torch.autograd.Function):
    """Returns the loss; with ``z_loss`` > 0 the triple (objective, cross-entropy, weighted z term), the last two
    not differentiable."""

    @staticmethod
    def forward(ctx, y, w, gw, targets, loss_scale, chunk_rows, wt, f8=None, version=0, y8=None, z_loss=0.0,
                softcap=0.0):
        n, d = y.shape
        V = w.shape[0]
        targets = targets.reshape(-1)
        valid = (targets != IGNORE_INDEX).sum().to(torch.float32)
        denom = valid.clamp_min(1.0)
        scale = (loss_scale / denom).reshape(1).contiguous()
        dy = torch.empty_like(y)
        loss_sum = torch.zeros(1, dtype=torch.float32, device=y.device)
        z_sum = torch.zeros(1, dtype=torch.float32, device=y.device) if z_loss else None  # sum lse^2, valid rows
        hip = _ext.use_hip(y)
        det = deterministic()
        q = r = None
        if f8 is not None and hip:
            from .fp8 import E5M2, issue_wgrad_f8
            from .gemm import gemm_pp_f8, pp_f8_supported
            kx, kdy, y8, wq = f8.operands(LM_KEY, y, w, version, y8)
            q = r = f8.recipe if pp_f8_supported(y8, wq.w8) and V % 128 == 0 else None
        for s, e in _chunks(n, V, y.element_size() if hip else 4, chunk_rows):
            yc, tc = y[s:e], targets[s:e]
            if hip:
                if q is not None:  # fp8: e4m3 x e4m3 on the own fp8 ping-pong kernel
                    logits = gemm_pp_f8(y8[s:e], wq.w8, r.inv[kx:kx + 1], wq.inv)
                else:  # the selected plain projection GEMM (ops/linear.py proj_gemm: hipBLASLt by default)
                    logits = mm_nt(yc, w)
                rows = torch.empty(e - s, dtype=torch.float32, device=y.device) if det else None
                dl8 = None
                t8 = r.target(kdy, E5M2) if q is not None else None
                if softcap:
                    dl8 = _ce_cap_launch(logits, tc, loss_sum, z_sum, scale, rows, z_loss, softcap, t8)
                elif z_loss:
                    dl8 = _ce_z_launch(logits, tc, loss_sum, z_sum, scale, rows, z_loss, t8)
                elif t8 is not None:
                    # fp8: the CE kernel writes the e5m2 dlogits itself (no bf16 dlogits, no separate cast)
                    q8 = t8.alloc((e - s, V), y.device)
                    rc = _ext.lib().nd_ce_fwd_bwd_q8(_ext.ptr(logits), _ext.dtcode(logits), _ext.ptr(tc),
                                                     _ext.ptr(loss_sum), _ext.ptr(scale), e - s, V, IGNORE_INDEX, 0,
                                                     _ext.ptr(rows) if det else 0, *t8.args(q8),
                                                     _ext.stream_ptr(y.device))
                    if rc == 0:
                        dl8 = q8
                    elif rc != _HIP_INVALID_VALUE:  # invalid value = shape not taken: cast separately below
                        _ext.check(rc, "nd_ce_fwd_bwd_q8")
                if dl8 is None and not z_loss and not softcap:
                    _ext.check(_ext.lib().nd_ce_fwd_bwd(_ext.ptr(logits), _ext.dtcode(logits), _ext.ptr(tc),
                                                        _ext.ptr(loss_sum), _ext.ptr(scale), e - s, V, IGNORE_INDEX,
                                                        0, _ext.ptr(rows) if det else 0, 0.0,
                                                        _ext.stream_ptr(y.device)), "nd_ce_fwd_bwd")
                if det:  # per-row losses, one ordered reduction (no float atomics)
                    loss_sum += rows.sum()
                dl = logits if dl8 is None else None
            else:
                dl8 = None
                logits = torch.mm(yc.float(), w.float().t())
                if softcap:
                    th = torch.tanh(logits / softcap)
                    logits = softcap * th
                lse = torch.logsumexp(logits, dim=-1)
                ok = tc != IGNORE_INDEX
                tgt = torch.where(ok, tc, torch.zeros_like(tc))
                picked = logits.gather(1, tgt[:, None])[:, 0]
                loss_sum += torch.where(ok, lse - picked, torch.zeros_like(lse)).sum()
                p = torch.softmax(logits, dim=-1)
                if z_loss:
                    z_sum += torch.where(ok, lse * lse, torch.zeros_like(lse)).sum()
                    p *= (1.0 + 2.0 * z_loss * lse)[:, None]
                p.scatter_add_(1, tgt[:, None], -torch.ones_like(p[:, :1]))
                p *= ok[:, None].to(p.dtype) * scale
                if softcap:
                    p *= 1.0 - th * th
                dl = p.to(y.dtype)
            if q is not None:
                # e5m2 dlogits (one cast; delayed scaling of slot kdy), then both gradient GEMMs in fp8
                if dl8 is None:
                    dl8 = r.quantize(dl, kdy, E5M2)
                gemm_pp_f8(dl8, wq.wT8, r.inv[kdy:kdy + 1], wq.inv, out=dy[s:e])
                issue_wgrad_f8(gw, dl8, y8[s:e], r.inv[kdy:kdy + 1], r.inv[kx:kx + 1], dl)
                continue
            # dy rows written in place (a row slice of a contiguous tensor); with wt = W^T the GEMM
            # has the faster K-contiguous operand layout (ops/linear.py)
            if wt is not None and dl.dtype == wt.dtype:
                mm_nt(dl, wt, out=dy[s:e])
            elif dl.dtype == w.dtype:
                torch.mm(dl, w, out=dy[s:e])
            else:
                dy[s:e] = torch.mm(dl, w.to(dl.dtype))
            if gw is not None:
                # stays on the compute stream: the chunk loop is GEMM-bound (library GEMMs fence
                # side-stream work anyway, ops/linear.py)
                wgrad_accumulate(gw, dl, yc.to(dl.dtype))
        ctx.save_for_backward(dy)
        if not z_loss:
            return (loss_sum / denom).reshape(())
        ce = (loss_sum / denom).reshape(())
        z = (z_sum * z_loss / denom).reshape(())
        ctx.mark_non_differentiable(ce, z)
        return ce + z, ce, z

    @staticmethod
    def backward(ctx, g, *_):
        (dy,) = ctx.saved_tensors
        return (dy * g.to(dy.dtype),) + (None,) * 11


def _ce_z_launch(logits, tc, loss_sum, z_sum, scale, rows, z_coef, t8):
    """The z-loss CE kernel on one chunk of logits; ``rows`` (deterministic mode): per-row cross-entropy, with the
    per-row lse^2 in a buffer of its own, both summed in order here (no float atomics).  ``t8``: the fp8 target of the
    dlogits, if any; returns the fp8 dlogits when the q8 entry took the shape, else None (bf16 dlogits in place)."""
    n, V = logits.shape
    rows_z = torch.empty_like(rows) if rows is not None else None
    head = (_ext.ptr(logits), _ext.dtcode(logits), _ext.ptr(tc), _ext.ptr(loss_sum), _ext.ptr(z_sum), _ext.ptr(scale),
            n, V, IGNORE_INDEX, 0, _ext.ptr(rows), _ext.ptr(rows_z), z_coef)
    dl8 = None
    if t8 is not None:
        q8 = t8.alloc((n, V), logits.device)
        rc = _ext.lib().nd_ce_z_fwd_bwd_q8(*head, *t8.args(q8), _ext.stream_ptr(logits.device))
        if rc == 0:
            dl8 = q8
        elif rc != _HIP_INVALID_VALUE:  # invalid value = shape not taken: cast separately, as the z-free path
            _ext.check(rc, "nd_ce_z_fwd_bwd_q8")
    if dl8 is None:
        _ext.check(_ext.lib().nd_ce_z_fwd_bwd(*head, _ext.stream_ptr(logits.device)), "nd_ce_z_fwd_bwd")
    if rows is not None:
        z_sum += rows_z.sum()
    return dl8


def _ce_cap_launch(logits, tc, loss_sum, z_sum, scale, rows, z_coef, cap, t8):
    """The capped CE kernel on one chunk of logits, with z-loss (``z_sum`` given) or without; otherwise as
    ``_ce_z_launch``."""
    n, V = logits.shape
    rows_z = torch.empty_like(rows) if rows is not None and z_sum is not None else None
    head = (_ext.ptr(logits), _ext.dtcode(logits), _ext.ptr(tc), _ext.ptr(loss_sum), _ext.ptr(z_sum), _ext.ptr(scale),
            n, V, IGNORE_INDEX, 0, _ext.ptr(rows), _ext.ptr(rows_z), z_coef if z_sum is not None else 0.0, cap)
    dl8 = None
    if t8 is not None:
        q8 = t8.alloc((n, V), logits.device)
        rc = _ext.lib().nd_ce_cap_fwd_bwd_q8(*head, *t8.args(q8), _ext.stream_ptr(logits.device))
        if rc == 0:
            dl8 = q8
        elif rc != _HIP_INVALID_VALUE:  # invalid value = shape not taken: cast separately, as the cap-free path
            _ext.check(rc, "nd_ce_cap_fwd_bwd_q8")
    if dl8 is None:
        _ext.check(_ext.lib().nd_ce_cap_fwd_bwd(*head, _ext.stream_ptr(logits.device)), "nd_ce_cap_fwd_bwd")
    if rows_z is not None:
        z_sum += rows_z.sum()
    return dl8


LM_KEY = "x.lm"  # the lm head's slot pair / weight cache in Fp8Linears (ops/fp8.py fp8_projection("lm"))


def _z_coef(z_loss) -> float:
    z = float(z_loss)
    if not 0.0 <= z < float("inf"):  # refuses NaN too
        raise ValueError(f"z_loss must be a finite coefficient >= 0 (0 = off), got {z_loss!r}")
    return z


def _cap(softcap) -> float:
    if softcap is None:
        return 0.0
    if isinstance(softcap, (bool, str)):
        raise ValueError(f"softcap must be a finite number > 0 (0 = off), got {softcap!r}")
    c = float(softcap)
    if not 0.0 <= c < float("inf"):  # refuses NaN too
        raise ValueError(f"softcap must be a finite number > 0 (0 = off), got {softcap!r}")
    return c


def logit_softcap(logits: torch.Tensor, softcap: float) -> torch.Tensor:
    """``softcap * tanh(logits / softcap)`` IN PLACE on a contiguous bf16 / fp32 tensor (``nd_logit_softcap`` on the
    HIP path), returned; ``softcap`` 0 = off: nothing runs.  bf16 results are the fp32 value rounded once."""
    c = _cap(softcap)
    if c == 0.0 or logits.numel() == 0:
        return logits
    if not logits.is_contiguous():
        raise ValueError("logit_softcap works in place on a contiguous tensor")
    if _ext.use_hip(logits):
        _ext.check(_ext.lib().nd_logit_softcap(_ext.ptr(logits), _ext.dtcode(logits), logits.numel(), c,
                                               _ext.stream_ptr(logits.device)), "nd_logit_softcap")
    else:
        from .reference import softcap as _ref
        logits.copy_(_ref(logits, c))
    return logits


def lm_head_ce(y: torch.Tensor, w: torch.Tensor, gw: torch.Tensor, targets: torch.Tensor, loss_scale: float = 1.0,
               chunk_rows: int = 0, wt: torch.Tensor = None, f8=None, version: int = 0, y8=None,
               z_loss: float = 0.0, softcap: float = 0.0) -> torch.Tensor:
    """``wt``: optional W^T copy [d, V] for the input-gradient GEMM (see ops/linear.py).  ``f8``: the model's
    ``Fp8Linears`` for the fp8 lm head, with the weight ``version`` and ``y8``, the fused e4m3 copy of y if any.
    ``z_loss``: the z-loss coefficient (0.0 = off); the returned loss is the objective, cross-entropy + z term.
    ``softcap``: the logits' soft cap C (0.0 = off): loss and gradients are those of ``C * tanh(logits / C)``."""
    return lm_head_ce_parts(y, w, gw, targets, loss_scale, chunk_rows, wt, f8, version, y8, z_loss, softcap).loss


def lm_head_ce_parts(y: torch.Tensor, w: torch.Tensor, gw: torch.Tensor, targets: torch.Tensor,
                     loss_scale: float = 1.0, chunk_rows: int = 0, wt: torch.Tensor = None, f8=None, version: int = 0,
                     y8=None, z_loss: float = 0.0, softcap: float = 0.0) -> LMHeadLoss:
    """``lm_head_ce`` with the objective's two parts beside it (``LMHeadLoss``)."""
    z = _z_coef(z_loss)
    c = _cap(softcap)
    if c != 0.0:
        out = LMHeadCEFn.apply(y, w, gw, targets, float(loss_scale), int(chunk_rows), wt, f8, int(version), y8, z, c)
        return LMHeadLoss(*out) if z != 0.0 else LMHeadLoss(out, out.detach(), None)
    if z == 0.0:  # today's call, argument for argument
        loss = LMHeadCEFn.apply(y, w, gw, targets, float(loss_scale), int(chunk_rows), wt, f8, int(version), y8)
        return LMHeadLoss(loss, loss.detach(), None)
    return LMHeadLoss(*LMHeadCEFn.apply(y, w, gw, targets, float(loss_scale), int(chunk_rows), wt, f8, int(version),
                                        y8, z))


@torch.no_grad()
def lm_head_loss(y: torch.Tensor, w: torch.Tensor, targets: torch.Tensor, chunk_rows: int = 0, softcap: float = 0.0):
    """Loss-only lm head for evaluation: ``(row_loss [n] fp32, row_hit [n] bool)``.

    Per chunk ``logits = y_c @ W^T`` (the plain projection GEMM) and ``nd_ce_loss``: one of ``lm_head_ce``'s three
    GEMMs, no gradient written over the logits, no ``dy``.  ``row_loss`` = logsumexp - logit[target] (0 where the
    target is ``IGNORE_INDEX``); ``row_hit`` = the target's logit equals the row maximum (top-1, ties count, exact on
    the stored logits; False on ignored rows and on rows that hold a NaN).  Per-row stores only -- no atomics -- so
    the result is bitwise repeatable with or without the deterministic mode.  Always bf16 / fp32, never the fp8
    lm head.  CPU / ``--ops torch``: fp32 logits, as ``lm_head_ce``.  ``softcap`` (C > 0; 0.0 = off, today's launch):
    ``row_loss`` on ``C * tanh(logits / C)`` (``nd_ce_loss_cap``); ``row_hit`` stays the top-1 of the stored logits."""
    cap = _cap(softcap)
    n, V = y.shape[0], w.shape[0]
    targets = targets.reshape(-1)
    row_loss = torch.empty(n, dtype=torch.float32, device=y.device)
    row_hit = torch.empty(n, dtype=torch.bool, device=y.device)
    hip = _ext.use_hip(y)
    for s, e in _chunks(n, V, y.element_size() if hip else 4, int(chunk_rows)):
        yc, tc = y[s:e], targets[s:e]
        if hip:
            logits = mm_nt(yc, w)
            if cap:
                _ext.check(_ext.lib().nd_ce_loss_cap(_ext.ptr(logits), _ext.dtcode(logits), _ext.ptr(tc), e - s, V,
                                                     IGNORE_INDEX, _ext.ptr(row_loss[s:e]), 0, _ext.ptr(row_hit[s:e]),
                                                     cap, _ext.stream_ptr(y.device)), "nd_ce_loss_cap")
                continue
            _ext.check(_ext.lib().nd_ce_loss(_ext.ptr(logits), _ext.dtcode(logits), _ext.ptr(tc), e - s, V,
                                             IGNORE_INDEX, _ext.ptr(row_loss[s:e]), 0, _ext.ptr(row_hit[s:e]),
                                             _ext.stream_ptr(y.device)), "nd_ce_loss")
        else:
            logits = torch.mm(yc.float(), w.float().t())
            ok = tc != IGNORE_INDEX
            tgt = torch.where(ok, tc, torch.zeros_like(tc))
            hit = logits.gather(1, tgt[:, None])[:, 0] == logits.max(dim=-1).values  # on the stored logits
            if cap:
                logits = cap * torch.tanh(logits / cap)
            lse = torch.logsumexp(logits, dim=-1)
            picked = logits.gather(1, tgt[:, None])[:, 0]
            row_loss[s:e] = torch.where(ok, lse - picked, torch.zeros_like(lse))
            row_hit[s:e] = ok & hit & ~torch.isnan(lse)
    return row_loss, row_hit
