"""Muon inner optimizer (MuLoCo): Newton-Schulz products and the flat-buffer step.

Per Muon matrix W [m, n] with gradient G (``coef`` = the global clip coefficient of ``adamw_step``)::

    M  = mu * M + coef * G                      (fp32, M lives in exp_avg over the matrix's span)
    U  = coef * G + mu * M                      (Nesterov)
    X  = U / (||U||_F + 1e-7);  if m > n work on X^T
    repeat ns_steps times, (a, b, c) = NS_COEF:
        A = X X^T                               ``ns_gram``
        B = b * A + c * (A A^T)                 ``ns_poly``
        X = a * X + B X                         ``ns_update``
    W  = W * (1 - lr * wd) - lr * 0.2 * sqrt(max(m, n)) * X      (shadow = bf16(W))

Everything else (embedding, lm head, norms) takes ``adamw_step``'s update through a span table
(``adamw_step_spans``, HIP: csrc/muon.hip).  On a GPU X after normalisation, A, B and every new X are stored as
bf16, every product accumulates in fp32 and the ``b * A + ...`` / ``a * X + ...`` terms are applied to the fp32
result before the one rounding; on the CPU nothing is rounded to bf16.

The Newton-Schulz products and ``muon_step`` are PyTorch code: they run on the CPU and, on a GPU, only under the
PyTorch backend (``set_backend("torch")`` / ``--ops torch``).  There is no HIP kernel for them yet, and a GPU tensor
under the HIP backend raises instead of quietly running eager PyTorch (docs/DESIGN.md "Muon inner optimizer").
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _ext
from .optim import SUMSQ_BLOCKS, _adamw_update_torch

NS_COEF = (3.4445, -4.7750, 2.0315)
NORM_EPS = 1e-7
MUON_SUFFIXES = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
                 "self_attn.o_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")


def _torch_only(t: torch.Tensor, what: str) -> None:
    """The policy of ops/_ext.py: a GPU tensor takes a HIP kernel unless the PyTorch backend was asked for."""
    if _ext.use_hip(t):
        raise NotImplementedError(f"{what} has no HIP kernel: on a GPU it runs under the PyTorch backend only "
                                  f"(set_backend('torch') / --ops torch)")


def _wide(t):
    return t.float() if t.dtype in (torch.bfloat16, torch.float16) else t


def ns_gram(X: torch.Tensor) -> torch.Tensor:
    """``A[i] = X[i] X[i]^T`` for X ``[batch, m, n]`` (fp32 accumulation for bf16, stored in X's dtype)."""
    _torch_only(X, "ns_gram")
    x = _wide(X)
    return torch.bmm(x, x.transpose(1, 2)).to(X.dtype)


def ns_poly(A: torch.Tensor, b: float, c: float) -> torch.Tensor:
    """``B[i] = b * A[i] + c * A[i] A[i]^T`` for A ``[batch, m, m]`` (one rounding of the fp32 result)."""
    _torch_only(A, "ns_poly")
    a = _wide(A)
    return (b * a + c * torch.bmm(a, a.transpose(1, 2))).to(A.dtype)


def ns_update(B: torch.Tensor, X: torch.Tensor, a: float) -> torch.Tensor:
    """``X'[i] = a * X[i] + B[i] X[i]`` for B ``[batch, m, m]``, X ``[batch, m, n]``."""
    _torch_only(X, "ns_update")
    bb, x = _wide(B), _wide(X)
    return (a * x + torch.bmm(bb, x)).to(X.dtype)


def ns_iterate(X: torch.Tensor, steps: int = 5) -> torch.Tensor:
    """``steps`` Newton-Schulz iterations on an already normalised X ``[batch, r, c]`` with r <= c."""
    a, b, c = NS_COEF
    for _ in range(steps):
        A = ns_gram(X)
        X = ns_update(ns_poly(A, b, c), X, a)
    return X


def newton_schulz(X: torch.Tensor, steps: int = 5) -> torch.Tensor:
    """Muon's orthogonalisation of every matrix of X (``[m, n]`` or ``[batch, m, n]``): Frobenius normalisation,
    transpose when m > n, ``steps`` iterations, transpose back.  On a GPU the normalised X and every intermediate
    are bf16 (the result too); on the CPU the computation stays in X's precision (fp32 for bf16 input)."""
    single = X.dim() == 2
    if single:
        X = X.unsqueeze(0)
    if X.dim() != 3:
        raise ValueError(f"newton_schulz takes [m, n] or [batch, m, n], got {tuple(X.shape)}")
    _torch_only(X, "newton_schulz")
    m, n = X.shape[1], X.shape[2]
    x = _wide(X)
    norm = x.flatten(1).norm(dim=1).view(-1, 1, 1)
    Y = x / (norm + NORM_EPS)
    if m > n:
        Y = Y.transpose(1, 2)
    if X.is_cuda:
        Y = Y.to(torch.bfloat16)
    Y = ns_iterate(Y.contiguous(), steps)
    if m > n:
        Y = Y.transpose(1, 2)
    return Y[0] if single else Y


# ---------------------------------------------------------------------------------------------------------
class AdamWSpans:
    """Span list for ``adamw_step_spans`` plus its device table.  ``spans``: ``[(start, end), ...]`` in elements of
    the flat vector, increasing and disjoint; every start a multiple of 4 (16-byte vectors), any length.  Device
    table (int64): S rows ``(start, end)``, then S + 1 prefix sums of the lengths in 4-element vectors rounded up."""

    def __init__(self, spans: Sequence[Tuple[int, int]]):
        self.spans = [(int(a), int(b)) for a, b in spans]
        if not self.spans:
            raise ValueError("span table is empty")
        prev = 0
        self.pre = [0]
        for a, b in self.spans:
            if a % 4:
                raise ValueError(f"span [{a}, {b}) is misaligned: starts must be multiples of 4")
            if a < 0 or b <= a:
                raise ValueError(f"span [{a}, {b}) is empty or negative")
            if a < prev:
                raise ValueError(f"span [{a}, {b}) overlaps or precedes the span ending at {prev}")
            prev = b
            self.pre.append(self.pre[-1] + (b - a + 3) // 4)
        self.total4 = self.pre[-1]
        self.end = prev
        self._dev: Dict[torch.device, torch.Tensor] = {}

    def __len__(self):
        return len(self.spans)

    def device_table(self, device: torch.device) -> torch.Tensor:
        t = self._dev.get(device)
        if t is None:
            t = torch.tensor([x for ab in self.spans for x in ab] + self.pre, dtype=torch.int64, device=device)
            self._dev[device] = t
        return t


class MuonPlan:
    """Which spans of a flat parameter vector Muon owns, grouped by matrix shape (``groups``: (m, n) -> flat
    offsets), and the complementary AdamW span table (``adamw``).  Built once from ``names`` / ``shapes`` /
    ``offsets`` (a ``ParamStore``'s)."""

    def __init__(self, names: Sequence[str], shapes: Dict[str, Tuple[int, ...]], offsets: Dict[str, int]):
        self.groups: Dict[Tuple[int, int], List[int]] = {}
        self.muon_names: List[str] = []
        rest = []
        for name in names:
            shape, off = tuple(shapes[name]), int(offsets[name])
            if ".layers." in name and name.endswith(MUON_SUFFIXES) and len(shape) == 2:
                self.groups.setdefault((shape[0], shape[1]), []).append(off)
                self.muon_names.append(name)
            else:
                numel = 1
                for s in shape:
                    numel *= int(s)
                rest.append((off, off + numel))
        self.adamw = AdamWSpans(sorted(rest)) if rest else None

    @classmethod
    def from_store(cls, store) -> "MuonPlan":
        return cls(store.names, store.shapes, store.offsets)


def _clip_torch(grad, max_norm, norm_out, skip_nonfinite, skipped):
    """``adamw_step``'s PyTorch clip: ``(skip, coef)``, coef a 0-d tensor or None."""
    if max_norm is None and norm_out is None and not skip_nonfinite:
        return False, None
    total = grad.norm()
    if norm_out is not None:
        norm_out.copy_(total.reshape(norm_out.shape))
    if skip_nonfinite and not bool(torch.isfinite(total)):
        if skipped is not None:
            skipped += 1
        return True, None
    return False, (torch.clamp(max_norm / (total + 1e-6), max=1.0) if max_norm is not None else None)


def _adamw_spans_torch(master, grad, exp_avg, exp_avg_sq, sh, spans: AdamWSpans, coef, step, lr, betas, eps,
                       weight_decay) -> None:
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    for a, b in spans.spans:
        g = grad[a:b] if coef is None else grad[a:b] * coef
        _adamw_update_torch(master[a:b], g, exp_avg[a:b], exp_avg_sq[a:b], lr, b1, b2, eps, weight_decay, bc1, bc2)
        if sh is not None:
            sh[a:b].copy_(master[a:b])


def adamw_step_spans(master: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                     shadow: Optional[torch.Tensor], spans, step: int, lr: float, betas=(0.9, 0.999),
                     eps: float = 1e-8, weight_decay: float = 0.01, max_norm: Optional[float] = 1.0,
                     norm_out: Optional[torch.Tensor] = None, skip_nonfinite: bool = False,
                     skipped: Optional[torch.Tensor] = None) -> None:
    """``adamw_step`` on the elements of ``spans`` only (an :class:`AdamWSpans` or a span list), one launch: the
    global norm and clip coefficient still come from the WHOLE gradient, and inside the spans the result is bit for
    bit ``adamw_step``'s.  Elements outside the spans are never written."""
    table = spans if isinstance(spans, AdamWSpans) else AdamWSpans(spans)
    if table.end > min(master.numel(), grad.numel(), exp_avg.numel(), exp_avg_sq.numel()):
        raise ValueError(f"span table ends at {table.end}, past the flat buffers")
    sh = shadow if (shadow is not None and shadow.data_ptr() != master.data_ptr()) else None
    b1, b2 = betas
    if _ext.use_hip(master):
        L, s = _ext.lib(), _ext.stream_ptr(master.device)
        part = None
        if max_norm is not None or norm_out is not None or skip_nonfinite:
            part = torch.empty(SUMSQ_BLOCKS, dtype=torch.float32, device=master.device)
            _ext.check(L.nd_sumsq_partial(_ext.ptr(grad), grad.numel(), _ext.ptr(part), SUMSQ_BLOCKS, s),
                       "nd_sumsq_partial")
        _ext.check(L.nd_adamw_step_spans(
            _ext.ptr(master), _ext.ptr(grad), _ext.ptr(exp_avg), _ext.ptr(exp_avg_sq), _ext.ptr(sh),
            _ext.dtcode(sh) if sh is not None else 0, _ext.ptr(table.device_table(master.device)), len(table),
            table.total4, _ext.ptr(part), SUMSQ_BLOCKS, float(lr), float(b1), float(b2), float(eps),
            float(weight_decay), float(1.0 - b1 ** step), float(1.0 - b2 ** step),
            float(max_norm if max_norm is not None else -1.0), _ext.ptr(norm_out), 1 if skip_nonfinite else 0,
            _ext.ptr(skipped), s), "nd_adamw_step_spans")
        return
    skip, coef = _clip_torch(grad, max_norm, norm_out, skip_nonfinite, skipped)
    if not skip:
        _adamw_spans_torch(master, grad, exp_avg, exp_avg_sq, sh, table, coef, step, lr, betas, eps, weight_decay)


def muon_step(master: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
              shadow: Optional[torch.Tensor], plan: MuonPlan, step: int, lr: float, momentum: float = 0.95,
              ns_steps: int = 5, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01,
              max_norm: Optional[float] = 1.0, norm_out: Optional[torch.Tensor] = None,
              skip_nonfinite: bool = False, skipped: Optional[torch.Tensor] = None) -> None:
    """One clip + Muon / AdamW step over flat fp32 buffers (module docstring).  The Muon momentum is ``exp_avg``
    over the Muon spans (``exp_avg_sq`` is not touched there); ``step`` is the 1-based AdamW step count.  A
    non-finite global norm with ``skip_nonfinite`` skips the whole step and counts it once."""
    _torch_only(master, "muon_step")
    sh = shadow if (shadow is not None and shadow.data_ptr() != master.data_ptr()) else None
    skip_step, coef = _clip_torch(grad, max_norm, norm_out, skip_nonfinite, skipped)
    if skip_step:
        return
    for (m, n), offs in plan.groups.items():
        us = []
        for o in offs:
            G = grad[o:o + m * n].view(m, n)
            M = exp_avg[o:o + m * n].view(m, n)
            Gc = G if coef is None else G * coef
            M.mul_(momentum).add_(Gc)
            us.append(Gc + momentum * M)
        X = newton_schulz(torch.stack(us), ns_steps)
        for i, o in enumerate(offs):
            W = master[o:o + m * n].view(m, n)
            W.mul_(1.0 - lr * weight_decay).add_(X[i].to(W.dtype), alpha=-lr * 0.2 * math.sqrt(max(m, n)))
            if sh is not None:
                sh[o:o + m * n].copy_(master[o:o + m * n])
    if plan.adamw is not None:
        _adamw_spans_torch(master, grad, exp_avg, exp_avg_sq, sh, plan.adamw, coef, step, lr, betas, eps, weight_decay)
