"""QK-norm: an RMSNorm over ``head_dim`` of every query and key head, before RoPE (Qwen3 / OLMo-2 / Gemma-3), with
one learnable fp32 ``[hd]`` weight each for q and k.  docs/DESIGN.md, "QK-norm".

Both ops work on the packed q|k|v projection output ``[N, (nh + 2 nkv) * hd]`` and never touch its v columns:
``x_hat = x * rstd``, ``rstd = rsqrt(mean_d x^2 + eps)`` over the ``hd`` elements of one (token, head), fp32
statistics, ``y = w * x_hat`` rounded once to the compute dtype.

``qk_norm``       the norm alone, in place, no autograd, static shapes and no host sync: the decode step's form
                  (``nd_qk_norm``), and the first half of the composition the fused forward equals bit for bit.
``qk_norm_rope``  the training / prefill form, an autograd Function.  HIP path: ``nd_qk_norm_rope_fwd`` norms AND
                  rotates q|k in one pass (bitwise ``nd_rope_inplace`` of ``qk_norm``'s output), so the caller runs
                  ``attention(..., rotated=True)``, whose backward returns the gradient with respect to the normed,
                  un-rotated q|k; ``nd_qk_norm_bwd`` turns that into the gradient of the raw projection and adds the
                  weight gradients into the fp32 grad views (beta = 1, fixed order: bitwise repeatable).  Saved for
                  the backward: the raw q|k, compactly, and ``rstd`` [N, nh + nkv].  PyTorch path (CPU, ``--ops
                  torch``): the norm only, out of place; the attention rotates as it always does.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _ext
from . import reference as ref

HEAD_DIMS = (32, 64, 128)
MAX_PARTS = 1024  # partial rows (= workgroups) of the backward, csrc/qk_norm.hip


def _check(qkv, wq, wk, nh, nkv, hd):
    W = (nh + 2 * nkv) * hd
    if qkv.dim() != 2 or qkv.shape[1] != W:
        raise ValueError(f"qk_norm: qkv must be [N, (nh + 2 nkv) hd] = [N, {W}], not {tuple(qkv.shape)}")
    for name, w in (("wq", wq), ("wk", wk)):
        if tuple(w.shape) != (hd,) or w.dtype != torch.float32 or w.device != qkv.device:
            raise ValueError(f"qk_norm: {name} must be an fp32 [{hd}] tensor on the device of qkv")


def _check_hip(qkv, wq, wk, hd):
    if hd not in HEAD_DIMS:
        raise ValueError(f"qk_norm: head_dim {hd} not in {HEAD_DIMS} on the HIP path")
    if qkv.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"qk_norm: unsupported dtype {qkv.dtype}")
    if not qkv.is_contiguous() or qkv.data_ptr() % 16:
        raise ValueError("qk_norm: qkv must be contiguous and 16-byte aligned")
    for name, w in (("wq", wq), ("wk", wk)):
        if not w.is_contiguous() or w.data_ptr() % 16:
            raise ValueError(f"qk_norm: {name} must be contiguous and 16-byte aligned")


def bwd_parts(rows: int, nh: int, nkv: int, hd: int) -> int:
    """Workgroups (= dW partial rows) of ``nd_qk_norm_bwd``: a function of the shape alone, four passes of a
    workgroup's 4096 / hd heads each, at most ``MAX_PARTS``."""
    per_block = 4 * (4096 // hd)
    return max(1, min(MAX_PARTS, (rows * (nh + nkv) + per_block - 1) // per_block))


@torch.no_grad()
def qk_norm(qkv: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, nh: int, nkv: int, hd: int,
            eps: float) -> torch.Tensor:
    """``y = w * x_hat`` on the q and k heads of ``qkv``, IN PLACE; returns ``qkv``."""
    _check(qkv, wq, wk, nh, nkv, hd)
    if _ext.use_hip(qkv):
        _check_hip(qkv, wq, wk, hd)
        _ext.check(_ext.lib().nd_qk_norm(_ext.ptr(qkv), _ext.dtcode(qkv), _ext.ptr(wq), _ext.ptr(wk), qkv.shape[0],
                                         nh, nkv, hd, qkv.shape[1], float(eps), _ext.stream_ptr(qkv.device)),
                   "nd_qk_norm")
        return qkv
    qkv.copy_(ref.qk_norm(qkv, wq, wk, nh, nkv, hd, eps))
    return qkv


def qk_norm_rope_fwd_launch(qkv, wq, wk, cos, sin, T, nh, nkv, hd, eps, save: bool):
    """``nd_qk_norm_rope_fwd`` in place on ``qkv``; returns (rstd [N, nh + nkv], the raw q|k [N, (nh + nkv) hd] or
    None).  Everything the kernel relies on is checked here."""
    _check(qkv, wq, wk, nh, nkv, hd)
    _check_hip(qkv, wq, wk, hd)
    N = qkv.shape[0]
    if T < 1 or N % T:
        raise ValueError(f"qk_norm_rope: {N} rows are no multiple of T = {T}")
    for name, t in (("cos", cos), ("sin", sin)):
        if t.dtype != torch.float32 or t.device != qkv.device or not t.is_contiguous() or t.dim() != 2 \
                or t.shape[1] != hd or t.shape[0] < T or t.data_ptr() % 16:
            raise ValueError(f"qk_norm_rope: {name} must be a contiguous fp32 [>= {T}, {hd}] table on the device")
    rstd = torch.empty(N, nh + nkv, dtype=torch.float32, device=qkv.device)
    raw = torch.empty(N, (nh + nkv) * hd, dtype=qkv.dtype, device=qkv.device) if save else None
    _ext.check(_ext.lib().nd_qk_norm_rope_fwd(_ext.ptr(qkv), _ext.dtcode(qkv), _ext.ptr(wq), _ext.ptr(wk),
                                              _ext.ptr(cos), _ext.ptr(sin), _ext.ptr(rstd), _ext.ptr(raw), N, T, nh,
                                              nkv, hd, qkv.shape[1], float(eps), _ext.stream_ptr(qkv.device)),
               "nd_qk_norm_rope_fwd")
    return rstd, raw


def qk_norm_bwd_launch(dy, raw, rstd, wq, wk, gwq, gwk, nh, nkv, hd):
    """``nd_qk_norm_bwd`` IN PLACE on ``dy`` (the gradient with respect to the normed q|k, packed with the v
    gradient): its q|k columns become the gradient of the raw projection, ``gwq`` / ``gwk`` (fp32 [hd] views, or both
    None) are accumulated into.  Returns ``dy``."""
    _check(dy, wq, wk, nh, nkv, hd)
    _check_hip(dy, wq, wk, hd)
    N = dy.shape[0]
    if tuple(raw.shape) != (N, (nh + nkv) * hd) or raw.dtype != dy.dtype or not raw.is_contiguous() \
            or raw.data_ptr() % 16:
        raise ValueError("qk_norm backward: the saved q|k must be a contiguous [N, (nh + nkv) hd] tensor of dy's dtype")
    if tuple(rstd.shape) != (N, nh + nkv) or rstd.dtype != torch.float32 or not rstd.is_contiguous():
        raise ValueError("qk_norm backward: rstd must be a contiguous fp32 [N, nh + nkv] tensor")
    if (gwq is None) != (gwk is None):
        raise ValueError("qk_norm backward: gwq and gwk are given together")
    for name, g in (("gwq", gwq), ("gwk", gwk)):
        if g is not None and (tuple(g.shape) != (hd,) or g.dtype != torch.float32 or not g.is_contiguous()
                              or g.device != dy.device):
            raise ValueError(f"qk_norm backward: {name} must be a contiguous fp32 [{hd}] tensor on the device")
    parts = bwd_parts(N, nh, nkv, hd)
    part = torch.empty(parts, 2 * hd, dtype=torch.float32, device=dy.device)
    _ext.check(_ext.lib().nd_qk_norm_bwd(_ext.ptr(dy), _ext.dtcode(dy), _ext.ptr(raw), _ext.ptr(rstd), _ext.ptr(wq),
                                         _ext.ptr(wk), _ext.ptr(part), parts, _ext.ptr(gwq), _ext.ptr(gwk), N, nh,
                                         nkv, hd, dy.shape[1], _ext.stream_ptr(dy.device)), "nd_qk_norm_bwd")
    return dy


class QKNormRopeFn(torch.autograd.Function):
    """HIP path.  The packed buffer is this op's private input (the projection's backward saved its input, not its
    output; ``qk_norm_rope`` clones it otherwise): q|k are normed and rotated in place and the buffer is returned
    (``mark_dirty``).  The backward works in place on the incoming gradient under the same ownership rule:
    ``inplace`` says that the gradient buffer (the attention backward's fresh output) is private too."""

    @staticmethod
    def forward(ctx, qkv, wq, wk, gwq, gwk, cos, sin, T, nh, nkv, hd, eps, inplace):
        need = ctx.needs_input_grad[0]
        rstd, raw = qk_norm_rope_fwd_launch(qkv, wq, wk, cos, sin, T, nh, nkv, hd, eps, save=need)
        ctx.mark_dirty(qkv)
        if need:
            ctx.save_for_backward(raw, rstd, wq, wk)
        ctx.gw, ctx.dims, ctx.inplace = (gwq, gwk), (nh, nkv, hd), inplace
        return qkv

    @staticmethod
    def backward(ctx, dy):
        raw, rstd, wq, wk = ctx.saved_tensors
        nh, nkv, hd = ctx.dims
        dy = dy.contiguous() if ctx.inplace else dy.clone(memory_format=torch.contiguous_format)
        dx = qk_norm_bwd_launch(dy, raw, rstd, wq, wk, ctx.gw[0], ctx.gw[1], nh, nkv, hd)
        return (dx,) + (None,) * 12


class QKNormFn(torch.autograd.Function):
    """PyTorch path: the norm only (out of place), gradients by ``reference.qk_norm_backward``."""

    @staticmethod
    def forward(ctx, qkv, wq, wk, gwq, gwk, nh, nkv, hd, eps):
        ctx.save_for_backward(qkv, wq, wk)
        ctx.gw, ctx.dims = (gwq, gwk), (nh, nkv, hd, eps)
        return ref.qk_norm(qkv, wq, wk, nh, nkv, hd, eps)

    @staticmethod
    def backward(ctx, dy):
        qkv, wq, wk = ctx.saved_tensors
        nh, nkv, hd, eps = ctx.dims
        dx, dwq, dwk = ref.qk_norm_backward(dy, qkv, wq, wk, nh, nkv, hd, eps)
        if ctx.gw[0] is not None:
            ctx.gw[0].add_(dwq)
            ctx.gw[1].add_(dwk)
        return (dx,) + (None,) * 8


def qk_norm_rope(qkv: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, gwq: Optional[torch.Tensor],
                 gwk: Optional[torch.Tensor], cos: torch.Tensor, sin: torch.Tensor, T: int, nh: int, nkv: int, hd: int,
                 eps: float, inplace: bool = False) -> Tuple[torch.Tensor, bool]:
    """-> (packed buffer, rotated).  HIP path: q|k normed and rotated (position ``row % T``), ``rotated`` True: pass
    it on to ``attention(..., rotated=True)`` and ``cache_fill``.  PyTorch path: q|k normed only, ``rotated`` False.
    The v columns are bit-identical to the input.  ``gwq`` / ``gwk``: fp32 [hd] grad views the weight gradients are
    accumulated into (None: evaluation).  ``inplace=True`` lets the HIP path overwrite ``qkv`` and, in the backward,
    the gradient buffer it is handed (the model passes it for the projection output and the attention gradient it
    owns); otherwise both are copied first."""
    _check(qkv, wq, wk, nh, nkv, hd)
    if _ext.use_hip(qkv):
        x = qkv.contiguous()
        if not inplace and x.data_ptr() == qkv.data_ptr():
            x = x.clone()  # never overwrite a caller-visible tensor
        return QKNormRopeFn.apply(x, wq, wk, gwq, gwk, cos, sin, T, nh, nkv, hd, eps, bool(inplace)), True
    return QKNormFn.apply(qkv, wq, wk, gwq, gwk, nh, nkv, hd, eps), False
