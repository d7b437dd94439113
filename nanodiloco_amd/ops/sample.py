"""Token sampling for generation: temperature, top-k, top-p and the draw.

``sample(logits, u, temperature, top_k=0, top_p=1.0, return_stats=False)``: ``logits`` fp32 [B, V], ``u`` fp32 [B] with
every value in [0, 1) (one uniform number per row: the caller owns the generator); returns the token ids int64 [B], with
``return_stats`` also ``thr`` fp32 [B] (the smallest kept logit, as the input value) and ``nkept`` int32 [B].

Contract, with ``x = logits / temperature`` (the kept set is ``models.llama.filter_logits``', stated without a sort):

* top-k (``0 < top_k < V``): keep every token whose logit is >= the k-th largest; ties at the threshold all stay.
* top-p (``top_p < 1``, on what top-k kept): Z the kept mass, G(v) the mass of the kept logits strictly greater than v;
  the threshold is the smallest kept logit v with ``G(v) / Z < top_p``; keep every logit >= it.
* draw: over the kept tokens in index order, masses ``m_i``, total ``Z'``: the smallest kept index whose inclusive
  prefix mass exceeds ``u Z'``.
* ``-inf`` logits are legal (mass 0, never returned).  A row of ``-inf`` only, or with a NaN, is outside the contract.

HIP path (``csrc/sample.hip``, ``nd_sample_topk_topp``): one launch, one workgroup per row, radix selects for both
thresholds on 64-bit fixed-point masses; a row's result does not depend on B.  On the CPU, or under ``--ops torch``, a
PyTorch twin with the same contract runs: the ``topk`` threshold, float64 masses, and a bisection on the mass-above
definition over the logits' order-preserving integer keys -- no sort.  The two agree up to the rounding of the masses
(the kernel's are fp32 exponentials rounded to 2^-40), not bit for bit.
"""
from __future__ import annotations

import math

import torch

from . import _ext

MAX_V = 1 << 20  # the kernel's 2^40-scaled masses are summed in a uint64


def _check(logits, u, temperature, top_k, top_p):
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"sample: logits must be fp32 [B, V], not {logits.dtype} {tuple(logits.shape)}")
    B, V = logits.shape
    if V > MAX_V:
        raise ValueError(f"sample: V = {V} exceeds {MAX_V}")
    if u.dtype != torch.float32 or tuple(u.shape) != (B,) or u.device != logits.device:
        raise ValueError(f"sample: u must be fp32 [{B}] on the logits' device, not {u.dtype} {tuple(u.shape)}")
    if not (isinstance(temperature, (int, float)) and temperature > 0 and math.isfinite(temperature)):
        raise ValueError(f"sample: temperature must be a finite number > 0, not {temperature!r} (0 is greedy: argmax)")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"sample: top_k must be an integer >= 0 (0 = off), not {top_k!r}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"sample: top_p must lie in (0, 1] (1 = off), not {top_p!r}")
    return B, V


def _launch(logits, u, temperature, top_k, top_p, return_stats):
    """``nd_sample_topk_topp``; what the kernel relies on beyond ``_check`` is checked here, before the launch."""
    B, V = logits.shape
    if not logits.is_cuda or logits.stride(1) != 1 or logits.stride(0) < V:
        raise ValueError("sample: logits must be a GPU tensor with contiguous rows and a row stride >= V")
    if not u.is_contiguous():
        raise ValueError("sample: u must be contiguous")
    if logits.data_ptr() % 4 or u.data_ptr() % 4:
        raise ValueError("sample: logits and u must be 4-byte aligned")
    tok = torch.empty(B, dtype=torch.int64, device=logits.device)
    thr = torch.empty(B, dtype=torch.float32, device=logits.device) if return_stats else None
    nkept = torch.empty(B, dtype=torch.int32, device=logits.device) if return_stats else None
    _ext.check(_ext.lib().nd_sample_topk_topp(_ext.ptr(logits), _ext.ptr(u), _ext.ptr(tok), _ext.ptr(thr),
                                              _ext.ptr(nkept), B, V, logits.stride(0), float(temperature),
                                              min(int(top_k), 2 ** 31 - 1), float(top_p),
                                              _ext.stream_ptr(logits.device)), "nd_sample_topk_topp")
    return (tok, thr, nkept) if return_stats else tok


def _keys(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> int64 in [0, 2^32) whose order is the float order (the kernel's keys; -0 joins +0)."""
    b = (x + 0.0).contiguous().view(torch.int32).long() & 0xFFFFFFFF
    return torch.where(b >= 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000)


def _twin(logits, u, temperature, top_k, top_p, return_stats):
    V = logits.shape[1]
    keep = torch.ones_like(logits, dtype=torch.bool)
    if 0 < top_k < V:
        keep = logits >= logits.topk(int(top_k), dim=-1).values[:, -1:]
    x = logits.double() / temperature
    m = torch.where(keep, (x - x.amax(-1, keepdim=True)).exp(), torch.zeros_like(x))
    if top_p < 1.0:
        # H(t) = the kept mass of keys > t falls as t rises: bisect for the smallest t with H(t) < top_p Z; the
        # threshold is the smallest kept key >= t
        key, bound = _keys(logits), top_p * m.sum(-1, keepdim=True)
        lo = torch.zeros_like(key[:, :1])
        hi = torch.full_like(lo, 0xFFFFFFFF)
        for _ in range(32):
            mid = (lo + hi) // 2
            ok = torch.where(key > mid, m, torch.zeros_like(m)).sum(-1, keepdim=True) < bound
            lo, hi = torch.where(ok, lo, mid + 1), torch.where(ok, mid, hi)
        keep = keep & (key >= lo)
        m = torch.where(keep, m, torch.zeros_like(m))
    cdf = m.cumsum(-1)
    tok = (cdf > u.double()[:, None] * cdf[:, -1:]).int().argmax(-1)
    if not return_stats:
        return tok
    thr = torch.where(keep, logits, torch.full_like(logits, float("inf"))).amin(-1)
    return tok, thr, keep.sum(-1).int()


def sample(logits: torch.Tensor, u: torch.Tensor, temperature: float, top_k: int = 0, top_p: float = 1.0,
           return_stats: bool = False):
    """One token id per row of ``logits``; see the module doc."""
    _check(logits, u, temperature, top_k, top_p)
    fn = _launch if _ext.use_hip(logits) else _twin
    return fn(logits, u, float(temperature), int(top_k), float(top_p), return_stats)
