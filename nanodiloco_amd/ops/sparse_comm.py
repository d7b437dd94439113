"""Top-k sparse transport of the DiLoCo pseudo-gradient with error feedback (``csrc/sparse_comm.hip``; wire
format and rules in docs/DESIGN.md "Top-k sparse transport").

  ``nd_pseudograd_topk``      acc = (theta_sync - theta_local) + e; of every chunk of 4096 elements the k entries
                              with the largest |acc| go to this worker's wire slot, e keeps the rest
  -- all-gather of the W slots --
  ``nd_outer_nesterov_topk``  the W workers' entries summed per chunk in worker order, then ``nd_outer_nesterov``'s
                              update with d = sum / W on every element

Selection order: the key of an element is the int32 bit pattern of ``|acc|``; the larger key wins, and among equal
keys the lower index.  That is a total order, so the selected set is unique (NaN > inf > any finite value, -0 and
+0 tie).  The entries of a chunk are emitted in ascending index order.

One wire slot of ``n`` elements (``nchunks = ceil(n / 4096)``) is
``[uint16 idx[nchunks][k], padded to 16 B][val[nchunks][k], padded to 16 B]`` with fp32 or bf16 values; ``idx`` is
the position inside the chunk.  A chunk with fewer than k elements fills its unused entries with index ``0xFFFF``
and value 0.  The padding bytes are never written.

Residual: ``e = acc - float(sent)`` for a sent element (exact; zero for fp32 values), ``e = acc`` otherwise.

Every function has a PyTorch implementation with the identical operation order (CPU path).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _ext
from .optim import outer_nesterov

CHUNK = 4096
NO_INDEX = 0xFFFF
VALUE_DTYPES = (torch.float32, torch.bfloat16)


def _pad16(nbytes: int) -> int:
    return (nbytes + 15) // 16 * 16


def _check_format(k: int, value_dtype) -> int:
    if not 1 <= int(k) <= CHUNK:
        raise ValueError(f"top-k transport keeps 1 <= k <= {CHUNK} entries per chunk, not {k}")
    if value_dtype not in VALUE_DTYPES:
        raise ValueError(f"top-k values travel as torch.float32 or torch.bfloat16, not {value_dtype}")
    return 4 if value_dtype == torch.float32 else 2


def topk_chunks(n: int) -> int:
    return -(-int(n) // CHUNK)


def topk_slot_bytes(n: int, k: int, value_dtype) -> int:
    """Wire bytes of one worker's slot for a span of ``n`` elements."""
    vs = _check_format(k, value_dtype)
    nch = topk_chunks(n)
    return _pad16(nch * k * 2) + _pad16(nch * k * vs)


def slot_views(slot: torch.Tensor, n: int, k: int, value_dtype):
    """(idx int16 ``[nchunks, k]`` -- the uint16 indices, ``0xFFFF`` reads -1 --, val ``[nchunks, k]``) views of a slot."""
    vs = _check_format(k, value_dtype)
    nch = topk_chunks(n)
    if slot.dtype != torch.uint8 or slot.dim() != 1 or not slot.is_contiguous() \
            or slot.numel() != topk_slot_bytes(n, k, value_dtype):
        raise ValueError(f"a top-k slot of {n} elements, k={k}, is contiguous uint8 of "
                         f"{topk_slot_bytes(n, k, value_dtype)} bytes, got {tuple(slot.shape)} {slot.dtype}")
    off = _pad16(nch * k * 2)
    return slot[:nch * k * 2].view(torch.int16).view(nch, k), slot[off:off + nch * k * vs].view(value_dtype).view(nch, k)


def _chunk_lengths(n: int, device) -> torch.Tensor:
    nch = topk_chunks(n)
    m = torch.full((nch,), CHUNK, dtype=torch.int64, device=device)
    if nch:
        m[-1] = n - (nch - 1) * CHUNK
    return m


def pseudograd_topk(sync: torch.Tensor, master: torch.Tensor, resid: torch.Tensor, slot: torch.Tensor, k: int,
                    value_dtype) -> None:
    """``slot`` = the k largest entries per chunk of ``(sync - master) + resid``; ``resid`` (fp32, the span's
    length) is rewritten in place with what was not sent.  Chunks are counted from the start of the span."""
    n = master.numel()
    _check_format(k, value_dtype)
    if sync.numel() != n or resid.numel() != n or resid.dtype != torch.float32 or not resid.is_contiguous() \
            or resid.device != master.device:
        raise ValueError("pseudograd_topk: sync, master and the fp32 residual have the span's length")
    if slot.dtype != torch.uint8 or slot.numel() != topk_slot_bytes(n, k, value_dtype) or not slot.is_contiguous():
        raise ValueError("pseudograd_topk: the wire slot does not match the span (topk_slot_bytes)")
    if _ext.use_hip(master):
        _ext.check(_ext.lib().nd_pseudograd_topk(_ext.ptr(sync), _ext.ptr(master), _ext.ptr(resid), n, _ext.ptr(slot),
                                                 int(k), _ext.DT_F32 if value_dtype == torch.float32 else _ext.DT_BF16,
                                                 _ext.stream_ptr(master.device)), "nd_pseudograd_topk")
        return
    if n == 0:
        return
    dev = master.device
    nch = topk_chunks(n)
    acc = torch.sub(sync, master).add_(resid)  # two fp32 operations, in this order
    key = torch.full((nch * CHUNK,), -1, dtype=torch.int32, device=dev)  # past the span: below every real key
    key[:n] = acc.view(torch.int32) & 0x7FFFFFFF
    # stable descending sort = larger key first, lower index first among equals; then ascending index
    order = torch.sort(key.view(nch, CHUNK), dim=1, descending=True, stable=True).indices[:, :k]
    order = torch.sort(order, dim=1).values
    valid = order < _chunk_lengths(n, dev)[:, None]  # a short chunk: the rest of its k entries stay unused
    g = (order + torch.arange(nch, device=dev)[:, None] * CHUNK)[valid]
    sent = acc[g].to(value_dtype)
    idx, val = slot_views(slot, n, k, value_dtype)
    idx.copy_(torch.where(valid, order, torch.full_like(order, -1)).to(torch.int16))  # -1 = 0xFFFF
    val.zero_()
    val[valid] = sent
    acc[g] = acc[g] - sent.float()
    resid.copy_(acc)


def densify(gathered: torch.Tensor, nworkers: int, n: int, k: int, value_dtype) -> torch.Tensor:
    """fp32 ``[n]``: the entries of ``nworkers`` slots (back to back, worker order) summed into a dense span,
    worker by worker from zero (PyTorch; CPU path, tests and tools).  ``0xFFFF`` -- any index past its chunk's
    end -- is skipped."""
    sb = topk_slot_bytes(n, k, value_dtype)
    if gathered.dtype != torch.uint8 or gathered.numel() != nworkers * sb or nworkers < 1:
        raise ValueError(f"{nworkers} top-k slots of {n} elements, k={k}, are {nworkers} x {sb} bytes")
    dev = gathered.device
    dense = torch.zeros(n, dtype=torch.float32, device=dev)
    nch = topk_chunks(n)
    m = _chunk_lengths(n, dev)[:, None]
    first = torch.arange(nch, device=dev)[:, None] * CHUNK
    for r in range(nworkers):
        idx, val = slot_views(gathered[r * sb:(r + 1) * sb], n, k, value_dtype)
        idx = idx.to(torch.int64) & 0xFFFF
        ok = idx < m
        g = (idx + first)[ok]
        dense[g] = dense[g] + val[ok].float()  # one worker's indices are distinct
    return dense


def outer_nesterov_topk(master: torch.Tensor, sync: torch.Tensor, gathered: torch.Tensor, nworkers: int, k: int,
                        value_dtype, mom: torch.Tensor, shadow: Optional[torch.Tensor], inv_w: float, lr: float,
                        mu: float, first: bool) -> None:
    """The outer Nesterov update (``ops.outer_nesterov`` without drift) of one bucket whose pseudo-gradient sum is
    read from the gathered slots: ``d = densify(...) * inv_w``.  Dense: momentum decays on every element."""
    n = master.numel()
    if gathered.dtype != torch.uint8 or gathered.numel() != nworkers * topk_slot_bytes(n, k, value_dtype) \
            or nworkers < 1 or sync.numel() != n or mom.numel() != n or (shadow is not None and shadow.numel() != n):
        raise ValueError("outer_nesterov_topk: span / wire buffer sizes do not match")
    if _ext.use_hip(master):
        sh = shadow if (shadow is not None and shadow.data_ptr() != master.data_ptr()) else None
        _ext.check(_ext.lib().nd_outer_nesterov_topk(
            _ext.ptr(master), _ext.ptr(sync), _ext.ptr(gathered), int(nworkers), int(k),
            _ext.DT_F32 if value_dtype == torch.float32 else _ext.DT_BF16, _ext.ptr(mom), _ext.ptr(sh),
            _ext.dtcode(sh) if sh is not None else 0, n, float(inv_w), float(lr), float(mu), 1 if first else 0,
            _ext.stream_ptr(master.device)), "nd_outer_nesterov_topk")
        return
    outer_nesterov(master, sync, densify(gathered, nworkers, n, k, value_dtype), mom, shadow, inv_w, lr, mu, first)
