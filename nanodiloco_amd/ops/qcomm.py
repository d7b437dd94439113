"""Block-quantised transport of the DiLoCo pseudo-gradient: int8 / int4 codes with one fp32 scale per
256 elements (``csrc/qcomm.hip``; wire format in docs/DESIGN.md "Quantised outer transport").

  ``nd_pseudograd_q``      delta = theta_sync - theta_local, quantised in registers -> W wire chunks
  -- all-to-all: chunk w of every worker goes to worker w --
  ``nd_qreduce``           the W received chunks -> one requantised chunk holding their SUM
  -- all-gather of the reduced chunks --
  ``nd_outer_nesterov_q``  ``nd_outer_nesterov`` with d = (code * scale) / W read from the gathered chunks

Block quantiser (256 consecutive elements): ``amax = max|x|``, ``scale = amax / QMAX``,
``inv = QMAX / amax`` (0 for a zero block), ``code = clamp(rint(x * inv), -QMAX, QMAX)`` (half to even);
QMAX = 127 (int8) or 7 (int4).  A block holding an inf or a NaN gets a NaN scale and zero codes.

One wire chunk of ``c`` elements (a multiple of 256) is ``[codes: c*bits/8 bytes][scales: c/256 fp32]``;
a wire buffer is ``nchunks`` chunks back to back (uint8).  int4 codes are two's-complement nibbles, element
2i in the low nibble of byte i.

Error feedback (``pseudograd_q_ef`` / ``qreduce_ef``, docs/DESIGN.md "Error feedback"): the same two stages with
an fp32 residual ``e`` carried across outer steps -- ``x = fl(v + e)`` is quantised instead of ``v`` and
``e = fl(x - fl(code * scale))`` is what the receivers did not get.  With ``e = 0`` the wire bytes are those of
the stateless functions.

Every function has a PyTorch implementation with the identical operation order (CPU path).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _ext

QBLOCK = 256


def qmax(bits: int) -> int:
    if bits not in (8, 4):
        raise ValueError(f"quantised transport is int8 or int4, not {bits} bits")
    return 127 if bits == 8 else 7


def chunk_bytes(c: int, bits: int) -> int:
    """Wire bytes of one chunk of ``c`` elements: codes, then one fp32 scale per block."""
    qmax(bits)
    if c <= 0 or c % QBLOCK:
        raise ValueError("a wire chunk is a positive multiple of 256 elements")
    return c * bits // 8 + c // QBLOCK * 4


def chunk_elems(n: int, nchunks: int) -> int:
    """c = ceil(n / nchunks) rounded up to a multiple of 256 (at least one block)."""
    per = -(-max(n, 1) // nchunks)
    return -(-per // QBLOCK) * QBLOCK


def wire_views(buf: torch.Tensor, nchunks: int, c: int, bits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(codes, scales) views of a wire buffer: codes uint8 ``[nchunks, c*bits/8]``, scales fp32 ``[nchunks, c/256]``."""
    pb = chunk_bytes(c, bits)
    if buf.dtype != torch.uint8 or buf.dim() != 1 or buf.numel() != nchunks * pb or not buf.is_contiguous():
        raise ValueError(f"wire buffer must be contiguous uint8 of {nchunks} x {pb} bytes, got {tuple(buf.shape)} {buf.dtype}")
    cb = c * bits // 8
    b2 = buf.view(nchunks, pb)
    return b2[:, :cb], b2[:, cb:].view(torch.float32)


def _quantize_blocks(x: torch.Tensor, bits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """x fp32 ``[nb, 256]`` -> (codes int8 ``[nb, 256]``, scales fp32 ``[nb]``)."""
    q = float(qmax(bits))
    bad = ~torch.isfinite(x).all(dim=1)
    amax = torch.where(bad[:, None], torch.zeros((), dtype=x.dtype, device=x.device), x.abs()).amax(dim=1)
    live = (amax > 0) & ~bad
    safe = torch.where(live, amax, torch.ones_like(amax))
    # tensor / tensor: one correctly rounded division, like the kernel (`scalar / tensor` would be reciprocal * scalar)
    # kept finite like the kernel's: a tiny amax overflows the quotient, and 0 * inf would be NaN
    inv = torch.where(live, (torch.full_like(amax, q) / safe).clamp(max=torch.finfo(torch.float32).max),
                      torch.zeros_like(amax))
    codes = (x * inv[:, None]).round().clamp(-q, q)
    codes = torch.where(bad[:, None], torch.zeros_like(codes), codes).to(torch.int8)
    scale = torch.where(bad, torch.full_like(amax, float("nan")), amax / q)
    return codes, scale


def _pack(codes: torch.Tensor, bits: int) -> torch.Tensor:
    """int8 codes ``[..., m]`` -> wire bytes (uint8 ``[..., m*bits/8]``)."""
    u = codes.view(torch.uint8)
    if bits == 8:
        return u
    return (u[..., 0::2] & 0xF) | (u[..., 1::2] << 4)


def _unpack(wire: torch.Tensor, bits: int) -> torch.Tensor:
    """wire bytes -> codes as fp32 ``[..., m]``."""
    if bits == 8:
        return wire.contiguous().view(torch.int8).float()
    lo = ((wire & 0xF).to(torch.int16) ^ 8) - 8  # sign-extend a nibble
    hi = ((wire >> 4).to(torch.int16) ^ 8) - 8
    return torch.stack([lo, hi], dim=-1).flatten(-2).float()


def _store(out: torch.Tensor, nchunks: int, c: int, bits: int, codes: torch.Tensor, scale: torch.Tensor) -> None:
    oc, osc = wire_views(out, nchunks, c, bits)
    oc.copy_(_pack(codes.view(nchunks, c), bits))
    osc.copy_(scale.view(nchunks, c // QBLOCK))


def dequantize(buf: torch.Tensor, nchunks: int, c: int, bits: int) -> torch.Tensor:
    """fp32 ``[nchunks, c]``: ``code * scale`` of every element of a wire buffer (PyTorch; CPU path and tools)."""
    codes, scales = wire_views(buf, nchunks, c, bits)
    return _unpack(codes, bits) * scales.repeat_interleave(QBLOCK, dim=1)


def pseudograd_q(sync: torch.Tensor, master: torch.Tensor, out: torch.Tensor, nchunks: int, c: int, bits: int) -> None:
    """``out`` = the quantised ``sync - master`` as ``nchunks`` wire chunks of ``c`` elements; element i lies in
    chunk ``i // c``.  Elements past ``master.numel()`` count as zero; the fp32 difference is never stored."""
    n = master.numel()
    pb = chunk_bytes(c, bits)
    if sync.numel() != n or n > nchunks * c or out.numel() != nchunks * pb or out.dtype != torch.uint8:
        raise ValueError("pseudograd_q: span / wire buffer sizes do not match")
    if _ext.use_hip(master):
        _ext.check(_ext.lib().nd_pseudograd_q(_ext.ptr(sync), _ext.ptr(master), n, _ext.ptr(out), nchunks,
                                              c // QBLOCK, bits, _ext.stream_ptr(master.device)), "nd_pseudograd_q")
        return
    d = torch.zeros(nchunks * c, dtype=torch.float32, device=master.device)
    torch.sub(sync, master, out=d[:n])
    codes, scale = _quantize_blocks(d.view(-1, QBLOCK), bits)
    _store(out, nchunks, c, bits, codes, scale)


def _residual(x: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """x fp32 ``[nb, 256]`` minus what its codes deliver: ``x - code * scale``, two roundings (NaN for a NaN scale)."""
    return x - codes.float() * scale[:, None]


def pseudograd_q_ef(sync: torch.Tensor, master: torch.Tensor, resid: torch.Tensor, out: torch.Tensor, nchunks: int,
                    c: int, bits: int) -> None:
    """:func:`pseudograd_q` with error feedback: quantises ``(sync - master) + resid`` and rewrites ``resid``
    (fp32, ``master.numel()`` elements) in place with ``x - code * scale``.  Padding past the span holds no residual."""
    n = master.numel()
    pb = chunk_bytes(c, bits)
    if sync.numel() != n or n > nchunks * c or out.numel() != nchunks * pb or out.dtype != torch.uint8:
        raise ValueError("pseudograd_q_ef: span / wire buffer sizes do not match")
    if resid.numel() != n or resid.dtype != torch.float32 or not resid.is_contiguous() or resid.device != master.device:
        raise ValueError("pseudograd_q_ef: the residual is a contiguous fp32 tensor of the span's length")
    if _ext.use_hip(master):
        _ext.check(_ext.lib().nd_pseudograd_q_ef(_ext.ptr(sync), _ext.ptr(master), _ext.ptr(resid), n, _ext.ptr(out),
                                                 nchunks, c // QBLOCK, bits, _ext.stream_ptr(master.device)),
                   "nd_pseudograd_q_ef")
        return
    x = torch.zeros(nchunks * c, dtype=torch.float32, device=master.device)
    torch.sub(sync, master, out=x[:n])
    x[:n] += resid
    codes, scale = _quantize_blocks(x.view(-1, QBLOCK), bits)
    _store(out, nchunks, c, bits, codes, scale)
    resid.copy_(_residual(x.view(-1, QBLOCK), codes, scale).view(-1)[:n])


def qreduce(inp: torch.Tensor, nw: int, c: int, bits: int, out: torch.Tensor) -> None:
    """``inp``: ``nw`` received chunks in worker-rank order; ``out``: one chunk, the requantised
    ``sum_w code_w * scale_w`` (fp32, summed in rank order)."""
    pb = chunk_bytes(c, bits)
    if not 1 <= nw <= 64 or inp.numel() != nw * pb or out.numel() != pb or out.dtype != torch.uint8 \
            or inp.dtype != torch.uint8:
        raise ValueError("qreduce: wire buffer sizes do not match")
    if _ext.use_hip(inp):
        _ext.check(_ext.lib().nd_qreduce(_ext.ptr(inp), nw, c // QBLOCK, bits, _ext.ptr(out),
                                         _ext.stream_ptr(inp.device)), "nd_qreduce")
        return
    codes, scales = wire_views(inp, nw, c, bits)
    acc = torch.zeros(c, dtype=torch.float32, device=inp.device)
    for w in range(nw):
        acc = acc + _unpack(codes[w], bits) * scales[w].repeat_interleave(QBLOCK)
    q, scale = _quantize_blocks(acc.view(-1, QBLOCK), bits)
    _store(out, 1, c, bits, q, scale)


def qreduce_ef(inp: torch.Tensor, nw: int, c: int, bits: int, resid: torch.Tensor, out: torch.Tensor) -> None:
    """:func:`qreduce` with error feedback: the rank-order sum first, then ``+ resid`` (fp32, ``c`` elements), which
    is rewritten in place with what the requantised chunk does not deliver."""
    pb = chunk_bytes(c, bits)
    if not 1 <= nw <= 64 or inp.numel() != nw * pb or out.numel() != pb or out.dtype != torch.uint8 \
            or inp.dtype != torch.uint8:
        raise ValueError("qreduce_ef: wire buffer sizes do not match")
    if resid.numel() != c or resid.dtype != torch.float32 or not resid.is_contiguous() or resid.device != inp.device:
        raise ValueError("qreduce_ef: the residual is a contiguous fp32 tensor of one chunk's length")
    if _ext.use_hip(inp):
        _ext.check(_ext.lib().nd_qreduce_ef(_ext.ptr(inp), nw, c // QBLOCK, bits, _ext.ptr(resid), _ext.ptr(out),
                                            _ext.stream_ptr(inp.device)), "nd_qreduce_ef")
        return
    codes, scales = wire_views(inp, nw, c, bits)
    acc = torch.zeros(c, dtype=torch.float32, device=inp.device)
    for w in range(nw):
        acc = acc + _unpack(codes[w], bits) * scales[w].repeat_interleave(QBLOCK)
    x = (acc + resid).view(-1, QBLOCK)
    q, scale = _quantize_blocks(x, bits)
    _store(out, 1, c, bits, q, scale)
    resid.copy_(_residual(x, q, scale).view(-1))


def outer_nesterov_q(master: torch.Tensor, sync: torch.Tensor, gathered: torch.Tensor, nchunks: int, c: int, bits: int,
                     mom: torch.Tensor, shadow: Optional[torch.Tensor], inv_world: float, lr: float, momentum: float,
                     first: bool) -> None:
    """The outer Nesterov update (``ops.optim.outer_nesterov`` without drift) on one bucket whose pseudo-gradient sum is read from
    the gathered wire buffer: ``d = (code * scale) * inv_world``.  Touches ``master.numel()`` elements."""
    n = master.numel()
    if n > nchunks * c or gathered.numel() != nchunks * chunk_bytes(c, bits) or gathered.dtype != torch.uint8 \
            or sync.numel() != n or mom.numel() != n or (shadow is not None and shadow.numel() != n):
        raise ValueError("outer_nesterov_q: span / wire buffer sizes do not match")
    if _ext.use_hip(master):
        sh = shadow if (shadow is not None and shadow.data_ptr() != master.data_ptr()) else None
        _ext.check(_ext.lib().nd_outer_nesterov_q(
            _ext.ptr(master), _ext.ptr(sync), _ext.ptr(gathered), bits, c // QBLOCK, _ext.ptr(mom), _ext.ptr(sh),
            _ext.dtcode(sh) if sh is not None else 0, n, float(inv_world), float(lr), float(momentum),
            1 if first else 0, _ext.stream_ptr(master.device)), "nd_outer_nesterov_q")
        return
    # the kernel's order, which is torch.optim.SGD(nesterov=True)'s: every multiply-add is ONE add(alpha=...)
    d = dequantize(gathered, nchunks, c, bits).view(-1)[:n] * inv_world
    if first:
        mom.copy_(d)
    else:
        mom.mul_(momentum).add_(d)
    new = sync.add(d.add(mom, alpha=momentum), alpha=-lr)
    master.copy_(new)
    sync.copy_(new)
    if shadow is not None and shadow.data_ptr() != master.data_ptr():
        shadow.copy_(master)
