"""RoPE + causal flash attention on the packed QKV GEMM output (K4 + K6).

Input ``qkv`` is the fused q|k|v projection output ``[B*T, (nh + 2*nkv) * hd]`` (token-major, heads
packed).  The HIP path never transposes to ``[B, H, T, hd]``: the attention kernels take
(batch, head, token) strides and read 128-B head rows straight out of the packed buffer, and
write ``O`` as ``[B*T, nh*hd]`` -- exactly the o_proj GEMM input.

HIP path (RoPE: q|k rotated in place by one streaming pass -- no copy; dq/dk are un-rotated inside the
backward kernels' store epilogues, so the backward needs no extra pass)
  fwd: ``nd_rope_inplace`` then ``nd_attn_fwd``  -- MFMA flash attention, online softmax, saves LSE (fp32, log2 domain)
  bwd: ``nd_attn_bwd_fused`` = a query-parallel dQ kernel that also computes delta = rowsum(dO * O)
       and the dK/dV kernel's seeds, then a key-parallel dK/dV kernel (both recompute P from LSE; no
       atomics -> deterministic); ``nd_attn_bwd_pre`` + ``nd_attn_bwd`` is the unfused form.
``nd_rope_inplace`` (stand-alone rotation kernel) remains available for other callers.
Packed windows (several EOS-separated documents per sequence): ``doc_bounds`` gives every token the bounds of its
document and ``attention(..., doc_bounds=...)`` runs ``nd_attn_fwd_doc`` / ``nd_attn_bwd_fused_doc`` -- block-diagonal
causal attention in the same kernels, which skip the key / query tiles that lie wholly outside a block's documents.
Sliding window (``attention(..., window=W)``, W < T): ``nd_attn_fwd_win`` / ``nd_attn_bwd_fused_win`` -- query q sees keys
max(kstart, q - W + 1) .. q; the LDS-DMA kernels skip the key / query tiles that lie wholly outside a block's windows.
GQA (nkv < nh) is handled by head-index mapping inside the kernels (no K/V repetition).
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from . import _ext
from . import reference as ref

_TABLES: Dict[Tuple, Tuple[torch.Tensor, torch.Tensor]] = {}


def rope_cache(T: int, hd: int, theta: float, scaling, device) -> Tuple[torch.Tensor, torch.Tensor]:
    key = (T, hd, float(theta), repr(scaling), str(device))
    t = _TABLES.get(key)
    if t is None:
        cos, sin = ref.rope_tables(T, hd, theta, scaling, device="cpu")
        t = (cos.to(device).contiguous(), sin.to(device).contiguous())
        _TABLES[key] = t
    return t


def _rope(qkv, cos, sin, B, T, nh, nkv, hd, inverse):
    L = _ext.lib()
    _ext.check(L.nd_rope_inplace(_ext.ptr(qkv), _ext.dtcode(qkv), _ext.ptr(cos), _ext.ptr(sin), B * T, T,
                                 nh, nkv, hd, qkv.shape[1], 1 if inverse else 0, _ext.stream_ptr(qkv.device)),
               "nd_rope_inplace")


_FUSED_STATS = {"enabled": True}


def set_attn_fused_stats(enabled: bool) -> None:
    """Backward row statistics computed inside the dQ kernel (default) vs the separate
    delta / statistics kernels (A/B)."""
    _FUSED_STATS["enabled"] = bool(enabled)


class FlashAttnFn(torch.autograd.Function):
    """RoPE is applied to q|k IN PLACE in the packed projection output (one streaming pass, no copy):
    that buffer is this op's private input -- the projection's backward saved its input, not its
    output -- and it is saved here only after the rotation.  The backward kernels un-rotate dq/dk in
    their store epilogues (rope_mode 2), so the gradient returned is w.r.t. the raw projection."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, B, T, nh, nkv, hd, kstart=None, rotated=False, doc_start=None, doc_end=None,
                window=None):
        ld = qkv.shape[1]
        if not rotated:  # else the projection GEMM's epilogue already rotated q|k
            _rope(qkv, cos, sin, B, T, nh, nkv, hd, inverse=False)
        k = qkv[:, nh * hd:]
        v = qkv[:, (nh + nkv) * hd:]
        o = torch.empty(B * T, nh * hd, dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty(B, nh, T, dtype=torch.float32, device=qkv.device)
        L = _ext.lib()
        ks = _ext.ptr(kstart) if kstart is not None else 0
        if window is not None:  # a real window (< T): ops.attention never passes another
            _ext.check(L.nd_attn_fwd_win(_ext.ptr(qkv), _ext.ptr(k), _ext.ptr(v), _ext.ptr(o), _ext.ptr(lse),
                                         B, nh, nkv, T, hd, ld, nh * hd, 0, 0, float(hd ** -0.5), ks, int(window),
                                         _ext.stream_ptr(qkv.device)), "nd_attn_fwd_win")
        elif doc_start is not None:
            _ext.check(L.nd_attn_fwd_doc(_ext.ptr(qkv), _ext.ptr(k), _ext.ptr(v), _ext.ptr(o), _ext.ptr(lse),
                                         B, nh, nkv, T, hd, ld, nh * hd, 0, 0, float(hd ** -0.5), _ext.ptr(doc_start),
                                         _ext.ptr(doc_end), _ext.stream_ptr(qkv.device)), "nd_attn_fwd_doc")
        else:
            _ext.check(L.nd_attn_fwd_ks(_ext.ptr(qkv), _ext.ptr(k), _ext.ptr(v), _ext.ptr(o), _ext.ptr(lse),
                                        B, nh, nkv, T, hd, ld, nh * hd, 0, 0, float(hd ** -0.5), ks,
                                        _ext.stream_ptr(qkv.device)), "nd_attn_fwd_ks")
        ctx.save_for_backward(qkv, o, lse, cos, sin)
        ctx.kstart = kstart
        ctx.doc = (doc_start, doc_end) if doc_start is not None else None
        ctx.window = window
        ctx.dims = (B, T, nh, nkv, hd)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, cos, sin = ctx.saved_tensors
        B, T, nh, nkv, hd = ctx.dims
        do = do.contiguous()
        ld = qkv.shape[1]
        L = _ext.lib()
        dev = do.device
        ks = _ext.ptr(ctx.kstart) if ctx.kstart is not None else 0
        if ctx.window is not None:  # sliding window: the fused LDS-DMA backward is the only one
            if T % 64:
                raise ValueError(f"sliding-window attention has no backward for T % 64 != 0 (T = {T})")
            dqkv = torch.empty_like(qkv)
            k, v = qkv[:, nh * hd:], qkv[:, (nh + nkv) * hd:]
            dk, dv = dqkv[:, nh * hd:], dqkv[:, (nh + nkv) * hd:]
            ws = torch.empty(2, B, nh, T, dtype=torch.float32, device=dev)
            _ext.check(L.nd_attn_bwd_fused_win(_ext.ptr(qkv), _ext.ptr(k), _ext.ptr(v), _ext.ptr(o), _ext.ptr(do),
                                               _ext.ptr(lse), _ext.ptr(dqkv), _ext.ptr(dk), _ext.ptr(dv), _ext.ptr(ws),
                                               B, nh, nkv, T, hd, ld, nh * hd, _ext.ptr(cos), _ext.ptr(sin),
                                               float(hd ** -0.5), 2, ks, int(ctx.window), _ext.stream_ptr(dev)),
                       "nd_attn_bwd_fused_win")
            return (dqkv,) + (None,) * 12
        if ctx.doc is not None:  # document mode: the fused LDS-DMA backward is the only one
            dqkv = torch.empty_like(qkv)
            k, v = qkv[:, nh * hd:], qkv[:, (nh + nkv) * hd:]
            dk, dv = dqkv[:, nh * hd:], dqkv[:, (nh + nkv) * hd:]
            ws = torch.empty(2, B, nh, T, dtype=torch.float32, device=dev)
            _ext.check(L.nd_attn_bwd_fused_doc(_ext.ptr(qkv), _ext.ptr(k), _ext.ptr(v), _ext.ptr(o), _ext.ptr(do),
                                               _ext.ptr(lse), _ext.ptr(dqkv), _ext.ptr(dk), _ext.ptr(dv), _ext.ptr(ws),
                                               B, nh, nkv, T, hd, ld, nh * hd, _ext.ptr(cos), _ext.ptr(sin),
                                               float(hd ** -0.5), 2, _ext.ptr(ctx.doc[0]), _ext.ptr(ctx.doc[1]),
                                               _ext.stream_ptr(dev)), "nd_attn_bwd_fused_doc")
            return (dqkv,) + (None,) * 12
        if _FUSED_STATS["enabled"] and T % 64 == 0:
            # dQ kernel computes delta = rowsum(dO * O) itself and seeds the dK/dV kernel
            dqkv = torch.empty_like(qkv)
            k, v = qkv[:, nh * hd:], qkv[:, (nh + nkv) * hd:]
            dk, dv = dqkv[:, nh * hd:], dqkv[:, (nh + nkv) * hd:]
            ws = torch.empty(2, B, nh, T, dtype=torch.float32, device=dev)
            _ext.check(L.nd_attn_bwd_fused_ks(_ext.ptr(qkv), _ext.ptr(k), _ext.ptr(v), _ext.ptr(o), _ext.ptr(do),
                                              _ext.ptr(lse), _ext.ptr(dqkv), _ext.ptr(dk), _ext.ptr(dv), _ext.ptr(ws),
                                              B, nh, nkv, T, hd, ld, nh * hd, _ext.ptr(cos), _ext.ptr(sin),
                                              float(hd ** -0.5), 2, ks, _ext.stream_ptr(dev)), "nd_attn_bwd_fused_ks")
            return (dqkv,) + (None,) * 12
        delta = torch.empty(B, nh, T, dtype=torch.float32, device=dev)
        _ext.check(L.nd_attn_bwd_pre(_ext.ptr(o), _ext.ptr(do), _ext.ptr(delta), B, nh, T, hd, nh * hd,
                                     _ext.stream_ptr(dev)), "nd_attn_bwd_pre")
        dqkv = torch.empty_like(qkv)
        k, v = qkv[:, nh * hd:], qkv[:, (nh + nkv) * hd:]
        dk, dv = dqkv[:, nh * hd:], dqkv[:, (nh + nkv) * hd:]
        ws = torch.empty(2, B, nh, T, dtype=torch.float32, device=dev)  # -LSE/c, -delta for the dK/dV kernel
        _ext.check(L.nd_attn_bwd_ks(_ext.ptr(qkv), _ext.ptr(k), _ext.ptr(v), _ext.ptr(do), _ext.ptr(lse),
                                    _ext.ptr(delta), _ext.ptr(dqkv), _ext.ptr(dk), _ext.ptr(dv), _ext.ptr(ws),
                                    B, nh, nkv, T, hd, ld, nh * hd, _ext.ptr(cos), _ext.ptr(sin), float(hd ** -0.5), 2,
                                    ks, _ext.stream_ptr(dev)), "nd_attn_bwd_ks")
        return (dqkv,) + (None,) * 12


def key_start(attention_mask: torch.Tensor) -> torch.Tensor:
    """Per-sequence first real key (int32 [B]) of an HF ``attention_mask`` [B, T] (1 = token, 0 = pad).

    Left padding ([0..0, 1..1]) gives the pad count; right padding ([1..1, 0..0]) gives 0 -- causal
    attention already keeps every real query off the trailing pad keys.  Masks with holes (a pad
    between real tokens) are not expressible as a key start: ``check_padding`` rejects them."""
    m = attention_mask.to(torch.int32)
    return (m.cumsum(1) == 0).sum(1).to(torch.int32)


def check_padding(attention_mask: torch.Tensor) -> None:
    """Raise unless every row is left- or right-padded (one contiguous run of real tokens)."""
    m = attention_mask.to(torch.int32)
    transitions = (m[:, 1:] != m[:, :-1]).sum(1)
    if bool((transitions > 2).any()) or bool(((transitions == 2) & (m[:, 0] == 1)).any()):
        raise ValueError("attention_mask rows must be one contiguous run of tokens (left or right padding)")


def doc_bounds(input_ids: torch.Tensor, eos_token_id: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-token document bounds (int32 [B, T] each, on the ids' device) of a packed window.

    A token starts a document at t == 0 or right after an EOS (the EOS belongs to the document it ends):
    ``doc_start[b, t]`` is the index of the first token of t's document, ``doc_end[b, t]`` one past its last.
    A window that begins mid-document has its first document start at 0.  Static-shape ops only, no host sync
    (capturable in a HIP graph)."""
    B, T = input_ids.shape
    t = torch.arange(T, device=input_ids.device, dtype=torch.int64).expand(B, T)
    eos = input_ids == eos_token_id
    first = torch.ones(B, 1, dtype=torch.bool, device=input_ids.device)
    starts = torch.cat([first, eos[:, :-1]], dim=1)
    doc_start = torch.where(starts, t, torch.zeros_like(t)).cummax(dim=1).values
    ends = torch.where(eos, t + 1, torch.full_like(t, T))
    doc_end = ends.flip(1).cummin(dim=1).values.flip(1)
    return doc_start.to(torch.int32).contiguous(), doc_end.to(torch.int32).contiguous()


def check_doc_bounds(doc_start: torch.Tensor, doc_end: torch.Tensor) -> None:
    """Raise ValueError unless (doc_start, doc_end) describe consecutive documents: doc_start non-decreasing and
    constant inside a document, ``doc_start[t] <= t < doc_end[t] <= T``, and every document ending where the next
    one starts.  The attention kernels rely on this.  Synchronises with the host (``--debug-checks``, tests)."""
    if doc_start.shape != doc_end.shape or doc_start.dim() != 2:
        raise ValueError("doc_start / doc_end must both be [B, T]")
    if doc_start.dtype != torch.int32 or doc_end.dtype != torch.int32:
        raise ValueError("doc_start / doc_end must be int32")
    B, T = doc_start.shape
    ds, de = doc_start.long(), doc_end.long()
    t = torch.arange(T, device=ds.device).expand(B, T)

    def bad(cond, what):
        if bool(cond.any()):
            raise ValueError(f"invalid document bounds: {what}")

    bad((ds < 0) | (ds > t), "doc_start[t] must lie in [0, t]")
    bad((de <= t) | (de > T), "doc_end[t] must lie in (t, T]")
    bad(ds[:, 1:] < ds[:, :-1], "doc_start must be non-decreasing")
    bad(de[:, 1:] < de[:, :-1], "doc_end must be non-decreasing")
    bad((ds[:, 1:] != ds[:, :-1]) & (ds[:, 1:] != t[:, 1:]), "doc_start must be constant inside a document")
    bad((de[:, :-1] != de[:, 1:]) & (de[:, :-1] != t[:, 1:]), "doc_end must be constant inside a document")
    # both describe the same documents: the one that starts at doc_start[t] ends at doc_end[t] and vice versa
    bad(de.gather(1, ds) != de, "doc_end differs inside a document")
    bad(ds.gather(1, de - 1) != ds, "doc_start differs inside a document")


def attention(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, B: int, T: int, nh: int, nkv: int,
              hd: int, inplace: bool = False, kstart: torch.Tensor = None, rotated: bool = False,
              doc_bounds: Tuple[torch.Tensor, torch.Tensor] = None, window: int = None) -> torch.Tensor:
    """Causal self-attention with RoPE; qkv [B*T, (nh+2nkv)*hd] -> [B*T, nh*hd].

    ``kstart`` (int32 [B], from :func:`key_start`) masks left padding: real queries (t >= kstart[b])
    never see the pad keys t' < kstart[b] -- the reference's causal + padding mask
    (REF/nanodiloco/main.py:79-88,109 -> HF SDPA).  ``inplace=True`` lets the HIP path rotate q|k
    inside ``qkv`` itself (the model passes it for the projection output it owns); otherwise a private
    copy is rotated.  ``rotated=True``: q|k already carry RoPE (the projection GEMM's epilogue,
    ops/linear.py LinearRopeFn); the backward still returns the gradient w.r.t. the un-rotated q|k.
    ``doc_bounds`` ((doc_start, doc_end) from :func:`doc_bounds`): block-diagonal causal attention for packed
    windows -- query q attends to keys doc_start[b, q] <= k <= q.  RoPE positions are not reset at document starts
    (scores depend on q - k only).  Not combinable with ``kstart``; the HIP path needs T % 64 == 0.
    ``window`` (None / 0 = off): sliding-window attention -- query q attends to keys
    max(kstart[b], q - window + 1) <= k <= q, the query itself counted (HF ``sliding_window``).  Composes with
    ``kstart``, not with ``doc_bounds``.  ``window >= T`` is no window: today's path, bit for bit.  The HIP path
    has no windowed backward for T % 64 != 0 (forward only, e.g. prefill): a gradient there is refused up front."""
    if rotated and not qkv.is_cuda:
        raise ValueError("rotated=True is a GPU-path contract (fused RoPE GEMM epilogue)")
    if window is not None and window < 0:
        raise ValueError(f"sliding window must be >= 1 (None / 0 = off), not {window}")
    if window and doc_bounds is not None:
        raise ValueError("a sliding window and doc_bounds (packed documents) cannot be combined")
    window = int(window) if window and window < T else None
    if kstart is not None and doc_bounds is not None:
        raise ValueError("kstart (left padding) and doc_bounds (packed documents) cannot be combined")
    if doc_bounds is not None:
        ds, de = doc_bounds
        if tuple(ds.shape) != (B, T) or tuple(de.shape) != (B, T):
            raise ValueError(f"doc_bounds must be two [B, T] = [{B}, {T}] tensors")
    if _ext.use_hip(qkv):
        if doc_bounds is not None and T % 64:
            raise ValueError(f"document-masked attention needs T % 64 == 0 on the HIP path (T = {T})")
        if window is not None:
            if hd not in (32, 64, 128):
                raise ValueError(f"sliding-window attention: head_dim {hd} not in (32, 64, 128)")
            if T % 64 and torch.is_grad_enabled() and qkv.requires_grad:
                raise ValueError(f"sliding-window attention has no backward for T % 64 != 0 on the HIP path (T = {T}); "
                                 "run the forward under no_grad")
        x = qkv.contiguous()
        if not inplace and x.data_ptr() == qkv.data_ptr():
            x = x.clone()  # never rotate a caller-visible tensor
        if doc_bounds is not None:
            ds = ds.to(device=qkv.device, dtype=torch.int32).contiguous()
            de = de.to(device=qkv.device, dtype=torch.int32).contiguous()
            return FlashAttnFn.apply(x, cos, sin, B, T, nh, nkv, hd, None, bool(rotated), ds, de)
        ks = kstart.to(device=qkv.device, dtype=torch.int32).contiguous() if kstart is not None else None
        if window is not None:
            return FlashAttnFn.apply(x, cos, sin, B, T, nh, nkv, hd, ks, bool(rotated), None, None, window)
        return FlashAttnFn.apply(x, cos, sin, B, T, nh, nkv, hd, ks, bool(rotated))
    return ref.attention_block(qkv, cos, sin, B, T, nh, nkv, hd, use_sdpa=True, kstart=kstart, doc_bounds=doc_bounds,
                               window=window)
