"""KV cache and single-query (decode) attention for text generation.

``KVCache`` holds, per layer, K and V as ``[B, nkv, S_max, hd]`` (each kv head's keys contiguous: a decode step
streams them front to back), one device ``pos`` int32 [B] (the slot and RoPE position of the NEXT token of every
sequence), one ``kstart`` int32 [B] (first real key under left padding, as in the training kernels) and the fp32
workspace of the split-KV partials (shared by the layers: they run one after the other on one stream).

``attention_decode(qkv, cache, layer, cos, sin)`` is one decode step of one layer: ``qkv`` [B, (nh + 2 nkv) hd] is
the plain (un-rotated) q|k|v projection of the new token; q and k are rotated at ``pos``, the rotated k and the v row
are written to slot ``pos`` and ``o = softmax(scale q k^T) v`` runs over keys ``kstart .. pos``.  ``pos`` is NOT advanced
(every layer of a step uses the same value); ``cache.advance()`` does that once per step.

HIP path (``csrc/attn_decode.hip``): ``nd_attn_decode`` -- RoPE, append and a split-KV single-query attention in one
launch plus a combine launch; static shapes, positions read on the device, so a step is HIP-graph capturable.  On the
CPU, or under ``--ops torch``, a PyTorch twin with the same contract runs (``reference.apply_rope`` at ``pos``, an
indexed slot write, masked SDPA over the whole cache); it is also the timing baseline.  The twin multiplies masked
probabilities (exact zeros) with whatever the unused slots hold, so it needs finite slots: ``KVCache`` starts zeroed.

``cache_fill`` is the prefill side: it copies the k|v columns of the training path's packed q|k|v buffer into slots
``0 .. T-1``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import _ext
from . import reference as ref

MAX_REP = 8  # query heads per kv head the decode kernel carries in registers
HEAD_DIMS = (32, 64, 128)


def decode_split() -> int:
    """Keys per workgroup of the decode kernel's fixed partition (compile-time ``SPLIT``)."""
    return int(_ext.lib().nd_attn_decode_split())


def decode_workspace(B: int, nh: int, hd: int, s_max: int, device, split: Optional[int] = None):
    """(part_o [B * nh * nchunks, hd], part_ml [B * nh * nchunks, 2]) fp32 for ``nd_attn_decode``."""
    split = split or decode_split()
    nchunks = (s_max + split - 1) // split
    return (torch.empty(B * nh * nchunks, hd, dtype=torch.float32, device=device),
            torch.empty(B * nh * nchunks, 2, dtype=torch.float32, device=device))


class KVCache:
    def __init__(self, config, batch: int, s_max: int, device, dtype: torch.dtype):
        c = config
        if batch < 1 or s_max < 1:
            raise ValueError("KVCache needs batch >= 1 and s_max >= 1")
        if s_max > c.max_position_embeddings:
            raise ValueError(f"s_max = {s_max} exceeds max_position_embeddings = {c.max_position_embeddings}")
        if c.num_attention_heads % c.num_key_value_heads:
            raise ValueError("num_attention_heads must be a multiple of num_key_value_heads")
        self.config = c
        self.batch, self.s_max = int(batch), int(s_max)
        self.device, self.dtype = torch.device(device), dtype
        self.nh, self.nkv, self.hd = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        # sliding window (None = off): a decode step sees keys max(kstart, pos - window + 1) .. pos.  The cache stays
        # static (s_max slots); only what a step reads shrinks
        self.window = int(getattr(c, "sliding_window", None) or 0) or None
        shape = (self.batch, self.nkv, self.s_max, self.hd)
        self.k = [torch.zeros(shape, dtype=dtype, device=self.device) for _ in range(c.num_hidden_layers)]
        self.v = [torch.zeros(shape, dtype=dtype, device=self.device) for _ in range(c.num_hidden_layers)]
        self.pos = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self.kstart = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        # host-side upper bound of pos: lets every step refuse a full cache without reading the device
        self.max_pos = 0
        self.part_o = self.part_ml = None
        if self.device.type == "cuda" and _ext.get_backend() != "torch":
            self.part_o, self.part_ml = decode_workspace(self.batch, self.nh, self.hd, self.s_max, self.device)

    def set_positions(self, pos, kstart=None) -> None:
        """Set ``pos`` (and ``kstart``; None: 0) from host sequences or tensors.  A setup call: a tensor ``pos`` is
        read back once for the host-side bound."""
        p = torch.as_tensor(pos, dtype=torch.int32).reshape(-1)
        if p.numel() != self.batch:
            raise ValueError(f"pos must have {self.batch} entries")
        lo, hi = int(p.min()), int(p.max())
        if lo < 0 or hi > self.s_max:
            raise ValueError(f"pos must lie in [0, s_max = {self.s_max}]")
        self.pos.copy_(p)
        self.max_pos = hi
        if kstart is None:
            self.kstart.zero_()
        else:
            ks = torch.as_tensor(kstart, dtype=torch.int32).reshape(-1)
            if ks.numel() != self.batch or int(ks.min()) < 0:
                raise ValueError(f"kstart must have {self.batch} non-negative entries")
            self.kstart.copy_(ks)

    def check_room(self) -> None:
        if self.max_pos >= self.s_max:
            raise ValueError(f"the KV cache is full: position {self.max_pos} with s_max = {self.s_max}")

    def advance(self, n: int = 1, device_side: bool = True) -> None:
        """One step done: ``pos += n`` on the device (no host sync).  ``device_side=False`` moves only the host-side
        bound -- for a replayed HIP graph whose captured step already holds the device increment."""
        if device_side:
            self.pos += n
        self.max_pos += n


def _check_cache_args(qkv, cos, sin, cache: KVCache, layer: int):
    W = (cache.nh + 2 * cache.nkv) * cache.hd
    if qkv.dim() != 2 or tuple(qkv.shape) != (cache.batch, W):
        raise ValueError(f"qkv must be [B, (nh + 2 nkv) hd] = [{cache.batch}, {W}], not {tuple(qkv.shape)}")
    if not 0 <= layer < len(cache.k):
        raise ValueError(f"layer {layer} outside the cache's {len(cache.k)} layers")
    if cos.shape[0] < cache.s_max or cos.shape[1] != cache.hd or cos.shape != sin.shape:
        raise ValueError(f"the RoPE tables must be [>= s_max = {cache.s_max}, hd = {cache.hd}]")
    cache.check_room()


def _check_window(window) -> Optional[int]:
    if window is None:
        return None
    if int(window) < 1:
        raise ValueError(f"decode attention: sliding window must be >= 1 (None = off), not {window}")
    return int(window)


def attn_decode_launch(qkv, cos, sin, pos, kstart, kcache, vcache, part_o, part_ml, nh: int, nkv: int, hd: int,
                       out: Optional[torch.Tensor] = None, window: Optional[int] = None) -> torch.Tensor:
    """``nd_attn_decode`` (``window``: ``nd_attn_decode_win``) on raw tensors; every shape, dtype, contiguity and
    alignment the kernel relies on is checked here, before the launch.  The positions live on the device and are NOT
    checked (``KVCache`` keeps a host-side bound for that); the kernel itself ignores a position outside the cache."""
    window = _check_window(window)
    if hd not in HEAD_DIMS:
        raise ValueError(f"decode attention: head_dim {hd} not in {HEAD_DIMS}")
    if nh < 1 or nkv < 1 or nh % nkv or nh // nkv > MAX_REP:
        raise ValueError(f"decode attention: nh = {nh}, nkv = {nkv}: need nh % nkv == 0 and nh / nkv <= {MAX_REP}")
    if kcache.dim() != 4 or kcache.shape != vcache.shape or kcache.shape[1] != nkv or kcache.shape[3] != hd:
        raise ValueError("decode attention: the caches must be [B, nkv, S_max, hd]")
    B, _, s_max, _ = kcache.shape
    if B < 1 or s_max < 1:
        raise ValueError("decode attention: empty cache")
    W = (nh + 2 * nkv) * hd
    if qkv.dim() != 2 or tuple(qkv.shape) != (B, W):
        raise ValueError(f"decode attention: qkv must be [{B}, {W}]")
    for name, t in (("qkv", qkv), ("kcache", kcache), ("vcache", vcache)):
        if t.dtype != torch.bfloat16 or not t.is_cuda:
            raise ValueError(f"decode attention: {name} must be a bf16 GPU tensor")
    if qkv.stride(1) != 1 or qkv.stride(0) < W or qkv.stride(0) % 8:
        raise ValueError("decode attention: qkv rows must be contiguous with a stride that is a multiple of 8")
    if not kcache.is_contiguous() or not vcache.is_contiguous():
        raise ValueError("decode attention: the caches must be contiguous")
    for name, t in (("cos", cos), ("sin", sin)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != hd \
                or t.shape[0] < s_max:
            raise ValueError(f"decode attention: {name} must be a contiguous fp32 [>= {s_max}, {hd}] GPU table")
    for name, t in (("pos", pos), ("kstart", kstart)):
        if t is None and name == "kstart":
            continue
        if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.numel() != B:
            raise ValueError(f"decode attention: {name} must be a contiguous int32 [{B}] GPU tensor")
    split = decode_split()
    nchunks = (s_max + split - 1) // split
    for name, t, cols in (("part_o", part_o, hd), ("part_ml", part_ml, 2)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() < B * nh * nchunks * cols:
            raise ValueError(f"decode attention: {name} must be a contiguous fp32 workspace of {B * nh * nchunks * cols}")
    if out is None:
        out = torch.empty(B, nh * hd, dtype=torch.bfloat16, device=qkv.device)
    elif out.dtype != torch.bfloat16 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (B, nh * hd):
        raise ValueError(f"decode attention: out must be a contiguous bf16 [{B}, {nh * hd}] GPU tensor")
    for name, t in (("qkv", qkv), ("cos", cos), ("sin", sin), ("kcache", kcache), ("vcache", vcache),
                    ("part_o", part_o), ("part_ml", part_ml)):
        if t.data_ptr() % 16:
            raise ValueError(f"decode attention: {name} must be 16-byte aligned")
    if window is not None:
        _ext.check(_ext.lib().nd_attn_decode_win(_ext.ptr(qkv), _ext.ptr(cos), _ext.ptr(sin), _ext.ptr(pos),
                                                 _ext.ptr(kstart), _ext.ptr(kcache), _ext.ptr(vcache), _ext.ptr(part_o),
                                                 _ext.ptr(part_ml), _ext.ptr(out), B, nh, nkv, hd, s_max, qkv.stride(0),
                                                 float(hd ** -0.5), min(window, 2 ** 31 - 1),
                                                 _ext.stream_ptr(qkv.device)), "nd_attn_decode_win")
        return out
    _ext.check(_ext.lib().nd_attn_decode(_ext.ptr(qkv), _ext.ptr(cos), _ext.ptr(sin), _ext.ptr(pos), _ext.ptr(kstart),
                                         _ext.ptr(kcache), _ext.ptr(vcache), _ext.ptr(part_o), _ext.ptr(part_ml),
                                         _ext.ptr(out), B, nh, nkv, hd, s_max, qkv.stride(0), float(hd ** -0.5),
                                         _ext.stream_ptr(qkv.device)), "nd_attn_decode")
    return out


def attention_decode_torch(qkv, cos, sin, pos, kstart, kcache, vcache, nh: int, nkv: int, hd: int,
                           window: Optional[int] = None) -> torch.Tensor:
    """The PyTorch twin on raw tensors (any device / float dtype); same contract as ``attn_decode_launch``."""
    window = _check_window(window)
    B, _, s_max, _ = kcache.shape
    q, k, v = qkv.split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    p = pos.long()
    c, s = cos[p].view(B, 1, 1, hd), sin[p].view(B, 1, 1, hd)  # each sequence's own table row
    q = ref.apply_rope(q.reshape(B, nh, 1, hd), c, s)
    k = ref.apply_rope(k.reshape(B, nkv, 1, hd), c, s)
    rows = torch.arange(B, device=qkv.device)
    kcache[rows, :, p] = k[:, :, 0]
    vcache[rows, :, p] = v.reshape(B, nkv, hd)
    t = torch.arange(s_max, device=qkv.device)
    lo = kstart.long().view(B, 1) if kstart is not None else torch.zeros(B, 1, dtype=torch.long, device=qkv.device)
    if window is not None:
        lo = torch.maximum(lo, p.view(B, 1) - window + 1)
    mask = ((t[None] >= lo) & (t[None] <= p.view(B, 1))).view(B, 1, 1, s_max)
    kk, vv = kcache, vcache
    if nkv != nh:
        kk = kk.repeat_interleave(nh // nkv, dim=1)
        vv = vv.repeat_interleave(nh // nkv, dim=1)
    o = F.scaled_dot_product_attention(q, kk, vv, attn_mask=mask)
    return o.reshape(B, nh * hd)


def attention_decode(qkv: torch.Tensor, cache: KVCache, layer: int, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """One decode step of layer ``layer``; see the module doc.  Returns o [B, nh * hd]."""
    _check_cache_args(qkv, cos, sin, cache, layer)
    if _ext.use_hip(qkv):
        if cache.part_o is None:
            cache.part_o, cache.part_ml = decode_workspace(cache.batch, cache.nh, cache.hd, cache.s_max, cache.device)
        return attn_decode_launch(qkv, cos, sin, cache.pos, cache.kstart, cache.k[layer], cache.v[layer], cache.part_o,
                                  cache.part_ml, cache.nh, cache.nkv, cache.hd, window=cache.window)
    return attention_decode_torch(qkv, cos, sin, cache.pos, cache.kstart, cache.k[layer], cache.v[layer], cache.nh,
                                  cache.nkv, cache.hd, window=cache.window)


def cache_fill(cache: KVCache, layer: int, qkv: torch.Tensor, B: int, T: int, cos=None, sin=None,
               rotated: bool = True) -> None:
    """Prefill: the k|v columns of the packed q|k|v buffer [B*T, (nh + 2 nkv) hd] into slots ``0 .. T-1``.
    ``rotated=True``: the k columns already carry RoPE (the HIP training path rotates the buffer in place, or in the
    projection GEMM's epilogue).  ``rotated=False`` (the PyTorch path leaves its input alone): k is rotated here, with
    the expression ``reference.attention_block`` uses.  A strided torch copy: not the hot path."""
    nh, nkv, hd = cache.nh, cache.nkv, cache.hd
    if B != cache.batch or T > cache.s_max:
        raise ValueError(f"a [{B}, {T}] prompt does not fit a KV cache of batch {cache.batch}, s_max {cache.s_max}")
    x = qkv.view(B, T, (nh + 2 * nkv) * hd)
    k = x[..., nh * hd:(nh + nkv) * hd].reshape(B, T, nkv, hd).transpose(1, 2)
    v = x[..., (nh + nkv) * hd:].reshape(B, T, nkv, hd).transpose(1, 2)
    if not rotated:
        k = ref.apply_rope(k, cos[:T], sin[:T])
    cache.k[layer][:, :, :T].copy_(k)
    cache.v[layer][:, :, :T].copy_(v)
