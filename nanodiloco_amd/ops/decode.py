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

``attention_extend(qkv, cache, layer, cos, sin, L)`` is the multi-token step: ``qkv`` [B*L, (nh + 2 nkv) hd] holds L new
tokens per sequence (row ``b*L + i`` at slot and RoPE position ``pos[b] + i``); they are rotated, appended to slots
``pos .. pos+L-1`` and every query row ``i`` attends keys ``max(kstart, pos+i-window+1) .. pos+i``.  HIP path
(``csrc/attn_extend.hip``, ``nd_attn_extend``): an append launch, then per block of at most ``extend_qblock()`` queries
an MFMA split-KV attention launch over the decode kernel's key partition and a combine launch; a row's bits depend on
its query, its key range and the partition alone (not on L, B or how a run of tokens was cut into calls).  ``pos`` is
not advanced: ``cache.advance(L)``.

``cache_fill`` is the prefill side: it copies the k|v columns of the training path's packed q|k|v buffer into slots
``0 .. T-1``.

``KVCache(..., kv_dtype="fp8")`` stores every K row (after RoPE) and V row as ``hd`` e4m3 codes plus one int8 exponent
(``kv8_quantize`` / ``kv8_dequantize`` below are the format's definition; docs/DESIGN.md "fp8 KV cache"): ``k`` / ``v``
are uint8 ``[B, nkv, S_max, hd]`` and ``k_exp`` / ``v_exp`` int8 ``[B, nkv, S_max]``.  The three entry points dispatch on
the cache; the HIP path is ``csrc/attn_kv8.hip`` (``nd_attn_decode_kv8``, ``nd_attn_extend_kv8``, ``nd_kv8_fill``), the
PyTorch twin dequantises the cache, runs the bf16 twins with the new rows passed through the quantiser, and stores the
new rows' codes.  The fp8 kernels do not carry attention soft-capping: such a config is refused at construction.
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


def extend_qblock() -> int:
    """Queries per attention launch of ``nd_attn_extend`` (compile-time ``QBLOCK``): what its workspace is sized for."""
    return int(_ext.lib().nd_attn_extend_qblock())


def extend_workspace(B: int, nh: int, hd: int, s_max: int, device):
    """(part_o [B * nh * nchunks * qblock, hd], part_ml [.., 2]) fp32 for ``nd_attn_extend``."""
    n = B * nh * ((s_max + decode_split() - 1) // decode_split()) * extend_qblock()
    return (torch.empty(n, hd, dtype=torch.float32, device=device),
            torch.empty(n, 2, dtype=torch.float32, device=device))


KV_DTYPES = ("bf16", "fp8")
KV8_EXP_MIN, KV8_EXP_MAX = -100, 100


def kv8_quantize(rows: torch.Tensor):
    """The fp8 cache format: ``rows`` [..., hd] (any float dtype, taken as fp32) -> (codes uint8 [..., hd], exps int8
    [...]), value = code * 2^e.  Per row, amax = max |x| = f 2^k with f in [0.5, 1): e = k - 9 if f <= 0.875 else k - 8
    (the smallest e with amax 2^-e <= 448), clamped to [-100, 100]; e = 0 for a zero row.  code = e4m3(x 2^-e),
    round-to-nearest-even, saturating; the scaling is by a power of two, so the code is a pure function of the row.
    Outside the contract (as the kernels): a row with an infinity gets e = 100; a NaN stays out of the amax and
    becomes the NaN code."""
    x = rows.float()
    amax = x.abs().nan_to_num(nan=0.0).amax(-1)
    f, k = torch.frexp(amax)
    e = torch.where(f <= 0.875, k - 9, k - 8)
    e = torch.where(torch.isinf(amax), torch.full_like(e, KV8_EXP_MAX), e).clamp(KV8_EXP_MIN, KV8_EXP_MAX)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    scaled = torch.ldexp(x, -e[..., None]).clamp(-448.0, 448.0)  # the cast alone would turn > 448 into NaN
    return scaled.to(torch.float8_e4m3fn).view(torch.uint8), e.to(torch.int8)


def kv8_dequantize(codes: torch.Tensor, exps: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """code * 2^e: exact in fp32 and in bf16 (4 significant bits, never below the smallest normal)."""
    return torch.ldexp(codes.view(torch.float8_e4m3fn).float(), exps.int()[..., None]).to(dtype)


class KVCache:
    def __init__(self, config, batch: int, s_max: int, device, dtype: torch.dtype, kv_dtype: str = "bf16"):
        c = config
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"KVCache: kv_dtype must be one of {KV_DTYPES}, not {kv_dtype!r}")
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
        # attention soft-cap (None = off): the decode scores are capped as the training kernels cap theirs
        self.softcap = ref.check_attn_softcap(getattr(c, "attn_logit_softcapping", None))
        self.kv_dtype = kv_dtype
        shape = (self.batch, self.nkv, self.s_max, self.hd)
        layers = range(c.num_hidden_layers)
        if kv_dtype == "fp8":
            if self.softcap is not None:
                raise ValueError("KVCache: kv_dtype='fp8' does not support attn_logit_softcapping (the fp8 cache "
                                 "kernels carry no soft-cap); use kv_dtype='bf16'")
            self.k = [torch.zeros(shape, dtype=torch.uint8, device=self.device) for _ in layers]
            self.v = [torch.zeros(shape, dtype=torch.uint8, device=self.device) for _ in layers]
            self.k_exp = [torch.zeros(shape[:3], dtype=torch.int8, device=self.device) for _ in layers]
            self.v_exp = [torch.zeros(shape[:3], dtype=torch.int8, device=self.device) for _ in layers]
        else:
            self.k = [torch.zeros(shape, dtype=dtype, device=self.device) for _ in layers]
            self.v = [torch.zeros(shape, dtype=dtype, device=self.device) for _ in layers]
            self.k_exp = self.v_exp = None
        self.pos = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self.kstart = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        # host-side upper bound of pos: lets every step refuse a full cache without reading the device
        self.max_pos = 0
        self.part_o = self.part_ml = None
        if self.device.type == "cuda" and _ext.get_backend() != "torch":
            self.part_o, self.part_ml = decode_workspace(self.batch, self.nh, self.hd, self.s_max, self.device)
        self.ext_o = self.ext_ml = None  # attention_extend's workspace, allocated at its first use

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

    def check_room(self, n: int = 1) -> None:
        if self.max_pos + n > self.s_max:
            raise ValueError(f"the KV cache is full: position {self.max_pos} + {n} with s_max = {self.s_max}")

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
                       out: Optional[torch.Tensor] = None, window: Optional[int] = None,
                       softcap: Optional[float] = None) -> torch.Tensor:
    """``nd_attn_decode`` (``window``: ``nd_attn_decode_win``; ``softcap``: ``nd_attn_decode_cap``) on raw tensors; every shape, dtype, contiguity and
    alignment the kernel relies on is checked here, before the launch.  The positions live on the device and are NOT
    checked (``KVCache`` keeps a host-side bound for that); the kernel itself ignores a position outside the cache."""
    window = _check_window(window)
    softcap = ref.check_attn_softcap(softcap)
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
    if softcap is not None:
        _ext.check(_ext.lib().nd_attn_decode_cap(_ext.ptr(qkv), _ext.ptr(cos), _ext.ptr(sin), _ext.ptr(pos),
                                                 _ext.ptr(kstart), _ext.ptr(kcache), _ext.ptr(vcache), _ext.ptr(part_o),
                                                 _ext.ptr(part_ml), _ext.ptr(out), B, nh, nkv, hd, s_max, qkv.stride(0),
                                                 float(hd ** -0.5), min(window or 0, 2 ** 31 - 1), softcap,
                                                 _ext.stream_ptr(qkv.device)), "nd_attn_decode_cap")
        return out
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


def _check_kv8_launch(tag, qkv, cos, sin, pos, kstart, kcodes, kexp, vcodes, vexp, part_o, part_ml, L, nh, nkv, hd, out):
    """Everything ``nd_attn_decode_kv8`` (``L`` None) / ``nd_attn_extend_kv8`` rely on; returns (B, s_max, out)."""
    if hd not in HEAD_DIMS:
        raise ValueError(f"{tag}: head_dim {hd} not in {HEAD_DIMS}")
    if nh < 1 or nkv < 1 or nh % nkv or nh // nkv > MAX_REP:
        raise ValueError(f"{tag}: nh = {nh}, nkv = {nkv}: need nh % nkv == 0 and nh / nkv <= {MAX_REP}")
    for name, t, dt in (("kcache", kcodes, torch.uint8), ("vcache", vcodes, torch.uint8), ("k_exp", kexp, torch.int8),
                        ("v_exp", vexp, torch.int8)):
        if t.dtype != dt or not t.is_cuda:
            raise ValueError(f"{tag}: {name} must be a {str(dt)[6:]} GPU tensor")
    if kcodes.dim() != 4 or kcodes.shape != vcodes.shape or kcodes.shape[1] != nkv or kcodes.shape[3] != hd:
        raise ValueError(f"{tag}: the code caches must be [B, nkv, S_max, hd]")
    B, _, s_max, _ = kcodes.shape
    if B < 1 or s_max < 1:
        raise ValueError(f"{tag}: empty cache")
    if tuple(kexp.shape) != (B, nkv, s_max) or tuple(vexp.shape) != (B, nkv, s_max):
        raise ValueError(f"{tag}: the exponents must be [B, nkv, S_max] = [{B}, {nkv}, {s_max}]")
    for name, t in (("kcache", kcodes), ("vcache", vcodes), ("k_exp", kexp), ("v_exp", vexp)):
        if not t.is_contiguous():
            raise ValueError(f"{tag}: {name} must be contiguous")
    n = 1 if L is None else L
    if n < 1 or n > s_max:
        raise ValueError(f"{tag}: L = {n} new tokens outside [1, s_max = {s_max}]")
    W = (nh + 2 * nkv) * hd
    if qkv.dim() != 2 or tuple(qkv.shape) != (B * n, W):
        raise ValueError(f"{tag}: qkv must be [{B * n}, {W}]")
    if qkv.dtype != torch.bfloat16 or not qkv.is_cuda:
        raise ValueError(f"{tag}: qkv must be a bf16 GPU tensor")
    if qkv.stride(1) != 1 or qkv.stride(0) < W or qkv.stride(0) % 8:
        raise ValueError(f"{tag}: qkv rows must be contiguous with a stride that is a multiple of 8")
    for name, t in (("cos", cos), ("sin", sin)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != hd \
                or t.shape[0] < s_max:
            raise ValueError(f"{tag}: {name} must be a contiguous fp32 [>= {s_max}, {hd}] GPU table")
    for name, t in (("pos", pos), ("kstart", kstart)):
        if t is None and name == "kstart":
            continue
        if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.numel() != B:
            raise ValueError(f"{tag}: {name} must be a contiguous int32 [{B}] GPU tensor")
    need = B * nh * ((s_max + decode_split() - 1) // decode_split()) * (1 if L is None else min(L, extend_qblock()))
    for name, t, cols in (("part_o", part_o, hd), ("part_ml", part_ml, 2)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() < need * cols:
            raise ValueError(f"{tag}: {name} must be a contiguous fp32 workspace of {need * cols}")
    if out is None:
        out = torch.empty(B * n, nh * hd, dtype=torch.bfloat16, device=qkv.device)
    elif out.dtype != torch.bfloat16 or not out.is_cuda or not out.is_contiguous() \
            or tuple(out.shape) != (B * n, nh * hd):
        raise ValueError(f"{tag}: out must be a contiguous bf16 [{B * n}, {nh * hd}] GPU tensor")
    for name, t in (("qkv", qkv), ("cos", cos), ("sin", sin), ("kcache", kcodes), ("vcache", vcodes),
                    ("part_o", part_o), ("part_ml", part_ml)):
        if t.data_ptr() % 16:
            raise ValueError(f"{tag}: {name} must be 16-byte aligned")
    return B, s_max, out


def attn_decode_kv8_launch(qkv, cos, sin, pos, kstart, kcodes, kexp, vcodes, vexp, part_o, part_ml, nh: int, nkv: int,
                           hd: int, out: Optional[torch.Tensor] = None, window: Optional[int] = None) -> torch.Tensor:
    """``nd_attn_decode_kv8`` on raw tensors: ``attn_decode_launch`` on an fp8 cache (codes uint8 [B, nkv, S_max, hd],
    exponents int8 [B, nkv, S_max]); every shape, dtype, contiguity and alignment is checked before the launch."""
    window = _check_window(window)
    B, s_max, out = _check_kv8_launch("fp8 decode attention", qkv, cos, sin, pos, kstart, kcodes, kexp, vcodes, vexp,
                                      part_o, part_ml, None, nh, nkv, hd, out)
    _ext.check(_ext.lib().nd_attn_decode_kv8(_ext.ptr(qkv), _ext.ptr(cos), _ext.ptr(sin), _ext.ptr(pos),
                                             _ext.ptr(kstart), _ext.ptr(kcodes), _ext.ptr(kexp), _ext.ptr(vcodes),
                                             _ext.ptr(vexp), _ext.ptr(part_o), _ext.ptr(part_ml), _ext.ptr(out), B, nh,
                                             nkv, hd, s_max, qkv.stride(0), float(hd ** -0.5),
                                             min(window or 0, 2 ** 31 - 1), _ext.stream_ptr(qkv.device)),
               "nd_attn_decode_kv8")
    return out


def attn_extend_kv8_launch(qkv, cos, sin, pos, kstart, kcodes, kexp, vcodes, vexp, part_o, part_ml, L: int, nh: int,
                           nkv: int, hd: int, out: Optional[torch.Tensor] = None,
                           window: Optional[int] = None) -> torch.Tensor:
    """``nd_attn_extend_kv8`` on raw tensors: ``attn_extend_launch`` on an fp8 cache (``qkv`` is overwritten: q and k
    rotated in place); checked like ``attn_decode_kv8_launch``."""
    window = _check_window(window)
    B, s_max, out = _check_kv8_launch("fp8 extend attention", qkv, cos, sin, pos, kstart, kcodes, kexp, vcodes, vexp,
                                      part_o, part_ml, int(L), nh, nkv, hd, out)
    _ext.check(_ext.lib().nd_attn_extend_kv8(_ext.ptr(qkv), _ext.ptr(cos), _ext.ptr(sin), _ext.ptr(pos),
                                             _ext.ptr(kstart), _ext.ptr(kcodes), _ext.ptr(kexp), _ext.ptr(vcodes),
                                             _ext.ptr(vexp), _ext.ptr(part_o), _ext.ptr(part_ml), _ext.ptr(out), B,
                                             int(L), nh, nkv, hd, s_max, qkv.stride(0), float(hd ** -0.5),
                                             min(window or 0, 2 ** 31 - 1), _ext.stream_ptr(qkv.device)),
               "nd_attn_extend_kv8")
    return out


def _kv8_twin(fn, cache, layer: int, slots: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """An fp8 cache through a bf16 twin ``fn(kcache, vcache, kv_round)``: the layer is dequantised, the new rows pass through the quantiser on
    their way into it (``kv_round``: they enter this step's attention as every later step sees them), and their codes
    and exponents are stored in ``slots`` ([B] or [B, L])."""
    kd = kv8_dequantize(cache.k[layer], cache.k_exp[layer], dt)
    vd = kv8_dequantize(cache.v[layer], cache.v_exp[layer], dt)
    new = {}

    def kv_round(k, v):  # k, v: the new rows as the twin indexes them into the cache, [B, (L,) nkv, hd]
        new["k"], new["v"] = kv8_quantize(k), kv8_quantize(v)
        return kv8_dequantize(*new["k"], dt), kv8_dequantize(*new["v"], dt)

    o = fn(kd, vd, kv_round)
    rows = torch.arange(cache.batch, device=slots.device).view(-1, *([1] * (slots.dim() - 1)))
    for codes, exps, (c, e) in ((cache.k[layer], cache.k_exp[layer], new["k"]), (cache.v[layer], cache.v_exp[layer], new["v"])):
        codes[rows, :, slots] = c
        exps[rows, :, slots] = e
    return o


def attention_decode_torch(qkv, cos, sin, pos, kstart, kcache, vcache, nh: int, nkv: int, hd: int,
                           window: Optional[int] = None, softcap: Optional[float] = None, kv_round=None) -> torch.Tensor:
    """The PyTorch twin on raw tensors (any device / float dtype); same contract as ``attn_decode_launch``.
    ``kv_round`` (the fp8 cache's twin): maps the new (k, v) rows to what is stored and attended."""
    window = _check_window(window)
    softcap = ref.check_attn_softcap(softcap)
    B, _, s_max, _ = kcache.shape
    q, k, v = qkv.split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    p = pos.long()
    c, s = cos[p].view(B, 1, 1, hd), sin[p].view(B, 1, 1, hd)  # each sequence's own table row
    q = ref.apply_rope(q.reshape(B, nh, 1, hd), c, s)
    k = ref.apply_rope(k.reshape(B, nkv, 1, hd), c, s)
    rows = torch.arange(B, device=qkv.device)
    knew, vnew = k[:, :, 0], v.reshape(B, nkv, hd)
    if kv_round is not None:
        knew, vnew = kv_round(knew, vnew)
    kcache[rows, :, p] = knew
    vcache[rows, :, p] = vnew
    t = torch.arange(s_max, device=qkv.device)
    lo = kstart.long().view(B, 1) if kstart is not None else torch.zeros(B, 1, dtype=torch.long, device=qkv.device)
    if window is not None:
        lo = torch.maximum(lo, p.view(B, 1) - window + 1)
    mask = ((t[None] >= lo) & (t[None] <= p.view(B, 1))).view(B, 1, 1, s_max)
    kk, vv = kcache, vcache
    if nkv != nh:
        kk = kk.repeat_interleave(nh // nkv, dim=1)
        vv = vv.repeat_interleave(nh // nkv, dim=1)
    if softcap is not None:  # SDPA cannot cap: a manual masked softmax in fp32
        z = softcap * torch.tanh(torch.matmul(q.float(), kk.float().transpose(-1, -2)) * (hd ** -0.5 / softcap))
        z = z.masked_fill(~mask, float("-inf"))
        live = mask.any(-1, keepdim=True)
        pr = torch.softmax(torch.where(live, z, torch.zeros_like(z)), dim=-1) * live
        return torch.matmul(pr, vv.float()).to(qkv.dtype).reshape(B, nh * hd)
    o = F.scaled_dot_product_attention(q, kk, vv, attn_mask=mask)
    return o.reshape(B, nh * hd)


def attention_decode(qkv: torch.Tensor, cache: KVCache, layer: int, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """One decode step of layer ``layer``; see the module doc.  Returns o [B, nh * hd]."""
    _check_cache_args(qkv, cos, sin, cache, layer)
    fp8 = cache.kv_dtype == "fp8"
    if _ext.use_hip(qkv):
        if cache.part_o is None:
            cache.part_o, cache.part_ml = decode_workspace(cache.batch, cache.nh, cache.hd, cache.s_max, cache.device)
        if fp8:
            return attn_decode_kv8_launch(qkv, cos, sin, cache.pos, cache.kstart, cache.k[layer], cache.k_exp[layer],
                                          cache.v[layer], cache.v_exp[layer], cache.part_o, cache.part_ml, cache.nh,
                                          cache.nkv, cache.hd, window=cache.window)
        return attn_decode_launch(qkv, cos, sin, cache.pos, cache.kstart, cache.k[layer], cache.v[layer], cache.part_o,
                                  cache.part_ml, cache.nh, cache.nkv, cache.hd, window=cache.window,
                                  softcap=cache.softcap)
    if fp8:
        return _kv8_twin(lambda kd, vd, rnd: attention_decode_torch(qkv, cos, sin, cache.pos, cache.kstart, kd, vd,
                                                                    cache.nh, cache.nkv, cache.hd, window=cache.window,
                                                                    kv_round=rnd),
                         cache, layer, cache.pos.long(), qkv.dtype)
    return attention_decode_torch(qkv, cos, sin, cache.pos, cache.kstart, cache.k[layer], cache.v[layer], cache.nh,
                                  cache.nkv, cache.hd, window=cache.window, softcap=cache.softcap)


def attn_extend_launch(qkv, cos, sin, pos, kstart, kcache, vcache, part_o, part_ml, L: int, nh: int, nkv: int, hd: int,
                       out: Optional[torch.Tensor] = None, window: Optional[int] = None,
                       softcap: Optional[float] = None) -> torch.Tensor:
    """``nd_attn_extend`` on raw tensors: L new tokens per sequence, ``qkv`` [B*L, (nh + 2 nkv) hd] (overwritten: q and
    k rotated in place).  Every shape, dtype, contiguity and alignment the kernels rely on is checked here, before the
    launch; the device positions are not (the kernels ignore a sequence whose L slots do not fit)."""
    window = _check_window(window)
    softcap = ref.check_attn_softcap(softcap)
    if hd not in HEAD_DIMS:
        raise ValueError(f"extend attention: head_dim {hd} not in {HEAD_DIMS}")
    if nh < 1 or nkv < 1 or nh % nkv or nh // nkv > MAX_REP:
        raise ValueError(f"extend attention: nh = {nh}, nkv = {nkv}: need nh % nkv == 0 and nh / nkv <= {MAX_REP}")
    if kcache.dim() != 4 or kcache.shape != vcache.shape or kcache.shape[1] != nkv or kcache.shape[3] != hd:
        raise ValueError("extend attention: the caches must be [B, nkv, S_max, hd]")
    B, _, s_max, _ = kcache.shape
    if B < 1 or s_max < 1:
        raise ValueError("extend attention: empty cache")
    if L < 1 or L > s_max:
        raise ValueError(f"extend attention: L = {L} new tokens outside [1, s_max = {s_max}]")
    W = (nh + 2 * nkv) * hd
    if qkv.dim() != 2 or tuple(qkv.shape) != (B * L, W):
        raise ValueError(f"extend attention: qkv must be [{B * L}, {W}]")
    for name, t in (("qkv", qkv), ("kcache", kcache), ("vcache", vcache)):
        if t.dtype != torch.bfloat16 or not t.is_cuda:
            raise ValueError(f"extend attention: {name} must be a bf16 GPU tensor")
    if qkv.stride(1) != 1 or qkv.stride(0) < W or qkv.stride(0) % 8:
        raise ValueError("extend attention: qkv rows must be contiguous with a stride that is a multiple of 8")
    if not kcache.is_contiguous() or not vcache.is_contiguous():
        raise ValueError("extend attention: the caches must be contiguous")
    for name, t in (("cos", cos), ("sin", sin)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != hd \
                or t.shape[0] < s_max:
            raise ValueError(f"extend attention: {name} must be a contiguous fp32 [>= {s_max}, {hd}] GPU table")
    for name, t in (("pos", pos), ("kstart", kstart)):
        if t is None and name == "kstart":
            continue
        if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.numel() != B:
            raise ValueError(f"extend attention: {name} must be a contiguous int32 [{B}] GPU tensor")
    need = B * nh * ((s_max + decode_split() - 1) // decode_split()) * min(L, extend_qblock())
    for name, t, cols in (("part_o", part_o, hd), ("part_ml", part_ml, 2)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() < need * cols:
            raise ValueError(f"extend attention: {name} must be a contiguous fp32 workspace of {need * cols}")
    if out is None:
        out = torch.empty(B * L, nh * hd, dtype=torch.bfloat16, device=qkv.device)
    elif out.dtype != torch.bfloat16 or not out.is_cuda or not out.is_contiguous() \
            or tuple(out.shape) != (B * L, nh * hd):
        raise ValueError(f"extend attention: out must be a contiguous bf16 [{B * L}, {nh * hd}] GPU tensor")
    for name, t in (("qkv", qkv), ("cos", cos), ("sin", sin), ("kcache", kcache), ("vcache", vcache),
                    ("part_o", part_o), ("part_ml", part_ml)):
        if t.data_ptr() % 16:
            raise ValueError(f"extend attention: {name} must be 16-byte aligned")
    _ext.check(_ext.lib().nd_attn_extend(_ext.ptr(qkv), _ext.ptr(cos), _ext.ptr(sin), _ext.ptr(pos), _ext.ptr(kstart),
                                         _ext.ptr(kcache), _ext.ptr(vcache), _ext.ptr(part_o), _ext.ptr(part_ml),
                                         _ext.ptr(out), B, L, nh, nkv, hd, s_max, qkv.stride(0), float(hd ** -0.5),
                                         min(window or 0, 2 ** 31 - 1), float(softcap or 0.0),
                                         _ext.stream_ptr(qkv.device)), "nd_attn_extend")
    return out


def attention_extend_torch(qkv, cos, sin, pos, kstart, kcache, vcache, L: int, nh: int, nkv: int, hd: int,
                           window: Optional[int] = None, softcap: Optional[float] = None, kv_round=None) -> torch.Tensor:
    """The PyTorch twin on raw tensors (any device / float dtype); same contract as ``attn_extend_launch`` except that
    ``qkv`` is left alone: rotation at ``pos + i``, slot writes by index, a masked fp32 softmax over the whole cache.
    ``kv_round``: as ``attention_decode_torch``."""
    window = _check_window(window)
    softcap = ref.check_attn_softcap(softcap)
    B, _, s_max, _ = kcache.shape
    q, k, v = qkv.view(B, L, -1).split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    slot = pos.long().view(B, 1) + torch.arange(L, device=qkv.device)  # [B, L]
    c, s = cos[slot].view(B, 1, L, hd), sin[slot].view(B, 1, L, hd)  # each token's own table row
    q = ref.apply_rope(q.reshape(B, L, nh, hd).transpose(1, 2), c, s)
    k = ref.apply_rope(k.reshape(B, L, nkv, hd).transpose(1, 2), c, s)
    rows = torch.arange(B, device=qkv.device).view(B, 1)
    knew, vnew = k.transpose(1, 2), v.reshape(B, L, nkv, hd)
    if kv_round is not None:
        knew, vnew = kv_round(knew, vnew)
    kcache[rows, :, slot] = knew.to(kcache.dtype)  # indexed [B, L, nkv, hd]
    vcache[rows, :, slot] = vnew.to(vcache.dtype)
    t = torch.arange(s_max, device=qkv.device)
    lo = kstart.long().view(B, 1) if kstart is not None else torch.zeros(B, 1, dtype=torch.long, device=qkv.device)
    lo = lo.expand(B, L)
    if window is not None:
        lo = torch.maximum(lo, slot - window + 1)
    mask = ((t >= lo[..., None]) & (t <= slot[..., None])).view(B, 1, L, s_max)
    kk, vv = kcache, vcache
    if nkv != nh:
        kk = kk.repeat_interleave(nh // nkv, dim=1)
        vv = vv.repeat_interleave(nh // nkv, dim=1)
    z = torch.matmul(q.float(), kk.float().transpose(-1, -2)) * hd ** -0.5
    if softcap is not None:
        z = softcap * torch.tanh(z / softcap)
    z = z.masked_fill(~mask, float("-inf"))
    live = mask.any(-1, keepdim=True)  # a pad query (slot < kstart) has no key: zeros, as the kernels
    pr = torch.softmax(torch.where(live, z, torch.zeros_like(z)), dim=-1) * mask
    o = torch.matmul(pr, vv.float()).to(qkv.dtype)
    return o.transpose(1, 2).reshape(B * L, nh * hd)


def attention_extend(qkv: torch.Tensor, cache: KVCache, layer: int, cos: torch.Tensor, sin: torch.Tensor,
                     L: int) -> torch.Tensor:
    """L new tokens per sequence through layer ``layer``; see the module doc.  Returns o [B*L, nh * hd]."""
    W = (cache.nh + 2 * cache.nkv) * cache.hd
    if L < 1 or qkv.dim() != 2 or tuple(qkv.shape) != (cache.batch * L, W):
        raise ValueError(f"qkv must be [B*L, (nh + 2 nkv) hd] = [{cache.batch * L}, {W}], not {tuple(qkv.shape)}")
    if not 0 <= layer < len(cache.k):
        raise ValueError(f"layer {layer} outside the cache's {len(cache.k)} layers")
    if cos.shape[0] < cache.s_max or cos.shape[1] != cache.hd or cos.shape != sin.shape:
        raise ValueError(f"the RoPE tables must be [>= s_max = {cache.s_max}, hd = {cache.hd}]")
    cache.check_room(L)
    fp8 = cache.kv_dtype == "fp8"
    if _ext.use_hip(qkv):
        if cache.ext_o is None:
            cache.ext_o, cache.ext_ml = extend_workspace(cache.batch, cache.nh, cache.hd, cache.s_max, cache.device)
        if fp8:
            return attn_extend_kv8_launch(qkv, cos, sin, cache.pos, cache.kstart, cache.k[layer], cache.k_exp[layer],
                                          cache.v[layer], cache.v_exp[layer], cache.ext_o, cache.ext_ml, L, cache.nh,
                                          cache.nkv, cache.hd, window=cache.window)
        return attn_extend_launch(qkv, cos, sin, cache.pos, cache.kstart, cache.k[layer], cache.v[layer], cache.ext_o,
                                  cache.ext_ml, L, cache.nh, cache.nkv, cache.hd, window=cache.window,
                                  softcap=cache.softcap)
    if fp8:
        slots = cache.pos.long().view(-1, 1) + torch.arange(L, device=qkv.device)
        return _kv8_twin(lambda kd, vd, rnd: attention_extend_torch(qkv, cos, sin, cache.pos, cache.kstart, kd, vd, L,
                                                                    cache.nh, cache.nkv, cache.hd, window=cache.window,
                                                                    kv_round=rnd),
                         cache, layer, slots, qkv.dtype)
    return attention_extend_torch(qkv, cos, sin, cache.pos, cache.kstart, cache.k[layer], cache.v[layer], L, cache.nh,
                                  cache.nkv, cache.hd, window=cache.window, softcap=cache.softcap)


def kv8_fill_launch(qkv, kcodes, kexp, vcodes, vexp, T: int, nh: int, nkv: int, hd: int) -> None:
    """``nd_kv8_fill`` on raw tensors: the k|v columns of the packed, rotated bf16 ``qkv`` [B*T, (nh + 2 nkv) hd]
    quantised into slots ``0 .. T-1``; checked before the launch like the attention launchers."""
    tag = "fp8 cache fill"
    if hd not in HEAD_DIMS or nh < 1 or nkv < 1 or nh % nkv or nh // nkv > MAX_REP:
        raise ValueError(f"{tag}: head_dim {hd} not in {HEAD_DIMS}, or nh = {nh}, nkv = {nkv} with nh / nkv > {MAX_REP}")
    for name, t, dt in (("kcache", kcodes, torch.uint8), ("vcache", vcodes, torch.uint8), ("k_exp", kexp, torch.int8),
                        ("v_exp", vexp, torch.int8)):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{tag}: {name} must be a contiguous {str(dt)[6:]} GPU tensor")
    if kcodes.dim() != 4 or kcodes.shape != vcodes.shape or kcodes.shape[1] != nkv or kcodes.shape[3] != hd:
        raise ValueError(f"{tag}: the code caches must be [B, nkv, S_max, hd]")
    B, _, s_max, _ = kcodes.shape
    if tuple(kexp.shape) != (B, nkv, s_max) or tuple(vexp.shape) != (B, nkv, s_max):
        raise ValueError(f"{tag}: the exponents must be [B, nkv, S_max] = [{B}, {nkv}, {s_max}]")
    W = (nh + 2 * nkv) * hd
    if T < 1 or T > s_max or qkv.dim() != 2 or tuple(qkv.shape) != (B * T, W):
        raise ValueError(f"{tag}: qkv must be [B*T, {W}] with 1 <= T <= s_max = {s_max}, not {tuple(qkv.shape)}")
    if qkv.dtype != torch.bfloat16 or not qkv.is_cuda or qkv.stride(1) != 1 or qkv.stride(0) < W or qkv.stride(0) % 8:
        raise ValueError(f"{tag}: qkv must be a bf16 GPU tensor, rows contiguous with a stride that is a multiple of 8")
    for name, t in (("qkv", qkv), ("kcache", kcodes), ("vcache", vcodes)):
        if t.data_ptr() % 16:
            raise ValueError(f"{tag}: {name} must be 16-byte aligned")
    _ext.check(_ext.lib().nd_kv8_fill(_ext.ptr(qkv), _ext.ptr(kcodes), _ext.ptr(kexp), _ext.ptr(vcodes), _ext.ptr(vexp),
                                      B, T, nh, nkv, hd, s_max, qkv.stride(0), _ext.stream_ptr(qkv.device)),
               "nd_kv8_fill")


def cache_fill(cache: KVCache, layer: int, qkv: torch.Tensor, B: int, T: int, cos=None, sin=None,
               rotated: bool = True) -> None:
    """Prefill: the k|v columns of the packed q|k|v buffer [B*T, (nh + 2 nkv) hd] into slots ``0 .. T-1``.
    ``rotated=True``: the k columns already carry RoPE (the HIP training path rotates the buffer in place, or in the
    projection GEMM's epilogue).  ``rotated=False`` (the PyTorch path leaves its input alone): k is rotated here, with
    the expression ``reference.attention_block`` uses.  A strided torch copy: not the hot path.  An fp8 cache
    quantises the rows on the way: ``nd_kv8_fill`` on the HIP path, ``kv8_quantize`` otherwise."""
    nh, nkv, hd = cache.nh, cache.nkv, cache.hd
    if B != cache.batch or T > cache.s_max:
        raise ValueError(f"a [{B}, {T}] prompt does not fit a KV cache of batch {cache.batch}, s_max {cache.s_max}")
    if cache.kv_dtype == "fp8" and _ext.use_hip(qkv):
        if not rotated:
            raise ValueError("cache_fill: the HIP fp8 fill takes an already rotated buffer")
        kv8_fill_launch(qkv, cache.k[layer], cache.k_exp[layer], cache.v[layer], cache.v_exp[layer], T, nh, nkv, hd)
        return
    x = qkv.view(B, T, (nh + 2 * nkv) * hd)
    k = x[..., nh * hd:(nh + nkv) * hd].reshape(B, T, nkv, hd).transpose(1, 2)
    v = x[..., (nh + nkv) * hd:].reshape(B, T, nkv, hd).transpose(1, 2)
    if not rotated:
        k = ref.apply_rope(k, cos[:T], sin[:T])
    if cache.kv_dtype == "fp8":
        for x, codes, exps in ((k, cache.k[layer], cache.k_exp[layer]), (v, cache.v[layer], cache.v_exp[layer])):
            c, e = kv8_quantize(x)
            codes[:, :, :T].copy_(c)
            exps[:, :, :T].copy_(e)
        return
    cache.k[layer][:, :, :T].copy_(k)
    cache.v[layer][:, :, :T].copy_(v)
