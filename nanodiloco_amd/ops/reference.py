"""Pure-PyTorch reference implementations of every hot op.

These are (a) the compute path on CPU (BASELINE config 1: CPU/gloo), (b) the fp32 numerics
oracle every HIP kernel is tested against, and (c) the explicit ``--ops torch`` baseline on GPU.
Semantics follow HF ``LlamaForCausalLM`` exactly (HF/models/llama/modeling_llama.py):

* RMSNorm upcasts to fp32, ``x * rsqrt(mean(x^2) + eps)``, casts back, then ``* w``  (:62-67)
* RoPE uses the half-split ``rotate_half`` convention, fp32 tables cast to the input dtype (:108-160)
* attention is causal SDPA with scale ``head_dim**-0.5`` and GQA by KV repetition (:226-281)
* SwiGLU MLP ``down(silu(gate(x)) * up(x))`` (:169-176)
* loss is mean token cross-entropy on fp32 logits over shifted labels, ignore_index=-100
  (HF/loss/loss_utils.py:32-71)
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


# ----------------------------------------------------------------------------- norms
def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    dt = x.dtype
    xf = x.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    y = xf * torch.rsqrt(var + eps)
    return w.to(dt) * y.to(dt) if w.dtype != torch.float32 else (w * y).to(dt)


def rmsnorm_hf(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """Literal HF order of operations: ``weight * hidden.to(input_dtype)``."""
    dt = x.dtype
    xf = x.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    return w * (xf * torch.rsqrt(var + eps)).to(dt)


def rmsnorm_backward(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float):
    """Returns (dx fp32, dw fp32) for y = w * x * rstd, all math in fp32."""
    xf, dyf, wf = x.float(), dy.float(), w.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    xhat = xf * rstd
    dw = (dyf * xhat).reshape(-1, x.shape[-1]).sum(0)
    g = dyf * wf
    dx = rstd * (g - xhat * (g * xhat).mean(-1, keepdim=True))
    return dx, dw


def qk_norm(qkv: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, nh: int, nkv: int, hd: int,
            eps: float) -> torch.Tensor:
    """QK-norm: RMSNorm over ``hd`` of every q and k head of packed rows [N, (nh + 2 nkv) * hd] (fp32 statistics,
    ``w * (x * rstd)`` rounded once to the input dtype, as ``rmsnorm``); the v columns pass through.  Out of place,
    autograd-capable."""
    N = qkv.shape[0]
    q, k, v = qkv.split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    q = rmsnorm(q.reshape(N, nh, hd), wq, eps).reshape(N, nh * hd)
    k = rmsnorm(k.reshape(N, nkv, hd), wk, eps).reshape(N, nkv * hd)
    return torch.cat([q, k, v], dim=-1)


def qk_norm_backward(dy: torch.Tensor, qkv: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, nh: int, nkv: int,
                     hd: int, eps: float):
    """(dx in the dtype of ``qkv``, dwq fp32, dwk fp32) of ``qk_norm`` for the gradient ``dy`` of its output; the v
    columns of ``dy`` pass through."""
    N = qkv.shape[0]
    x = qkv.split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    d = dy.split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    dq, dwq = rmsnorm_backward(d[0].reshape(N, nh, hd), x[0].reshape(N, nh, hd), wq, eps)
    dk, dwk = rmsnorm_backward(d[1].reshape(N, nkv, hd), x[1].reshape(N, nkv, hd), wk, eps)
    dx = torch.cat([dq.reshape(N, nh * hd).to(qkv.dtype), dk.reshape(N, nkv * hd).to(qkv.dtype),
                    d[2].to(qkv.dtype)], dim=-1)
    return dx, dwq, dwk


# ----------------------------------------------------------------------------- rope
def rope_inv_freq(head_dim: int, theta: float, scaling: Optional[dict] = None, device=None) -> torch.Tensor:
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64, device=device).float() / head_dim))
    if scaling:
        kind = scaling.get("rope_type", scaling.get("type", "default"))
        if kind == "linear":
            inv = inv / float(scaling["factor"])
        elif kind == "llama3":
            factor = float(scaling["factor"])
            lo, hi = float(scaling["low_freq_factor"]), float(scaling["high_freq_factor"])
            old = float(scaling["original_max_position_embeddings"])
            lo_wl, hi_wl = old / lo, old / hi
            wl = 2 * math.pi / inv
            inv_l = torch.where(wl > lo_wl, inv / factor, inv)
            smooth = (old / wl - lo) / (hi - lo)
            smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
            is_med = ~(wl < hi_wl) & ~(wl > lo_wl)
            inv = torch.where(is_med, smoothed, inv_l)
    return inv


def rope_tables(seq_len: int, head_dim: int, theta: float, scaling: Optional[dict] = None,
                device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 cos/sin of shape [T, head_dim] (HF ``cat(freqs, freqs)`` layout)."""
    inv = rope_inv_freq(head_dim, theta, scaling, device=device)
    pos = torch.arange(seq_len, dtype=torch.float32, device=device)
    freqs = torch.outer(pos, inv)
    emb = torch.cat([freqs, freqs], dim=-1)
    return emb.cos(), emb.sin()


def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], dim=-1)


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x: [B, H, T, hd]; cos/sin: [T, hd] fp32 (cast to x.dtype like HF)."""
    c, s = cos.to(x.dtype), sin.to(x.dtype)
    return x * c + rotate_half(x) * s


# ----------------------------------------------------------------------------- attention
def split_qkv(qkv: torch.Tensor, B: int, T: int, nh: int, nkv: int, hd: int):
    q, k, v = qkv.view(B, T, -1).split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    q = q.reshape(B, T, nh, hd).transpose(1, 2)
    k = k.reshape(B, T, nkv, hd).transpose(1, 2)
    v = v.reshape(B, T, nkv, hd).transpose(1, 2)
    return q, k, v


def causal_attention(q, k, v, scale: Optional[float] = None):
    """q: [B, H, T, hd], k/v: [B, Hkv, T, hd] -> [B, H, T, hd].  Explicit math (no SDPA) for the oracle."""
    B, H, T, hd = q.shape
    rep = H // k.shape[1]
    if rep > 1:
        k = k.repeat_interleave(rep, dim=1)
        v = v.repeat_interleave(rep, dim=1)
    scale = hd ** -0.5 if scale is None else scale
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    mask = torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1)
    s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.matmul(p, v.float()).to(q.dtype)


def padded_causal_mask(kstart: torch.Tensor, T: int) -> torch.Tensor:
    """Boolean [B, 1, T, T] (True = attend): causal & key is not a left pad (HF's sdpa mask).  Pad
    query rows are fully masked; torch SDPA returns 0 for them, as the attention kernels do."""
    t = torch.arange(T, device=kstart.device)
    causal = t[None, :] <= t[:, None]
    real_k = t.view(1, 1, T) >= kstart.view(-1, 1, 1).to(t.dtype)
    return (causal[None] & real_k).unsqueeze(1)


def doc_causal_mask(doc_start: torch.Tensor, T: int) -> torch.Tensor:
    """Boolean [B, 1, T, T] (True = attend): causal & key is inside the query's document of a packed window,
    ``doc_start[b, q] <= k <= q`` (``ops.attention.doc_bounds``).  Every query sees itself: no empty row."""
    t = torch.arange(T, device=doc_start.device)
    causal = t[None, :] <= t[:, None]
    same_doc = t.view(1, 1, T) >= doc_start.view(-1, T, 1).to(t.dtype)
    return (causal[None] & same_doc).unsqueeze(1)


def window_causal_mask(window: int, T: int, kstart: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """Boolean [B or 1, 1, T, T] (True = attend): causal & key inside the query's sliding window of ``window`` >= 1
    keys, the query itself included -- ``max(kstart[b], q - window + 1) <= k <= q`` (HF's
    ``kv_idx > q_idx - sliding_window``), composed with the left-padding key start when one is given."""
    if window < 1:
        raise ValueError(f"sliding window must be >= 1, not {window}")
    device = kstart.device if kstart is not None else device
    t = torch.arange(T, device=device)
    m = ((t[None, :] <= t[:, None]) & (t[None, :] > t[:, None] - window))[None]
    if kstart is not None:
        m = m & (t.view(1, 1, T) >= kstart.view(-1, 1, 1).to(t.dtype))
    return m.unsqueeze(1)


def attention_block(qkv: torch.Tensor, cos, sin, B: int, T: int, nh: int, nkv: int, hd: int,
                    use_sdpa: bool = True, kstart: torch.Tensor = None, doc_bounds=None,
                    window: Optional[int] = None) -> torch.Tensor:
    """qkv [B*T, (nh+2nkv)*hd] -> RoPE -> causal attention -> [B*T, nh*hd] (autograd-capable).
    ``kstart``: left-padding key start per sequence (see ``ops.attention.key_start``).
    ``doc_bounds``: (doc_start, doc_end) of a packed window (see ``ops.attention.doc_bounds``).
    ``window``: sliding window (None / 0 = off; composes with ``kstart``, not with ``doc_bounds``); a window of T or
    more keys is the whole prefix and takes the un-windowed path."""
    if window is not None and window < 0:
        raise ValueError(f"sliding window must be >= 1 (None / 0 = off), not {window}")
    if window and doc_bounds is not None:
        raise ValueError("a sliding window and doc_bounds (packed documents) cannot be combined")
    if not window or window >= T:
        window = None
    q, k, v = split_qkv(qkv, B, T, nh, nkv, hd)
    q = apply_rope(q, cos[:T], sin[:T])
    k = apply_rope(k, cos[:T], sin[:T])
    if kstart is not None and doc_bounds is not None:
        raise ValueError("kstart (left padding) and doc_bounds (packed documents) cannot be combined")
    if kstart is not None or doc_bounds is not None or window is not None:
        if window is not None:
            mask = window_causal_mask(window, T, kstart.to(qkv.device) if kstart is not None else None, qkv.device)
        else:
            mask = padded_causal_mask(kstart.to(qkv.device), T) if kstart is not None \
                else doc_causal_mask(doc_bounds[0].to(qkv.device), T)
        if nkv != nh:
            k = k.repeat_interleave(nh // nkv, dim=1)
            v = v.repeat_interleave(nh // nkv, dim=1)
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
        return o.transpose(1, 2).reshape(B * T, nh * hd)
    if use_sdpa:
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=(nkv != nh))
    else:
        o = causal_attention(q, k, v)
    return o.transpose(1, 2).reshape(B * T, nh * hd)


# ----------------------------------------------------------------------------- mlp
def swiglu(gate_up: torch.Tensor) -> torch.Tensor:
    g, u = gate_up.chunk(2, dim=-1)
    return F.silu(g) * u


def swiglu_backward(dy: torch.Tensor, gate_up: torch.Tensor) -> torch.Tensor:
    g, u = gate_up.float().chunk(2, dim=-1)
    dyf = dy.float()
    sg = torch.sigmoid(g)
    silu = g * sg
    dg = dyf * u * (sg * (1 + g * (1 - sg)))
    du = dyf * silu
    return torch.cat([dg, du], dim=-1).to(gate_up.dtype)


# ----------------------------------------------------------------------------- loss
def shift_labels(labels: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """HF ForCausalLMLoss shift: position t predicts labels[t+1]; last position ignored."""
    return F.pad(labels[:, 1:], (0, 1), value=ignore_index)


def softcap(x: torch.Tensor, cap: float) -> torch.Tensor:
    """Final-logit soft-capping ``cap * tanh(x / cap)`` in fp32 (docs/DESIGN.md "Logit soft-capping"); ``cap`` 0 / None
    = off: ``x`` as it is."""
    if not cap:
        return x
    return float(cap) * torch.tanh(x.float() / float(cap))


def cross_entropy_loss(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    return F.cross_entropy(logits.float().view(-1, logits.shape[-1]), targets.view(-1),
                           ignore_index=ignore_index, reduction="mean")
