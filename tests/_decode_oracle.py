"""float64 oracle of one decode-attention step, built from ``_oracle64`` (which it imports and does not change).

For sequence b the packed rows ``[len, (nh + 2 nkv) hd]``, ``len = pos[b] + 1``, are assembled AS THE TRAINING KERNELS
WOULD SEE THEM: rows ``0 .. pos-1`` carry the cache slots (k already rotated, v; their q is never read and is 0), the
last row is the new token's q|k|v rotated with ``_oracle64.rope`` at its position and rounded to the storage dtype
(bf16 on the GPU; ``round_dtype=None`` keeps it for the fp32 CPU path).  ``_oracle64.attention(..., kstart=...)`` on
these rows, last query row taken, is the reference; the fp32 twin is the same assembly through plain fp32 PyTorch.
Slots outside ``[kstart, pos)`` are never read by a correct kernel and may hold NaN sentinels: they are zeroed here
(the oracle multiplies masked probabilities, exact zeros, with them).  The error rule is ``_oracle64.check``.
"""
import torch

from . import _oracle64 as o64


def rotated_row(qkv_row, cos, sin, p, nh, nkv, hd, round_dtype=torch.bfloat16):
    """The new token's packed row [1, W] rotated at position ``p`` in float64, rounded to ``round_dtype``."""
    r = o64.rope(qkv_row.reshape(1, -1), cos[p:p + 1], sin[p:p + 1], 1, 1, nh, nkv, hd)
    return r.to(round_dtype).double() if round_dtype is not None else r


def assemble(qkv_row, kc, vc, p, ks, nh, nkv, hd, cos, sin, round_dtype=torch.bfloat16):
    """Packed float64 rows [p + 1, W] of one sequence: cache slots 0 .. p-1 (``kc`` / ``vc`` [nkv, S_max, hd]) and
    the rotated new row."""
    W = (nh + 2 * nkv) * hd
    rows = torch.zeros(p + 1, W, dtype=torch.float64, device=kc.device)
    if p > 0:
        live = (torch.arange(p, device=kc.device) >= ks)[:, None]
        k = kc[:, :p].double().transpose(0, 1).reshape(p, nkv * hd)
        v = vc[:, :p].double().transpose(0, 1).reshape(p, nkv * hd)
        rows[:p, nh * hd:(nh + nkv) * hd] = torch.where(live, k, torch.zeros_like(k))
        rows[:p, (nh + nkv) * hd:] = torch.where(live, v, torch.zeros_like(v))
    rows[p] = rotated_row(qkv_row, cos, sin, p, nh, nkv, hd, round_dtype)[0]
    return rows


def _last_row_fp32(rows, ks, nh, nkv, hd, scale):
    """softmax(scale q k^T) v of the last query row in plain fp32 PyTorch; [nh * hd]."""
    x = rows.float()
    n = x.shape[0]
    rep = nh // nkv
    q = x[-1, :nh * hd].reshape(nh, 1, hd)
    k = x[:, nh * hd:(nh + nkv) * hd].reshape(n, nkv, hd).transpose(0, 1).repeat_interleave(rep, dim=0)
    v = x[:, (nh + nkv) * hd:].reshape(n, nkv, hd).transpose(0, 1).repeat_interleave(rep, dim=0)
    s = (q @ k.transpose(-1, -2)) * o64.f32_scalar(scale)
    dead = (torch.arange(n, device=x.device) < ks).view(1, 1, n)
    p = torch.softmax(s.masked_fill(dead, float("-inf")), dim=-1)
    return (p @ v).reshape(nh * hd)


def decode_refs(qkv, kcache, vcache, pos, kstart, nh, nkv, hd, cos, sin, round_dtype=torch.bfloat16):
    """(ref64, twin32), each [B, nh * hd]: one decode step of every sequence.  ``qkv`` [B, W] un-rotated; the caches
    [B, nkv, S_max, hd] BEFORE the step (slot pos[b] is not read); ``pos`` / ``kstart`` host ints per sequence
    (``kstart`` None: 0).  A sequence whose kstart exceeds pos has no key: 0."""
    B = qkv.shape[0]
    scale = hd ** -0.5
    ref, twin = [], []
    for b in range(B):
        p = int(pos[b])
        ks = int(kstart[b]) if kstart is not None else 0
        rows = assemble(qkv[b], kcache[b], vcache[b], p, ks, nh, nkv, hd, cos, sin, round_dtype)
        kt = torch.tensor([ks], device=rows.device)
        ref.append(o64.attention(rows, 1, p + 1, nh, nkv, hd, scale, kstart=kt)["o"][-1])
        twin.append(_last_row_fp32(rows, ks, nh, nkv, hd, scale) if ks <= p
                    else torch.zeros(nh * hd, device=rows.device))
    return torch.stack(ref), torch.stack(twin)
