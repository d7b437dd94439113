"""Weight-only projections for skinny M: ``out = x . dequant(codes, exps)^T`` (docs/DESIGN.md "fp8 weight-only
decode", "fp4 weight-only decode").

fp8: the weight format is the KV cache's (``ops.decode.kv8_quantize``): ``W`` [N, K] in groups of 128 along K, e4m3
codes uint8 [N, K] plus one int8 exponent per group [N, K / 128], value = code * 2^e.  ``quantize_weight`` /
``dequantize_weight`` are that definition on a 2-D weight.

fp4: the OCP MX block layout, groups of 32 along K: e2m1 codes, two to a byte, uint8 [N, K / 2] plus one int8
exponent per group [N, K / 32] (``quantize_weight_fp4`` / ``dequantize_weight_fp4``).  Much lossier than fp8: on a
Gaussian weight the relative Frobenius error is 0.119 against 0.0265.

``gemv_w8(x, codes, exps)`` / ``gemv_w4(x, codes, exps)``: ``x`` [M, K] bf16 -> [M, N] bf16 with fp32 accumulation.
HIP path (``csrc/gemv_w8.hip`` ``nd_gemv_w8``, ``csrc/gemv_w4.hip`` ``nd_gemv_w4``): M <= ``max_m()`` rows on MFMA,
the codes streamed once; a row's bits depend on that row, the weight, N and K alone.  Static shapes, no host sync, the
workspace is the caller's: capturable in a HIP graph.  On the CPU, or under ``--ops torch``, the PyTorch twin runs.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _ext
from .decode import KV8_EXP_MAX, KV8_EXP_MIN, kv8_dequantize, kv8_quantize

GROUP = 128  # fp8: codes per exponent; both formats: K is a multiple of it
FP4_GROUP = 32  # fp4: codes per exponent
FP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # e2m1 magnitudes by the low three bits of a nibble


class _Fmt(NamedTuple):
    name: str  # the op, and "nd_" + name the launcher
    pack: int  # weight elements per code byte
    group: int  # weight elements per exponent


_W8, _W4 = _Fmt("gemv_w8", 1, GROUP), _Fmt("gemv_w4", 2, FP4_GROUP)


def max_m() -> int:
    """Rows of ``x`` ``nd_gemv_w8`` and ``nd_gemv_w4`` take (compile-time ``MAX_M``)."""
    return int(_ext.lib().nd_gemv_w8_max_m())


def quantize_weight(w: torch.Tensor):
    """``w`` [N, K], K % 128 == 0 -> (codes uint8 [N, K], exps int8 [N, K / 128])."""
    if w.dim() != 2 or w.shape[1] < GROUP or w.shape[1] % GROUP:
        raise ValueError(f"fp8 weights need a 2-D weight with K a multiple of {GROUP}, not {tuple(w.shape)}")
    N, K = w.shape
    codes, exps = kv8_quantize(w.reshape(N, K // GROUP, GROUP))
    return codes.view(N, K), exps


def dequantize_weight(codes: torch.Tensor, exps: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    N, K = codes.shape
    return kv8_dequantize(codes.view(N, K // GROUP, GROUP), exps, dtype).view(N, K)


def quantize_weight_fp4(w: torch.Tensor):
    """``w`` [N, K], K % 128 == 0 (the fp8 rule: a model takes both formats or neither) -> (codes uint8 [N, K / 2],
    exps int8 [N, K / 32]).  Groups of 32 along K; element k is the low nibble of byte k / 2 for even k, the high
    nibble for odd k; a nibble's top bit is the sign, its low three bits index ``FP4_VALUES``; value = code * 2^e.
    Per group, amax = f 2^k with f in [0.5, 1): e = k - 3 if f <= 0.75 else k - 2 (the smallest e with amax 2^-e <= 6:
    the scaled amax lies in (3, 6]), clamped to [-100, 100]; e = 0 for a zero group.  Codes: round to nearest, ties
    to the even code, saturating at +-6.  e2m1 has no NaN: a non-finite weight raises ``ValueError``."""
    if w.dim() != 2 or w.shape[1] < GROUP or w.shape[1] % GROUP:
        raise ValueError(f"fp4 weights need a 2-D weight with K a multiple of {GROUP}, not {tuple(w.shape)}")
    N, K = w.shape
    x = w.float().reshape(N, K // FP4_GROUP, FP4_GROUP)
    if not bool(torch.isfinite(x).all()):
        raise ValueError("fp4 weights cannot hold a non-finite value")
    amax = x.abs().amax(-1)
    f, k = torch.frexp(amax)
    e = torch.where(f <= 0.75, k - 3, k - 2).clamp(KV8_EXP_MIN, KV8_EXP_MAX)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    a = torch.ldexp(x, -e[..., None]).abs().clamp(max=FP4_VALUES[-1])
    grid = torch.tensor(FP4_VALUES, device=w.device)
    mids = (grid[:-1] + grid[1:]) / 2
    idx = torch.bucketize(a, mids)  # midpoints below a: the nearest code, the lower one at a tie
    tie = mids[idx.clamp(max=mids.numel() - 1)] == a
    nib = (torch.where(tie & (idx % 2 == 1), idx + 1, idx) | (torch.signbit(x).long() << 3)).view(N, K // 2, 2)
    return (nib[..., 0] | (nib[..., 1] << 4)).to(torch.uint8), e.to(torch.int8)


def dequantize_weight_fp4(codes: torch.Tensor, exps: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """code * 2^e as [N, K]: exact in fp32 and in bf16 over the whole exponent range (a code has 2 significant bits,
    and 6 * 2^100 and 0.5 * 2^-100 are normal bf16 numbers)."""
    N, K = codes.shape[0], 2 * codes.shape[1]
    nib = torch.stack([codes & 15, codes >> 4], dim=-1).view(N, K).long()
    mag = torch.tensor(FP4_VALUES, device=codes.device)[nib & 7]
    val = torch.where(nib >= 8, -mag, mag).view(N, K // FP4_GROUP, FP4_GROUP)
    return torch.ldexp(val, exps.int()[..., None]).view(N, K).to(dtype)


def _splits(f: _Fmt, N: int, K: int) -> int:
    splits = int(getattr(_ext.lib(), f"nd_{f.name}_splits")(int(N), int(K)))
    if splits < 1:
        raise ValueError(f"{f.name}: bad weight shape [{N}, {K}]")
    return splits


def _workspace_numel(f: _Fmt, N: int, K: int) -> int:
    splits = _splits(f, N, K)
    return splits * max_m() * int(N) if splits > 1 else 0


def _workspace(f: _Fmt, N: int, K: int, device) -> Optional[torch.Tensor]:
    n = _workspace_numel(f, N, K)
    return torch.empty(n, dtype=torch.float32, device=device) if n else None


def _supported(f: _Fmt, x: torch.Tensor, codes: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and codes.dim() == 2 and _ext.use_hip(x)
            and 1 <= x.shape[0] <= max_m() and x.shape[1] == codes.shape[1] * f.pack and x.shape[1] % GROUP == 0)


def _launch(f: _Fmt, x, codes, exps, out: Optional[torch.Tensor], workspace: Optional[torch.Tensor]) -> torch.Tensor:
    cols = "K" if f.pack == 1 else f"K / {f.pack}"
    if codes.dim() != 2 or codes.dtype != torch.uint8 or not codes.is_cuda or not codes.is_contiguous():
        raise ValueError(f"{f.name}: codes must be a contiguous uint8 [N, {cols}] GPU tensor")
    N, K = codes.shape[0], codes.shape[1] * f.pack
    if N < 1 or K < GROUP or K % GROUP:
        raise ValueError(f"{f.name}: K = {K} must be a positive multiple of {GROUP} and N = {N} >= 1")
    if exps.dtype != torch.int8 or not exps.is_cuda or not exps.is_contiguous() or tuple(exps.shape) != (N, K // f.group):
        raise ValueError(f"{f.name}: exps must be a contiguous int8 [{N}, {K // f.group}] GPU tensor")
    if x.dim() != 2 or x.dtype != torch.bfloat16 or not x.is_cuda or x.shape[1] != K:
        raise ValueError(f"{f.name}: x must be a bf16 [M, {K}] GPU tensor")
    M = x.shape[0]
    if not 1 <= M <= max_m():
        raise ValueError(f"{f.name}: M = {M} outside [1, {max_m()}]")
    if x.stride(1) != 1 or (M > 1 and (x.stride(0) < K or x.stride(0) % 8)):
        raise ValueError(f"{f.name}: x rows must be contiguous with a stride that is a multiple of 8")
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    elif out.dtype != torch.bfloat16 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (M, N):
        raise ValueError(f"{f.name}: out must be a contiguous bf16 [{M}, {N}] GPU tensor")
    splits = _splits(f, N, K)
    if splits > 1:
        if workspace is None:
            workspace = _workspace(f, N, K, x.device)
        elif workspace.dtype != torch.float32 or not workspace.is_cuda or not workspace.is_contiguous() \
                or workspace.numel() < splits * max_m() * N:
            raise ValueError(f"{f.name}: workspace must be a contiguous fp32 GPU tensor of {splits * max_m() * N}")
    else:
        workspace = None
    for name, t in (("x", x), ("codes", codes), ("workspace", workspace)):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"{f.name}: {name} must be 16-byte aligned")
    launcher = getattr(_ext.lib(), "nd_" + f.name)
    _ext.check(launcher(_ext.ptr(x), _ext.ptr(codes), _ext.ptr(exps), _ext.ptr(out), _ext.ptr(workspace),
                        M, N, K, x.stride(0) if M > 1 else K, _ext.stream_ptr(x.device)), "nd_" + f.name)
    return out


def _into(y: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    if out is not None:
        out.copy_(y)
        return out
    return y


def gemv_w8_workspace_numel(N: int, K: int) -> int:
    """fp32 elements of workspace ``nd_gemv_w8`` needs for an [N, K] weight (0: its partition has one K slice)."""
    return _workspace_numel(_W8, N, K)


def gemv_w8_workspace(N: int, K: int, device) -> Optional[torch.Tensor]:
    """The fp32 workspace for an [N, K] weight, or None when none is needed."""
    return _workspace(_W8, N, K, device)


def gemv_w8_supported(x: torch.Tensor, codes: torch.Tensor) -> bool:
    """Whether ``gemv_w8`` runs the HIP kernel on these: a bf16 GPU ``x`` on the HIP backend, M <= ``max_m()`` and
    K a multiple of 128."""
    return _supported(_W8, x, codes)


def gemv_w8_torch(x: torch.Tensor, codes: torch.Tensor, exps: torch.Tensor) -> torch.Tensor:
    return x @ dequantize_weight(codes, exps, x.dtype).t()


def gemv_w8_launch(x, codes, exps, out: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``nd_gemv_w8`` on raw tensors; every shape, dtype, stride and alignment the kernel relies on is checked here,
    before the launch."""
    return _launch(_W8, x, codes, exps, out, workspace)


def gemv_w8(x: torch.Tensor, codes: torch.Tensor, exps: torch.Tensor, out: Optional[torch.Tensor] = None,
            workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x`` [M, K] times the fp8 weight (codes [N, K], exps [N, K / 128]) transposed -> [M, N] in ``x.dtype``.
    ``workspace``: ``gemv_w8_workspace(N, K, device)``, allocated here when None (pass it under graph capture)."""
    if _ext.use_hip(x):
        return gemv_w8_launch(x, codes, exps, out, workspace)
    return _into(gemv_w8_torch(x, codes, exps), out)


def gemv_w4_workspace_numel(N: int, K: int) -> int:
    """fp32 elements of workspace ``nd_gemv_w4`` needs for an [N, K] weight (0: its partition has one K slice)."""
    return _workspace_numel(_W4, N, K)


def gemv_w4_workspace(N: int, K: int, device) -> Optional[torch.Tensor]:
    """The fp32 workspace for an [N, K] weight, or None when none is needed."""
    return _workspace(_W4, N, K, device)


def gemv_w4_supported(x: torch.Tensor, codes: torch.Tensor) -> bool:
    """Whether ``gemv_w4`` runs the HIP kernel on these: a bf16 GPU ``x`` on the HIP backend, M <= ``max_m()`` and
    K (twice the code bytes of a row) a multiple of 128."""
    return _supported(_W4, x, codes)


def gemv_w4_torch(x: torch.Tensor, codes: torch.Tensor, exps: torch.Tensor) -> torch.Tensor:
    return x @ dequantize_weight_fp4(codes, exps, x.dtype).t()


def gemv_w4_launch(x, codes, exps, out: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``nd_gemv_w4`` on raw tensors, checked as ``gemv_w8_launch`` checks its own."""
    return _launch(_W4, x, codes, exps, out, workspace)


def gemv_w4(x: torch.Tensor, codes: torch.Tensor, exps: torch.Tensor, out: Optional[torch.Tensor] = None,
            workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x`` [M, K] times the fp4 weight (codes [N, K / 2], exps [N, K / 32]) transposed -> [M, N] in ``x.dtype``.
    ``workspace``: ``gemv_w4_workspace(N, K, device)``, allocated here when None (pass it under graph capture)."""
    if _ext.use_hip(x):
        return gemv_w4_launch(x, codes, exps, out, workspace)
    return _into(gemv_w4_torch(x, codes, exps), out)
