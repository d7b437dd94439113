"""fp8 weight-only projection for skinny M: ``out = x . dequant(codes, exps)^T`` (docs/DESIGN.md "fp8 weight-only
decode").

The weight format is the KV cache's (``ops.decode.kv8_quantize``): ``W`` [N, K] in groups of 128 along K, e4m3 codes
uint8 [N, K] plus one int8 exponent per group [N, K / 128], value = code * 2^e.  ``quantize_weight`` /
``dequantize_weight`` are that definition on a 2-D weight.

``gemv_w8(x, codes, exps)``: ``x`` [M, K] bf16 -> [M, N] bf16 with fp32 accumulation.  HIP path
(``csrc/gemv_w8.hip``, ``nd_gemv_w8``): M <= ``max_m()`` rows on MFMA, the codes streamed once; a row's bits depend on
that row, the weight, N and K alone.  Static shapes, no host sync, the workspace is the caller's: capturable in a HIP
graph.  On the CPU, or under ``--ops torch``, the PyTorch twin runs.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _ext
from .decode import kv8_dequantize, kv8_quantize

GROUP = 128  # codes per exponent


def max_m() -> int:
    """Rows of ``x`` ``nd_gemv_w8`` takes (compile-time ``MAX_M``)."""
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


def gemv_w8_workspace_numel(N: int, K: int) -> int:
    """fp32 elements of workspace ``nd_gemv_w8`` needs for an [N, K] weight (0: its partition has one K slice)."""
    splits = int(_ext.lib().nd_gemv_w8_splits(int(N), int(K)))
    if splits < 1:
        raise ValueError(f"gemv_w8: bad weight shape [{N}, {K}]")
    return splits * max_m() * int(N) if splits > 1 else 0


def gemv_w8_workspace(N: int, K: int, device) -> Optional[torch.Tensor]:
    """The fp32 workspace for an [N, K] weight, or None when none is needed."""
    n = gemv_w8_workspace_numel(N, K)
    return torch.empty(n, dtype=torch.float32, device=device) if n else None


def gemv_w8_supported(x: torch.Tensor, codes: torch.Tensor) -> bool:
    """Whether ``gemv_w8`` runs the HIP kernel on these: a bf16 GPU ``x`` on the HIP backend, M <= ``max_m()`` and
    K a multiple of 128."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and codes.dim() == 2 and _ext.use_hip(x)
            and 1 <= x.shape[0] <= max_m() and x.shape[1] == codes.shape[1] and codes.shape[1] % GROUP == 0)


def gemv_w8_torch(x: torch.Tensor, codes: torch.Tensor, exps: torch.Tensor) -> torch.Tensor:
    return x @ dequantize_weight(codes, exps, x.dtype).t()


def gemv_w8_launch(x, codes, exps, out: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``nd_gemv_w8`` on raw tensors; every shape, dtype, stride and alignment the kernel relies on is checked here,
    before the launch."""
    if codes.dim() != 2 or codes.dtype != torch.uint8 or not codes.is_cuda or not codes.is_contiguous():
        raise ValueError("gemv_w8: codes must be a contiguous uint8 [N, K] GPU tensor")
    N, K = codes.shape
    if N < 1 or K < GROUP or K % GROUP:
        raise ValueError(f"gemv_w8: K = {K} must be a positive multiple of {GROUP} and N = {N} >= 1")
    if exps.dtype != torch.int8 or not exps.is_cuda or not exps.is_contiguous() or tuple(exps.shape) != (N, K // GROUP):
        raise ValueError(f"gemv_w8: exps must be a contiguous int8 [{N}, {K // GROUP}] GPU tensor")
    if x.dim() != 2 or x.dtype != torch.bfloat16 or not x.is_cuda or x.shape[1] != K:
        raise ValueError(f"gemv_w8: x must be a bf16 [M, {K}] GPU tensor")
    M = x.shape[0]
    if not 1 <= M <= max_m():
        raise ValueError(f"gemv_w8: M = {M} outside [1, {max_m()}]")
    if x.stride(1) != 1 or (M > 1 and (x.stride(0) < K or x.stride(0) % 8)):
        raise ValueError("gemv_w8: x rows must be contiguous with a stride that is a multiple of 8")
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    elif out.dtype != torch.bfloat16 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (M, N):
        raise ValueError(f"gemv_w8: out must be a contiguous bf16 [{M}, {N}] GPU tensor")
    splits = int(_ext.lib().nd_gemv_w8_splits(N, K))
    if splits > 1:
        if workspace is None:
            workspace = gemv_w8_workspace(N, K, x.device)
        elif workspace.dtype != torch.float32 or not workspace.is_cuda or not workspace.is_contiguous() \
                or workspace.numel() < splits * max_m() * N:
            raise ValueError(f"gemv_w8: workspace must be a contiguous fp32 GPU tensor of {splits * max_m() * N}")
    else:
        workspace = None
    for name, t in (("x", x), ("codes", codes), ("workspace", workspace)):
        if t is not None and t.data_ptr() % 16:
            raise ValueError(f"gemv_w8: {name} must be 16-byte aligned")
    _ext.check(_ext.lib().nd_gemv_w8(_ext.ptr(x), _ext.ptr(codes), _ext.ptr(exps), _ext.ptr(out), _ext.ptr(workspace),
                                     M, N, K, x.stride(0) if M > 1 else K, _ext.stream_ptr(x.device)), "nd_gemv_w8")
    return out


def gemv_w8(x: torch.Tensor, codes: torch.Tensor, exps: torch.Tensor, out: Optional[torch.Tensor] = None,
            workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x`` [M, K] times the fp8 weight (codes [N, K], exps [N, K / 128]) transposed -> [M, N] in ``x.dtype``.
    ``workspace``: ``gemv_w8_workspace(N, K, device)``, allocated here when None (pass it under graph capture)."""
    if _ext.use_hip(x):
        return gemv_w8_launch(x, codes, exps, out, workspace)
    y = gemv_w8_torch(x, codes, exps)
    if out is not None:
        out.copy_(y)
        return out
    return y
