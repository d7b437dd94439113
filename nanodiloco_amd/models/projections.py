"""The decoder's projections behind one interface (docs/DESIGN.md, "The projection seam"): which GEMM runs q|k|v,
o, the MLP and the lm head.  ``Bf16Projections`` runs them in the compute dtype (bf16 on the GPU, fp32 on the CPU)
and owns the W^T copies of the input-gradient GEMMs; ``Fp8Projections`` wraps the model's ``Fp8Linears`` and hands
the kinds that ``fp8.fp8_projection`` keeps in bf16 to the ``Bf16Projections`` it holds (``.bf16``), which the model
uses directly for evaluation and generation.  Both read weights, gradient views and ``training`` from the model
that owns them, held weakly (``self.m()``): no reference cycle keeps the W^T and fp8 copies of a dropped model.
"""
import warnings
import weakref

import torch

from ..ops import fp8
from ..ops.cross_entropy import LM_KEY, lm_head_ce_parts
from ..ops.linear import (dgrad_transposed_enabled, linear, linear_rope, linear_rope_supported, mlp_fused,
                          mlp_fused_supported, transpose_into)
from ..ops.swiglu import swiglu


class Bf16Projections:
    lm_y8 = None  # fp8 only: the final norm's fused e4m3 copy of y, while it waits for the lm head
    bf16 = property(lambda self: self)  # what the model runs evaluation and generation on

    def __init__(self, model):
        self.m = weakref.ref(model)
        # W^T copies for the input-gradient GEMMs (ops/linear.py), refreshed lazily whenever the
        # store's weight version moves: key -> [W^T buffer, version it holds, W view]
        self.wt_cache = {}

    def qkv_w(self, i):
        m, c = self.m(), self.m().config
        return (m._fused(m._qkv_names[i], "shadow"), m._fused(m._qkv_names[i], "grad"), c.head_dim,
                (c.num_attention_heads + c.num_key_value_heads) * c.head_dim)

    def o_w(self, i):
        name = f"model.layers.{i}.self_attn.o_proj.weight"
        return self.m()._w(name), self.m()._g(name)

    def mlp_w(self, i):
        m, down = self.m(), f"model.layers.{i}.mlp.down_proj.weight"
        return m._fused(m._gu_names[i], "shadow"), m._fused(m._gu_names[i], "grad"), m._w(down), m._g(down)

    def lm_w(self):
        return self.m()._w(self.m()._lm_name()), self.m()._g(self.m()._lm_name())

    def _wt(self, key, w):
        """W^T (contiguous) for the dgrad GEMM, or None when the plain layout is used."""
        if not (self.m().training and w.is_cuda and w.dtype == torch.bfloat16 and dgrad_transposed_enabled()):
            return None
        e = self.wt_cache.get(key)
        if e is None:
            e = [torch.empty(w.shape[1], w.shape[0], dtype=w.dtype, device=w.device), -1, w]
            self.wt_cache[key] = e
        return self._fresh(e)

    def _fresh(self, e):
        if e[1] != self.m().store.version:
            transpose_into(e[0], e[2])
            e[1] = self.m().store.version
        return e[0]

    def refresh_transposed(self):
        """Bring every cached W^T up to the current weights (eagerly, e.g. before a HIP-graph
        replay, whose captured GEMMs read these buffers but never re-run the version check)."""
        for e in self.wt_cache.values() if dgrad_transposed_enabled() else ():
            self._fresh(e)

    def x_target(self, key):  # fused-quantisation target for ``key``'s input / for the gradient of its output
        return None

    dy_target = x_target

    def qkv(self, i, y, y8, cos, sin, T):  # -> (projection, whether RoPE ran in the GEMM epilogue)
        w, gw, hd, rope_cols = self.qkv_w(i)
        wt = self._wt(f"{i}.qkv", w)
        # QK-norm sits between the projection and RoPE: the plain GEMM, and ops.qk_norm_rope rotates
        if not self.m().config.qk_norm and linear_rope_supported(y, w, wt, hd, rope_cols):
            # own GEMM with RoPE on q|k in its epilogue: the attention skips its rotation pass
            return linear_rope(y, w, gw, wt, cos, sin, T, hd, rope_cols), True
        return linear(y, w, gw, wt), False

    def o(self, i, x):
        w, gw = self.o_w(i)
        return linear(x, w, gw, self._wt(f"{i}.o", w))

    def mlp_args(self, i):  # what ``mlp_fused`` takes after y
        w_gu, gw_gu, w_dn, gw_dn = self.mlp_w(i)
        return w_gu, gw_gu, self._wt(f"{i}.gu", w_gu), w_dn, gw_dn, self._wt(f"{i}.down", w_dn)

    def mlp_fuses(self, i, y) -> bool:
        w_gu, _, wt_gu, w_dn, _, wt_dn = self.mlp_args(i)
        return mlp_fused_supported(y, w_gu, wt_gu, w_dn, wt_dn)

    def mlp(self, i, y, q_gu=None):
        w_gu, gw_gu, wt_gu, w_dn, gw_dn, wt_dn = self.mlp_args(i)
        if mlp_fused_supported(y, w_gu, wt_gu, w_dn, wt_dn):
            # own GEMMs with SwiGLU in the gate|up epilogue and its backward in the down dgrad's
            return mlp_fused(y, w_gu, gw_gu, wt_gu, w_dn, gw_dn, wt_dn)
        return linear(swiglu(linear(y, w_gu, gw_gu, wt_gu)), w_dn, gw_dn, wt_dn)

    def lm_head_ce(self, y, targets, loss_scale, z_loss=0.0, softcap=0.0):  # -> ops.LMHeadLoss (objective, CE, z part)
        w, gw = self.lm_w()
        return lm_head_ce_parts(y, w, gw, targets, loss_scale, wt=self._wt("lm_head", w), z_loss=z_loss,
                                softcap=softcap)


class Fp8Projections:
    """``lin`` (``model.fp8``) keeps the fp8 state: recipe, slot pairs, weight caches.  Slots are created in call
    order, so the order of the ``lin`` calls below is part of the fp8 checkpoint format."""

    _warned = set()

    def __init__(self, model, wgrad_fp8: bool):
        self.bf16 = Bf16Projections(model)
        self.m = self.bf16.m
        self.lin = fp8.Fp8Linears(model.device, wgrad_fp8=wgrad_fp8)
        self._lm_q = None  # the final norm's target, from x_target(LM_KEY) until the lm head has taken its copy of y

    @property
    def lm_y8(self):
        return self._lm_q.out if self._lm_q is not None else None

    def refresh_transposed(self):
        self.bf16.refresh_transposed()

    def _warn_once(self, key: str, msg: str) -> None:
        if key not in self._warned:
            self._warned.add(key)
            warnings.warn(msg, RuntimeWarning, stacklevel=4)

    def _quantises(self, key: str) -> bool:  # fused quantisation and the fp8 lm head: training forwards only
        return fp8.fp8_projection(key.split(".")[1]) and self.m().training and torch.is_grad_enabled()

    def x_target(self, key):
        q = self.lin.target(key) if self._quantises(key) else None
        if key == LM_KEY:
            self._lm_q = q
        return q

    def dy_target(self, key):
        return self.lin.target(key, grad=True) if self._quantises(key) else None

    def qkv(self, i, y, y8, cos, sin, T):
        if not fp8.fp8_projection("qkv"):
            out = self.bf16.qkv(i, y, y8, cos, sin, T)
            if not out[1] and not self.m().config.qk_norm:  # with QK-norm the plain GEMM is the intended one
                self._warn_once("qkv", "--fp8-keep-fused rope: the fused bf16 q|k|v + RoPE GEMM cannot run on this "
                                       "shape; the projection runs as a plain bf16 GEMM + separate RoPE pass (slower "
                                       "than fp8)")
            return out
        w, gw, hd, rope_cols = self.bf16.qkv_w(i)
        if not self.m().config.qk_norm and self.lin.rope_ok(y, w, hd, rope_cols):
            # e4m3 operands on the own fp8 GEMM, RoPE on the dequantised accumulator
            return self.lin(f"{i}.qkv", y, w, gw, self.m().store.version, y8, (cos, sin, T, hd, rope_cols)), True
        return self.lin(f"{i}.qkv", y, w, gw, self.m().store.version, y8), False

    def o(self, i, x):
        w, gw = self.bf16.o_w(i)
        return self.lin(f"{i}.o", x, w, gw, self.m().store.version) if fp8.fp8_projection("o") else self.bf16.o(i, x)

    def mlp(self, i, y, q_gu=None):
        if not fp8.fp8_projection("gu"):
            if not self.bf16.mlp_fuses(i, y):
                self._warn_once("mlp", "--fp8-keep-fused mlp: the fused bf16 SwiGLU GEMMs cannot run on this shape; "
                                       "the MLP runs as plain bf16 GEMMs + separate SwiGLU passes (slower than fp8)")
            return self.bf16.mlp(i, y)
        kgu, kdn, version = f"{i}.gu", f"{i}.down", self.m().store.version
        w_gu, gw_gu, w_dn, gw_dn = self.bf16.mlp_w(i)
        y8 = q_gu.out if q_gu is not None else None
        if self.lin.mlp_ok(y, w_gu, w_dn):
            # SwiGLU and its backward in the epilogues of the own fp8 GEMMs
            return self.lin.mlp(kgu, kdn, y, w_gu, w_dn, gw_gu, gw_dn, version, y8)
        q_down = self.x_target(kdn)
        gu = self.lin(kgu, y, w_gu, gw_gu, version, y8)
        act = swiglu(gu, q8=q_down, q8_bwd=self.dy_target(kgu))
        return self.lin(kdn, act, w_dn, gw_dn, version, q_down.out if q_down is not None else None)

    def lm_head_ce(self, y, targets, loss_scale, z_loss=0.0, softcap=0.0):
        y8, self._lm_q = self.lm_y8, None
        if not self._quantises(LM_KEY):
            return self.bf16.lm_head_ce(y, targets, loss_scale, z_loss, softcap)
        w, gw = self.bf16.lm_w()
        return lm_head_ce_parts(y, w, gw, targets, loss_scale, f8=self.lin, version=self.m().store.version, y8=y8,
                                z_loss=z_loss, softcap=softcap)
