"""Llama causal LM over a flat :class:`ParamStore`.

Architecture and parameter names/shapes are exactly HF ``LlamaForCausalLM``
(HF/models/llama/modeling_llama.py:52-492), so checkpoints load into HF and HF
weights load here.  The compute graph is our own:

  h0  = embed(ids)                          fp32 residual stream, gathered from the fp32 master
  y   = rmsnorm(h0) * w_in[0]               compute dtype (bf16)
  per layer:
    qkv = rope(y @ [Wq|Wk|Wv]^T)            ONE GEMM (fused view of the flat buffer), RoPE in its epilogue
                                            (config.qk_norm: the plain GEMM, then a per-head RMSNorm of q and k fused
                                            with RoPE in one pass over q|k, ops.qk_norm_rope)
    o   = flash_attn(qkv)                   HIP kernel, reads packed qkv, writes [N, nh*hd]
    y,h = add_rmsnorm(h, o @ Wo^T, w_post)  residual add fused into the norm
    act = swiglu(y @ [Wgate|Wup]^T)         ONE GEMM, SwiGLU in its epilogue (SwiGLU backward in the
    y,h = add_rmsnorm(h, act @ Wdown^T, ..) down projection's dgrad epilogue)
  loss = lm_head_ce(y, W_lm, targets)       fused chunked GEMM + CE (+ its backward); config.final_logit_softcapping
                                            = C: on C * tanh(logits / C), as every logit the model hands out

Weight gradients are written straight into ``store.grad`` by the ops' backward (and, for the
lm head, during the forward).  ``layer_hook(i)`` is called from the backward as soon as every
gradient in layer i's span is final (used for the inner-DDP bucketed all-reduce overlapped with
backward; see ``_GradHook`` for why the hook sits on the next norm's input).
"""
from __future__ import annotations

import contextlib
import dataclasses
import functools
from typing import Callable, List, Optional

import torch

from .. import ops
from ..config import LlamaConfig
from ..ops.cross_entropy import LM_KEY
from .param_store import ParamStore
from .projections import Bf16Projections, Fp8Projections

_CONFIG = object()  # generate(): "take it from the model config"


@dataclasses.dataclass
class CausalLMOutput:
    loss: Optional[torch.Tensor] = None  # the objective: cross-entropy, plus the z term when model.z_loss > 0
    logits: Optional[torch.Tensor] = None
    ce_loss: Optional[torch.Tensor] = None  # the cross-entropy part, detached (z_loss 0: ``loss``, detached)
    z_loss: Optional[torch.Tensor] = None   # the weighted z term, detached; None when model.z_loss is 0


class _GradHook(torch.autograd.Function):
    """Identity; calls ``fn(idx)`` when the gradient w.r.t. its input has been produced.

    Placement matters: autograd runs a node only after every consumer of its output has produced
    its gradient, so a hook on the INPUT of the add+RMSNorm that feeds layer i fires after the whole
    backward of layer i (GEMMs, attention, SwiGLU, both norms) -- i.e. when layer i's span of the
    flat grad buffer is final.  (A hook on a layer's OUTPUT would fire before that layer's own
    backward has run.)"""

    @staticmethod
    def forward(ctx, x, fn, idx):
        ctx.fn, ctx.idx = fn, idx
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ops.join_wgrad()  # the layer's weight gradients may still be in flight on the side stream
        ctx.fn(ctx.idx)
        return g, None, None


class LlamaForCausalLM:
    def __init__(self, config: LlamaConfig, device="cpu", compute_dtype: torch.dtype = torch.float32,
                 store: Optional[ParamStore] = None, activation_checkpointing: bool = False, fp8: bool = False,
                 fp8_wgrad: bool = False, residual_dtype: Optional[torch.dtype] = None, doc_mask: bool = False):
        self.config = config
        # packed windows: attention stays inside each EOS-separated document (ops.doc_bounds)
        self.doc_mask = bool(doc_mask)
        if self.doc_mask and config.sliding_window:
            raise ValueError("doc_mask (packed documents) and a sliding window cannot be combined")
        self.debug_checks = False  # validate the derived bounds every forward (host sync: never under graph capture)
        # z-loss coefficient of the training objective (--z-loss; ops/cross_entropy.py): 0.0 = off.  A hyperparameter,
        # not state; evaluation (loss_stats) ignores it
        self.z_loss = 0.0
        # final-logit soft cap C (config.final_logit_softcapping; 0.0 = off): a property of the model, so it acts
        # wherever a logit is produced -- training loss, loss_stats, forward().logits, prefill and decode_step
        self.softcap = float(config.final_logit_softcapping or 0.0)
        self.device = torch.device(device)
        self.compute_dtype = compute_dtype
        # residual stream: fp32 (default, the autocast recipe) or bf16 (Megatron's default; ops/norm.py)
        self.residual_dtype = residual_dtype or torch.float32
        if self.residual_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("residual_dtype must be float32 or bfloat16")
        self.activation_checkpointing = activation_checkpointing
        L = config.num_hidden_layers
        groups = []
        for i in range(L):
            p = f"model.layers.{i}."
            groups.append([p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight"])
            groups.append([p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"])
        self.store = store or ParamStore(config.param_shapes(), device, compute_dtype, fuse_groups=groups)
        self._qkv_names = [g for g in groups[0::2]]
        self._gu_names = [g for g in groups[1::2]]
        self.layer_hook: Optional[Callable[[int], None]] = None
        self.training = True
        if fp8 and (compute_dtype != torch.bfloat16 or self.device.type != "cuda"):
            raise ValueError("fp8 needs bf16 compute on an MI355X")
        self.proj = Fp8Projections(self, fp8_wgrad) if fp8 else Bf16Projections(self)
        self.fp8 = self.proj.lin if fp8 else None  # the fp8 state (Fp8Linears) behind self.proj

    # ------------------------------------------------------------------ init / io
    @torch.no_grad()
    def init_weights(self, seed: int = 1337):
        """HF ``_init_weights``: N(0, initializer_range) for Linear/Embedding, ones for RMSNorm."""
        std = self.config.initializer_range
        gen_dev = self.device if self.device.type == "cuda" else torch.device("cpu")
        g = torch.Generator(device=gen_dev)
        g.manual_seed(seed)
        for name in self.store.names:
            v = self.store.master_view(name)
            if v.dim() == 1:
                v.fill_(1.0)
            else:
                t = torch.empty(v.shape, dtype=torch.float32, device=gen_dev)
                t.normal_(0.0, std, generator=g)
                v.copy_(t)
        pad = self.config.pad_token_id
        if pad is not None:
            self.store.master_view("model.embed_tokens.weight")[pad].zero_()
        self.store.sync_shadow()
        return self

    def state_dict(self):
        return self.store.state_dict("master")

    def load_state_dict(self, sd, strict=True):
        self.store.load_state_dict(sd, strict=strict)

    def num_parameters(self) -> int:
        return self.store.num_params

    def train(self):
        self.training = True
        return self

    def eval(self):
        self.training = False
        return self

    def __call__(self, *a, **kw):
        return self.forward(*a, **kw)

    # ------------------------------------------------------------------ views
    def _w(self, name):  # compute-dtype weight (GEMM operand)
        return self.store.shadow_view(name)

    def _m(self, name):  # fp32 master weight (norms, embedding gather)
        return self.store.master_view(name)

    def _g(self, name):
        return self.store.grad_view(name) if self.training else None

    def _fused(self, names, which):
        if which == "grad" and not self.training:
            return None
        return self.store.fused_view(which, names)

    # ------------------------------------------------------------------ forward
    def refresh_transposed(self):  # bring every cached W^T up to the current weights
        self.proj.refresh_transposed()

    def _layer(self, i, h, y, cos, sin, B, T, next_norm, y8=None, kstart=None, doc=None, cache=None):
        c, proj = self.config, self.proj
        p = f"model.layers.{i}."
        qkv, rotated = proj.qkv(i, y, y8, cos, sin, T)  # rotated: RoPE ran in the GEMM epilogue
        if c.qk_norm:
            # the plain projection (never the RoPE epilogue), then norm + RoPE in one pass over q|k (HIP) or the norm
            # alone (PyTorch path); the attention backward hands back the gradient of the normed, un-rotated q|k
            qkv, rotated = ops.qk_norm_rope(qkv, self._m(p + "self_attn.q_norm.weight"),
                                            self._m(p + "self_attn.k_norm.weight"),
                                            self._g(p + "self_attn.q_norm.weight"),
                                            self._g(p + "self_attn.k_norm.weight"), cos, sin, T,
                                            c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.rms_norm_eps,
                                            inplace=True)
        o = ops.attention(qkv, cos, sin, B, T, c.num_attention_heads, c.num_key_value_heads, c.head_dim,
                          inplace=True, kstart=kstart, rotated=rotated, doc_bounds=doc, window=c.sliding_window)
        if cache is not None:
            # prefill: the HIP path has rotated q|k inside qkv by now (in place, or in the GEMM epilogue); the
            # PyTorch path leaves its input alone and cache_fill rotates k itself
            ops.cache_fill(cache, i, qkv, B, T, cos, sin, rotated=rotated or ops._ext.use_hip(qkv))
        a = proj.o(i, o)
        q_gu = proj.x_target(f"{i}.gu")
        y, h = ops.add_rmsnorm(h, a, self._m(p + "post_attention_layernorm.weight"),
                               self._g(p + "post_attention_layernorm.weight"), c.rms_norm_eps, self.compute_dtype,
                               q8=q_gu, q8_bwd=proj.dy_target(f"{i}.o"))
        return proj.mlp(i, y, q_gu), h

    def hidden_states(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                      cache=None) -> torch.Tensor:
        """Final-normed hidden states [B*T, d] in the compute dtype.  ``attention_mask`` (HF [B, T],
        left or right padded) becomes a per-sequence key start for the attention kernels.  With ``doc_mask`` the
        document bounds of the packed window are derived from ``input_ids`` once and shared by every layer.
        ``cache`` (an ``ops.KVCache``, prefill only): every layer's rotated k and v go into slots 0 .. T-1."""
        c = self.config
        if self.doc_mask and attention_mask is not None:
            raise ValueError("doc_mask (packed documents) and attention_mask (padded batches) cannot be combined")
        kstart = ops.key_start(attention_mask) if attention_mask is not None else None
        doc = ops.doc_bounds(input_ids, c.eos_token_id) if self.doc_mask else None
        if doc is not None and self.debug_checks:
            ops.check_doc_bounds(*doc)
        B, T = input_ids.shape
        cdt = self.compute_dtype
        eps = c.rms_norm_eps
        cos, sin = ops.rope_cache(T, c.head_dim, c.rope_theta, c.rope_scaling, self.device)
        h = ops.embedding(input_ids, self._m("model.embed_tokens.weight"), self._g("model.embed_tokens.weight"),
                          out_dtype=self.residual_dtype)
        hook = self.layer_hook if (self.layer_hook is not None and self.training and torch.is_grad_enabled()) else None
        if hook is not None:
            # layer 0's last gradient (its input_layernorm weight) is written by the backward of the
            # norm below; the hook node on the norm's INPUT runs right after that backward
            h = _GradHook.apply(h, hook, 0)
        q = self.proj.x_target("0.qkv")
        # (y, h): the embedding output feeds both the first norm and the residual stream; rmsnorm_res
        # fuses the two gradient contributions inside the norm's backward kernel
        y, h = ops.rmsnorm_res(h, self._m("model.layers.0.input_layernorm.weight"),
                               self._g("model.layers.0.input_layernorm.weight"), eps, cdt, q8=q)
        y8 = q.out if q is not None else None
        L = c.num_hidden_layers
        for i in range(L):
            nxt = f"model.layers.{i + 1}.input_layernorm.weight" if i + 1 < L else "model.norm.weight"
            if self.activation_checkpointing and self.training and torch.is_grad_enabled():
                from torch.utils.checkpoint import checkpoint
                m, h = checkpoint(self._layer, i, h, y, cos, sin, B, T, nxt, None, kstart, doc, use_reentrant=False)
            else:
                m, h = self._layer(i, h, y, cos, sin, B, T, nxt, y8, kstart, doc, cache)
            if hook is not None and i + 1 < L:
                # layer i+1's gradients are final once the backward of the add+norm that produces its
                # input (and owns its input_layernorm weight) has run: hook that norm's input
                m = _GradHook.apply(m, hook, i + 1)
            q = self.proj.x_target(f"{i + 1}.qkv" if i + 1 < L else LM_KEY)
            y, h = ops.add_rmsnorm(h, m, self._m(nxt), self._g(nxt), eps, cdt, q8=q,
                                   q8_bwd=self.proj.dy_target(f"{i}.down"))
            y8 = q.out if q is not None else None
        return y

    def forward(self, input_ids: torch.Tensor, labels: Optional[torch.Tensor] = None, attention_mask=None,
                loss_scale: float = 1.0, return_logits: bool = False, targets: Optional[torch.Tensor] = None
                ) -> CausalLMOutput:
        """``labels`` follow HF semantics (shifted internally, -100 ignored).  ``attention_mask``
        follows HF too: pad keys are masked for every real token (left or right padding; pad positions
        should carry label -100, as the HF data path sets them)."""
        y = self.hidden_states(input_ids, attention_mask)
        out = CausalLMOutput()
        if labels is not None or targets is not None:
            if targets is None:
                targets = ops.reference.shift_labels(labels, ops.IGNORE_INDEX)
            out.loss, out.ce_loss, out.z_loss = self.proj.lm_head_ce(y, targets.reshape(-1), loss_scale, self.z_loss,
                                                                     self.softcap)
        if return_logits or (labels is None and targets is None):
            with torch.no_grad():
                B, T = input_ids.shape
                out.logits = self._capped(ops.mm_nt(y.detach(), self._w(self._lm_name())).float()).view(B, T, -1)
        return out

    @torch.no_grad()
    def loss_stats(self, input_ids: torch.Tensor, labels: torch.Tensor, attention_mask=None) -> torch.Tensor:
        """Evaluation of one batch: float64 ``[sum of row losses, valid tokens, top-1 hits]`` on the device (no
        host sync), so batches -- and ranks -- add up before anything is divided.  ``labels`` follow HF semantics
        as in ``forward`` (shifted internally, -100 ignored); ``doc_mask`` / ``attention_mask`` and the residual
        dtype act as they do there.

        The call leaves no trace: it runs under ``no_grad`` with the gradient views off (nothing is written to the
        flat grad buffer), takes the loss-only lm head (``ops.lm_head_loss``: one GEMM per chunk, the logits are
        only read) and restores ``training``.  With fp8 the evaluation forward runs the bf16 projections on the
        bf16 shadow weights: no activation is quantised, so neither the delayed-scaling state of ``Fp8Recipe``
        (amax partials, history, scales, first-use flags) nor the ``Fp8Weight`` caches are read or written, the
        next training step is bitwise what it would have been without the evaluation, and the number does not
        depend on the scaling history."""
        with self._inference():
            y = self.hidden_states(input_ids, attention_mask)
            targets = ops.reference.shift_labels(labels, ops.IGNORE_INDEX).reshape(-1)
            row_loss, row_hit = ops.lm_head_loss(y, self._w(self._lm_name()), targets, softcap=self.softcap)
        return torch.stack([row_loss.sum(dtype=torch.float64), (targets != ops.IGNORE_INDEX).sum().double(),
                            row_hit.sum().double()])

    # ------------------------------------------------------------------ generation
    def _lm_name(self) -> str:
        return "lm_head.weight" if not self.config.tie_word_embeddings else "model.embed_tokens.weight"

    def _capped(self, logits: torch.Tensor) -> torch.Tensor:
        """The fp32 logits of a projection as the model hands them out: soft-capped in place when the config says so
        (one HIP kernel on the HIP path, static shapes: capturable)."""
        return ops.logit_softcap(logits, self.softcap) if self.softcap else logits

    @contextlib.contextmanager
    def _inference(self):
        """Evaluation and generation: gradient views off, and for an fp8 model its held bf16 projections on the bf16
        shadow weights, so that nothing of the delayed-scaling state is read or written; everything restored on exit."""
        saved = (self.training, self.proj)
        self.training, self.proj = False, self.proj.bf16
        try:
            with torch.no_grad():
                yield
        finally:
            self.training, self.proj = saved

    def new_cache(self, batch: int, s_max: int):
        return ops.KVCache(self.config, batch, s_max, self.device, self.compute_dtype)

    def prefill(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], cache) -> torch.Tensor:
        """The existing forward on a (left-padded) prompt batch [B, T], every layer's k|v into ``cache`` slots
        0 .. T-1, ``pos = T``, ``kstart = ops.key_start(attention_mask)``.  Returns the last position's logits [B, V]
        (fp32).  Positions are slot indices, the training path's convention under left padding (scores depend on
        q - k only)."""
        B, T = input_ids.shape
        if self.doc_mask:
            raise ValueError("generation runs on single documents: build the model without doc_mask")
        if B != cache.batch or T > cache.s_max:
            raise ValueError(f"a [{B}, {T}] prompt does not fit a KV cache of batch {cache.batch}, "
                             f"s_max {cache.s_max}")
        with self._inference():
            y = self.hidden_states(input_ids, attention_mask, cache=cache)
            cache.pos.fill_(T)
            cache.max_pos = T
            if attention_mask is not None:
                cache.kstart.copy_(ops.key_start(attention_mask))
            else:
                cache.kstart.zero_()
            last = y.view(B, T, -1)[:, -1].contiguous()
            return self._capped(ops.mm_nt(last, self._w(self._lm_name())).float())

    def _decode_device(self, tokens: torch.Tensor, cache) -> torch.Tensor:
        """The device work of one decode step (static shapes, no host sync: HIP-graph capturable), ``pos += 1``
        included; the host-side bound of the cache is the caller's."""
        c = self.config
        cdt, eps = self.compute_dtype, c.rms_norm_eps
        B = tokens.shape[0]
        cos, sin = ops.rope_cache(cache.s_max, c.head_dim, c.rope_theta, c.rope_scaling, self.device)
        h = ops.embedding(tokens.view(B, 1), self._m("model.embed_tokens.weight"), None, out_dtype=self.residual_dtype)
        y, h = ops.rmsnorm_res(h, self._m("model.layers.0.input_layernorm.weight"), None, eps, cdt)
        L = c.num_hidden_layers
        for i in range(L):
            p = f"model.layers.{i}."
            qkv = ops.mm_nt(y, self._fused(self._qkv_names[i], "shadow"))
            if c.qk_norm:  # in place on the new row; the decode kernel rotates what it finds there
                ops.qk_norm(qkv, self._m(p + "self_attn.q_norm.weight"), self._m(p + "self_attn.k_norm.weight"),
                            c.num_attention_heads, c.num_key_value_heads, c.head_dim, eps)
            o = ops.attention_decode(qkv, cache, i, cos, sin)
            a = ops.mm_nt(o, self._w(p + "self_attn.o_proj.weight"))
            y, h = ops.add_rmsnorm(h, a, self._m(p + "post_attention_layernorm.weight"), None, eps, cdt)
            gu = ops.mm_nt(y, self._fused(self._gu_names[i], "shadow"))
            m = ops.mm_nt(ops.swiglu(gu), self._w(p + "mlp.down_proj.weight"))
            nxt = f"model.layers.{i + 1}.input_layernorm.weight" if i + 1 < L else "model.norm.weight"
            y, h = ops.add_rmsnorm(h, m, self._m(nxt), None, eps, cdt)
        logits = self._capped(ops.mm_nt(y, self._w(self._lm_name())).float())
        cache.pos += 1
        return logits

    def decode_step(self, tokens: torch.Tensor, cache) -> torch.Tensor:
        """One token per sequence (``tokens`` [B], at slot ``cache.pos``) -> next-token logits [B, V] (fp32)."""
        cache.check_room()
        with self._inference():
            logits = self._decode_device(tokens, cache)
        cache.advance(device_side=False)
        return logits

    def generate(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                 max_new_tokens: int = 32, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                 eos_token_id=_CONFIG, pad_token_id=_CONFIG, seed: int = 0, use_cache: bool = True,
                 hip_graph="auto", return_logits: bool = False):
        """Continue a (left-padded) prompt batch ``input_ids`` [B, T]; returns the token ids [B, T + n], n <=
        ``max_new_tokens`` (generation ends early once every row has produced ``eos_token_id``; a finished row is
        filled with ``pad_token_id``).  ``temperature`` 0 is greedy; otherwise ``filter_logits`` (top-k, top-p) and
        ``torch.multinomial`` with a generator seeded by ``seed``.  ``use_cache=False`` recomputes the whole prefix
        per token (the check and the timing baseline).  ``hip_graph``: True / False / "auto" (on for a GPU, non-fp8
        model on the HIP path): the decode step is captured once after two eager steps and replayed.
        ``return_logits``: also the fp32 logits [B, n, V] every token was drawn from."""
        c = self.config
        eos = c.eos_token_id if eos_token_id is _CONFIG else eos_token_id
        pad = pad_token_id
        if pad is _CONFIG or pad is None:
            pad = c.pad_token_id if c.pad_token_id is not None else (eos if eos is not None else 0)
        B, T = input_ids.shape
        n = int(max_new_tokens)
        if n < 1:
            raise ValueError("max_new_tokens must be at least 1")
        if temperature < 0 or not 0.0 < top_p <= 1.0 or top_k < 0:
            raise ValueError("need temperature >= 0, 0 < top_p <= 1, top_k >= 0")
        if attention_mask is not None:
            ops.check_padding(attention_mask)
            if not bool(attention_mask[:, -1].all()):
                raise ValueError("generation needs left-padded prompts (every row's last token real)")
        dev = input_ids.device
        gen = None
        if temperature > 0:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
        if hip_graph == "auto":
            hip_graph = use_cache and self.fp8 is None and ops._ext.get_backend() != "torch" and dev.type == "cuda"
        if hip_graph and (not use_cache or dev.type != "cuda"):
            raise ValueError("hip_graph needs use_cache=True on a GPU")
        if use_cache:
            cache = self.new_cache(B, T + n - 1)  # the last token drawn is never fed back
            logits = self.prefill(input_ids, attention_mask, cache)
            step = functools.partial(self.decode_step, cache=cache)
            if hip_graph:
                from ..utils.graphs import GraphedDecodeStep
                step = GraphedDecodeStep(self, cache)
        else:
            if T + n - 1 > c.max_position_embeddings:
                raise ValueError(f"{T} + {n} tokens exceed max_position_embeddings = {c.max_position_embeddings}")
            ids = input_ids
            mask = attention_mask
            with self._inference():
                logits = self.forward(ids, attention_mask=mask).logits[:, -1]
        out = torch.full((B, n), pad, dtype=input_ids.dtype, device=dev)
        finished = torch.zeros(B, dtype=torch.bool, device=dev)
        kept = [] if return_logits else None
        done = 0
        for i in range(n):
            if kept is not None:
                kept.append(logits.clone())  # a graphed step returns its static buffer
            tok = sample_logits(logits, temperature, top_k, top_p, gen).to(input_ids.dtype)
            if eos is not None:
                tok = torch.where(finished, torch.full_like(tok, pad), tok)
                finished = finished | (tok == eos)
            out[:, i] = tok
            done = i + 1
            if done == n or (eos is not None and done % 16 == 0 and bool(finished.all())):
                break
            if use_cache:
                logits = step(tok)
            else:
                ids = torch.cat([ids, tok[:, None]], dim=1)
                if mask is not None:
                    mask = torch.cat([mask, torch.ones_like(mask[:, :1])], dim=1)
                with self._inference():
                    logits = self.forward(ids, attention_mask=mask).logits[:, -1]
        if eos is not None:
            # as HF: the result ends with the step at which the last row finished
            hit = out[:, :done] == eos
            first = torch.where(hit.any(1), hit.int().argmax(1) + 1, torch.full_like(hit[:, 0].int(), done))
            done = int(first.max())
        res = torch.cat([input_ids, out[:, :done]], dim=1)
        if return_logits:
            return res, torch.stack(kept[:done], dim=1)
        return res


def filter_logits(logits: torch.Tensor, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """fp32 logits [B, V] with everything outside the top-k / nucleus set at -inf.  top-k keeps every logit >= the
    k-th largest; top-p (applied to what top-k left) keeps, in descending order, every token whose preceding
    probability mass is < ``top_p``.  Ties at either threshold are kept, so the result does not depend on the order
    a sort gives equal logits."""
    x = logits.float()
    V = x.shape[-1]
    if 0 < top_k < V:
        kth = x.topk(top_k, dim=-1).values[..., -1:]
        x = x.masked_fill(x < kth, float("-inf"))
    if top_p < 1.0:
        sl = x.sort(dim=-1, descending=True).values
        pr = torch.softmax(sl, dim=-1)
        before = pr.cumsum(-1) - pr
        thr = sl.masked_fill(before >= top_p, float("inf")).amin(-1, keepdim=True)
        x = x.masked_fill(x < thr, float("-inf"))
    return x


def sample_logits(logits: torch.Tensor, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                  generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """One token id per row of fp32 ``logits`` [B, V]: argmax at temperature 0, else a seeded multinomial draw."""
    if temperature == 0:
        return logits.argmax(-1)
    x = filter_logits(logits.float() / temperature, top_k, top_p)
    return torch.multinomial(torch.softmax(x, dim=-1), 1, generator=generator)[:, 0]
