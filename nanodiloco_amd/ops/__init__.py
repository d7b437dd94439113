"""Hot-path ops.  Each op dispatches to a hand-written HIP/CDNA4 kernel for GPU tensors and to the
PyTorch reference (``ops.reference``) for CPU tensors; see ``ops/_ext.py`` for the policy."""
from ._ext import available as hip_available, set_backend, get_backend, ExtensionMissing
from .linear import linear, wgrad_accumulate, set_wgrad_overlap, wgrad_overlap_enabled, join_wgrad, \
    set_dgrad_transposed, dgrad_transposed_enabled, transpose_into, mm_nt, set_proj_gemm, proj_gemm, \
    set_fused_epilogues, fused_epilogues, linear_rope, linear_rope_supported, mlp_fused, mlp_fused_supported, \
    set_wgrad_group, wgrad_group_enabled
from .norm import rmsnorm, rmsnorm_res, add_rmsnorm
from .qk_norm import qk_norm, qk_norm_rope
from .embedding import embedding
from .swiglu import swiglu
from .attention import attention, rope_cache, set_attn_fused_stats, key_start, check_padding, doc_bounds, \
    check_doc_bounds
from .decode import KVCache, attention_decode, cache_fill, decode_split
from .cross_entropy import lm_head_ce, lm_head_ce_parts, lm_head_loss, logit_softcap, LMHeadLoss, IGNORE_INDEX
from .optim import adamw_step, global_grad_norm, pseudograd, outer_nesterov, frag_pseudograd, frag_outer_mix, \
    SpanTable
from .muon import ns_gram, ns_poly, ns_update, ns_iterate, newton_schulz, muon_step, adamw_step_spans, \
    MuonPlan, AdamWSpans
from .qcomm import pseudograd_q, qreduce, outer_nesterov_q, pseudograd_q_ef, qreduce_ef
from .sparse_comm import pseudograd_topk, outer_nesterov_topk, topk_slot_bytes, densify
from .lowrank_comm import LowRankPlan, lowrank_project, lowrank_orthonormalize, lowrank_backproject, \
    outer_nesterov_lowrank, lowrank_wire_elems
from .determinism import set_deterministic, deterministic
from . import reference

__all__ = ["hip_available", "set_backend", "get_backend", "ExtensionMissing", "linear", "wgrad_accumulate",
           "set_wgrad_overlap", "wgrad_overlap_enabled", "join_wgrad", "set_wgrad_group", "wgrad_group_enabled",
           "set_dgrad_transposed", "dgrad_transposed_enabled", "transpose_into",
           "rmsnorm", "rmsnorm_res", "add_rmsnorm", "qk_norm", "qk_norm_rope", "set_attn_fused_stats", "embedding", "swiglu", "attention", "rope_cache", "doc_bounds", "check_doc_bounds",
           "KVCache", "attention_decode", "cache_fill", "decode_split",
           "lm_head_ce", "lm_head_ce_parts", "LMHeadLoss", "lm_head_loss", "logit_softcap",
           "IGNORE_INDEX", "adamw_step", "global_grad_norm", "pseudograd", "outer_nesterov", "pseudograd_q", "qreduce",
           "outer_nesterov_q", "pseudograd_q_ef", "qreduce_ef", "pseudograd_topk", "outer_nesterov_topk",
           "topk_slot_bytes", "densify", "LowRankPlan", "lowrank_project", "lowrank_orthonormalize",
           "lowrank_backproject", "outer_nesterov_lowrank", "lowrank_wire_elems", "frag_pseudograd", "frag_outer_mix", "SpanTable", "reference",
           "ns_gram", "ns_poly", "ns_update", "ns_iterate", "newton_schulz", "muon_step", "adamw_step_spans", "MuonPlan", "AdamWSpans"]
