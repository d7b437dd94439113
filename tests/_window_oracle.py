"""A sliding window as the existing float64 oracles understand it: a per-query lower bound.

``_oracle64.attention`` / ``_model_oracle.logits64`` take ``doc_start[b, t]``, the first key query t of sequence b may
see; ``_decode_oracle.decode_refs`` takes ``kstart[b]`` for the single query at ``pos[b]``.  A window of W keys that
counts the query itself, composed with a left-padding key start, is ``max(kstart[b], t - W + 1)``: nothing in the
oracles changes.  A pad query (t < kstart[b]) gets a bound above itself and so sees no key, as under ``kstart`` alone.
"""
import torch


def window_doc_start(B, T, window, device, kstart=None):
    """int32 [B, T]: ``max(kstart[b], t - window + 1, 0)``."""
    t = torch.arange(T, device=device, dtype=torch.int64)
    lo = (t - int(window) + 1).clamp(min=0).expand(B, T).clone()
    if kstart is not None:
        lo = torch.maximum(lo, kstart.to(device).long().view(B, 1))
    return lo.to(torch.int32).contiguous()


def kstart_eff(pos, window, kstart=None):
    """int32 [B]: the decode step's lower bound ``max(kstart[b], pos[b] - window + 1, 0)``."""
    lo = (pos.long() - int(window) + 1).clamp(min=0)
    if kstart is not None:
        lo = torch.maximum(lo, kstart.long().clamp(min=0))
    return lo.to(torch.int32).contiguous()


def dense_window_mask(B, T, window, device, kstart=None):
    """Boolean [B, T, T] written as two loops' worth of comparisons (row = query, column = key): the definition the
    helpers above and ``reference.window_causal_mask`` are checked against."""
    q = torch.arange(T, device=device).view(1, T, 1)
    k = torch.arange(T, device=device).view(1, 1, T)
    ok = (k <= q) & (k > q - int(window))
    ok = ok.expand(B, T, T).clone()
    if kstart is not None:
        ok &= k >= kstart.to(device).long().view(B, 1, 1)
    return ok
