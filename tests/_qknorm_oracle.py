"""float64 oracles of QK-norm: the norm, norm + RoPE, their backward, and the whole model with QK-norm.

Plain PyTorch in float64, written from the math in ``csrc/qk_norm.hip`` and docs/DESIGN.md ("QK-norm"); none of it
calls an op of the project.  The model oracle is ``_model_oracle.logits64`` with the two norms added between the
q / k projections and the rotation; it takes that module's input helpers (RoPE tables, key start, document starts,
the weights the model computes with) as they are.
"""
import torch

from . import _model_oracle as mo
from ._oracle64 import f32_scalar


def _heads(x, n, hd):
    return x.reshape(x.shape[0], n, hd)


def qk_norm(qkv, wq, wk, nh, nkv, hd, eps, dy=None):
    """Packed rows [N, (nh + 2 nkv) hd].  Per (token, head): rstd = 1 / sqrt(mean_d x^2 + eps), xhat = x rstd,
    y = w xhat with w = wq (q heads) / wk (k heads); v passes through.  With ``dy`` (the gradient of y, packed with
    the v gradient): g = w dy, dx = rstd (g - xhat mean_d(g xhat)), dwq[d] = sum over tokens and q heads of dy xhat
    (dwk likewise); the v gradient passes through.  Returns float64 ``y``, ``rstd`` [N, nh + nkv] and, with ``dy``,
    ``dx``, ``dwq``, ``dwk``."""
    x = qkv.double()
    N = x.shape[0]
    e = f32_scalar(eps)
    sizes = [nh * hd, nkv * hd, nkv * hd]
    q, k, v = x.split(sizes, dim=-1)
    out, ys, rs, xh = {}, [], [], []
    for t, n, w in ((q, nh, wq), (k, nkv, wk)):
        t = _heads(t, n, hd)
        r = 1.0 / torch.sqrt((t * t).mean(-1, keepdim=True) + e)
        xh.append(t * r)
        rs.append(r[..., 0])
        ys.append((w.double() * xh[-1]).reshape(N, n * hd))
    out["y"] = torch.cat(ys + [v], dim=-1)
    out["rstd"] = torch.cat(rs, dim=-1)
    if dy is not None:
        d = dy.double().split(sizes, dim=-1)
        dxs, dws = [], []
        for i, (n, w) in enumerate(((nh, wq), (nkv, wk))):
            di = _heads(d[i], n, hd)
            g = di * w.double()
            r = rs[i][..., None]
            dxs.append((r * (g - xh[i] * (g * xh[i]).mean(-1, keepdim=True))).reshape(N, n * hd))
            dws.append((di * xh[i]).sum((0, 1)))
        out.update(dx=torch.cat(dxs + [d[2]], dim=-1), dwq=dws[0], dwk=dws[1])
    return out


def rope(x, cos, sin, B, T, nh, nkv, hd):
    """Half-split rotation of the q and k heads of packed float64 rows at position ``row % T`` (element i pairs with
    i + hd/2; first half of the fp32 tables read and widened); v passes through."""
    nrot, half = nh + nkv, hd // 2
    blk = x[:, :nrot * hd].reshape(B, T, nrot, hd)
    c = cos[:T, :half].double()[None, :, None, :]
    s = sin[:T, :half].double()[None, :, None, :]
    x1, x2 = blk[..., :half], blk[..., half:]
    rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).reshape(B * T, nrot * hd)
    return torch.cat([rot, x[:, nrot * hd:]], dim=1)


def qk_norm_rope(qkv, wq, wk, cos, sin, B, T, nh, nkv, hd, eps, round_to=None):
    """The norm followed by the rotation.  ``round_to`` (a torch dtype): the normed value is rounded to it before the
    rotation, as the kernels' rounding contract states."""
    y = qk_norm(qkv, wq, wk, nh, nkv, hd, eps)["y"]
    if round_to is not None:
        y = y.to(round_to).double()
    return rope(y, cos, sin, B, T, nh, nkv, hd)


# ------------------------------------------------------------------------------------------ the model
def logits64(c, P, ids, kstart=None, doc_start=None):
    """``_model_oracle.logits64`` for a config with ``qk_norm``: q and k are normed per head (weights
    ``self_attn.q_norm.weight`` / ``k_norm.weight``, [hd]) between their projections and the rotation."""
    assert c.qk_norm and (kstart is None or doc_start is None)
    nh, nkv, hd, eps = c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.rms_norm_eps
    B, T = ids.shape
    dev = ids.device
    cos, sin = mo.rope_tables(T, hd, c.rope_theta, c.rope_scaling, dev)
    t = torch.arange(T, device=dev)
    ok = (t[None, :] <= t[:, None])[None].expand(B, T, T).clone()
    if kstart is not None:
        ok &= t.view(1, 1, T) >= kstart.to(dev).long().view(B, 1, 1)
    if doc_start is not None:
        ok &= t.view(1, 1, T) >= doc_start.to(dev).long().view(B, T, 1)
    ok = ok[:, None]
    seen = ok.any(-1, keepdim=True)
    h = P["embed"][ids]
    for i in range(c.num_hidden_layers):
        p = f"model.layers.{i}."
        y = mo._norm(h, P[p + "input_layernorm.weight"], eps)
        q = (y @ P[p + "self_attn.q_proj.weight"].t()).view(B, T, nh, hd)
        k = (y @ P[p + "self_attn.k_proj.weight"].t()).view(B, T, nkv, hd)
        v = (y @ P[p + "self_attn.v_proj.weight"].t()).view(B, T, nkv, hd).transpose(1, 2)
        q = mo._norm(q, P[p + "self_attn.q_norm.weight"], eps).transpose(1, 2)
        k = mo._norm(k, P[p + "self_attn.k_norm.weight"], eps).transpose(1, 2)
        q, k = mo._rotate(q, cos, sin), mo._rotate(k, cos, sin)
        k, v = k.repeat_interleave(nh // nkv, dim=1), v.repeat_interleave(nh // nkv, dim=1)
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        s = torch.where(seen, s.masked_fill(~ok, float("-inf")), torch.zeros_like(s))
        a = (torch.softmax(s, dim=-1) * seen) @ v
        h = h + a.transpose(1, 2).reshape(B, T, nh * hd) @ P[p + "self_attn.o_proj.weight"].t()
        y = mo._norm(h, P[p + "post_attention_layernorm.weight"], eps)
        g, u = y @ P[p + "mlp.gate_proj.weight"].t(), y @ P[p + "mlp.up_proj.weight"].t()
        h = h + (g * torch.sigmoid(g) * u) @ P[p + "mlp.down_proj.weight"].t()
    return mo._norm(h, P["model.norm.weight"], eps) @ P["lm"].t()


def grads64(m, ids, labels, loss_scale=1.0, kstart=None, doc_mask=False):
    """(loss, {HF parameter name: float64 gradient of loss_scale * loss}) of the QK-norm model ``m``, by
    torch.autograd through ``logits64``; tied weights: the two uses summed."""
    c = m.config
    P = {k: v.requires_grad_(True) for k, v in mo.weights64(m, ids.device).items()}
    ds = mo.doc_starts(ids, c.eos_token_id) if doc_mask else None
    loss = mo.loss64(logits64(c, P, ids, kstart=kstart, doc_start=ds), labels)
    keys = list(P)
    gs = dict(zip(keys, torch.autograd.grad(loss * loss_scale, [P[k] for k in keys])))
    out = {k: g for k, g in gs.items() if k not in ("embed", "lm")}
    if c.tie_word_embeddings:
        out["model.embed_tokens.weight"] = gs["embed"] + gs["lm"]
    else:
        out["model.embed_tokens.weight"], out["lm_head.weight"] = gs["embed"], gs["lm"]
    return loss.detach(), out
