"""Dense soft-capped attention for the tests of ``softcap=``: z = C tanh(scale q.k / C), a boolean mask, softmax, P V,
on packed rows q|k|v [B*T, (nh + 2 nkv) hd] as the kernels see them (q|k already rotated)."""
import torch


def mask(B, T, device, kstart=None, doc_start=None, window=None):
    """Boolean [B, 1, T, T]: key <= query, key >= kstart[b], key >= doc_start[b, q], key > query - window."""
    t = torch.arange(T, device=device)
    ok = (t[None, :] <= t[:, None]).expand(B, T, T).clone()
    if kstart is not None:
        ok &= t.view(1, 1, T) >= kstart.to(device).long().view(B, 1, 1)
    if doc_start is not None:
        ok &= t.view(1, 1, T) >= doc_start.to(device).long().view(B, T, 1)
    if window:
        ok &= t.view(1, 1, T) > t.view(1, T, 1) - window
    return ok.unsqueeze(1)


def attention(qkv, B, T, nh, nkv, hd, cap, ok, dO=None, dtype=torch.float64, rnd=None):
    """o [B*T, nh*hd], lse [B, nh, T] (log2 domain; -inf on rows without a key, whose o is 0), seen [B, T]; with ``dO``
    the packed dqkv.  ``rnd`` None: the plain function, gradients from autograd.  ``rnd`` (the twin: to bf16 and back):
    the kernels' rounding points -- P before P V and P^T dO, O in delta, dS before dS K and dS^T Q -- with the backward
    written out, dS = P (dP - delta) (1 - t^2)."""
    x = qkv.detach().to(dtype).clone().requires_grad_(dO is not None and rnd is None)
    r = rnd or (lambda a: a)
    rep, scale = nh // nkv, hd ** -0.5
    q, k, v = x.view(B, T, -1).split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    q = q.reshape(B, T, nh, hd).transpose(1, 2)
    k = k.reshape(B, T, nkv, hd).transpose(1, 2).repeat_interleave(rep, dim=1)
    v = v.reshape(B, T, nkv, hd).transpose(1, 2).repeat_interleave(rep, dim=1)
    t = torch.tanh((q @ k.transpose(-1, -2)) * (scale / cap))
    z = (cap * t).masked_fill(~ok, float("-inf"))
    m = z.amax(-1, keepdim=True)
    seen = torch.isfinite(m)
    p = torch.exp(z - torch.where(seen, m, torch.zeros_like(m)))
    l = p.sum(-1, keepdim=True)
    l1 = torch.where(seen, l, torch.ones_like(l))
    rows = lambda t4: t4.transpose(1, 2).reshape(B * T, -1)  # noqa: E731
    o = rows((r(p) @ v) / l1)
    out = {"o": o.detach(), "lse": ((m + torch.log(l)) * 1.4426950408889634)[..., 0].detach(), "seen": seen[:, 0, :, 0]}
    if dO is not None and rnd is None:
        out["dqkv"] = torch.autograd.grad(o, x, dO.to(dtype))[0]
    elif dO is not None:
        d = dO.to(dtype).view(B, T, nh, hd).transpose(1, 2)
        delta = (d * r(o).view(B, T, nh, hd).transpose(1, 2)).sum(-1, keepdim=True)
        dS = r(p / l1 * (d @ v.transpose(-1, -2) - delta) * (1 - t * t))
        dk = (scale * (dS.transpose(-1, -2) @ q)).view(B, nkv, rep, T, hd).sum(2)
        dv = (r(p / l1).transpose(-1, -2) @ d).view(B, nkv, rep, T, hd).sum(2)
        out["dqkv"] = torch.cat([rows(scale * (dS @ k)), rows(dk), rows(dv)], dim=1)
    return out


def oracle_and_twin(*a, dO=None):
    """(float64 oracle, twin); the twin's LSE (an fp32 output) is the plain function in fp32."""
    twin = attention(*a, dO, rnd=lambda t: t.bfloat16().to(t.dtype))
    twin["lse"] = attention(*a, dtype=torch.float32)["lse"]
    return attention(*a, dO), twin
