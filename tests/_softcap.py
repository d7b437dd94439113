"""float64 oracle and fp32 twin of the lm-head cross-entropy on soft-capped logits (``csrc/cross_entropy.hip`` CAP
kernels, ``csrc/ce_loss.hip``, ``ops.lm_head_ce(..., softcap=)``), written from the formulae of docs/DESIGN.md "Logit
soft-capping"; neither calls the code under test.  With t_j = tanh(x_j / C) and y_j = C t_j, per row with a valid
target t (ignored rows give 0 everywhere):

    lse = logsumexp(y)   p_j = exp(y_j - lse)   CE = lse - y_t   Z = lse^2
    dlogits_j = s * (p_j * g - [j == t]) * (1 - t_j^2),   s = loss_scale / n_valid,   g = 1 + 2 z_coef lse

``tests/test_softcap_cpu.py`` checks the oracle against float64 autograd of the objective;
``tests/test_softcap_gpu.py`` uses it against the HIP kernels.
"""
import torch

IGN = -100


def softcap64(x, cap):
    """float64 C tanh(x / C) of the stored values."""
    return float(cap) * torch.tanh(x.double() / float(cap))


def softcap_twin(x32, cap):
    assert x32.dtype == torch.float32
    return float(cap) * torch.tanh(x32 / float(cap))


def _rows(x, targets, scale, z_coef, cap):
    t = torch.tanh(x / cap)
    y = cap * t
    lse = torch.logsumexp(y, dim=-1)
    ok = targets != IGN
    safe = torch.where(ok, targets, torch.zeros_like(targets))
    zero = torch.zeros_like(lse)
    ce = torch.where(ok, lse - y.gather(1, safe[:, None])[:, 0], zero)
    z = torch.where(ok, lse * lse, zero)
    p = torch.exp(y - lse[:, None]) * (1.0 + 2.0 * z_coef * lse)[:, None]
    p.scatter_add_(1, safe[:, None], -torch.ones_like(p[:, :1]))
    return lse, ce, z, p * (ok[:, None].to(x.dtype) * scale) * (1 - t * t)


def ce_cap_rows(logits, targets, scale, z_coef, cap):
    """float64 (lse, CE row, lse^2 row, dlogits); ``scale`` = s, ``z_coef`` and ``cap`` the C floats the kernel
    receives (z_coef 0.0: no z-loss)."""
    return _rows(logits.double(), targets, float(scale), float(z_coef), float(cap))


def ce_cap_rows_twin(logits32, targets, scale, z_coef, cap):
    """The same formulae in fp32 PyTorch: ``torch.tanh`` and ``1 - t * t`` (``scale``: an fp32 tensor or a number)."""
    assert logits32.dtype == torch.float32
    return _rows(logits32, targets, scale, float(z_coef), float(cap))


def lm_head_ce_cap(y, w, targets, loss_scale, z_coef, cap):
    """float64 oracle of the whole op on the operands as stored: (CE mean, weighted z term, dy, gW) with
    dy = dlogits W and gW = dlogits^T y, dlogits scaled by loss_scale / n_valid."""
    y64, w64 = y.double(), w.double()
    n_valid = max(1, int((targets != IGN).sum()))
    _, ce, z, dl = ce_cap_rows(y64 @ w64.t(), targets, loss_scale / n_valid, z_coef, cap)
    return ce.sum() / n_valid, float(z_coef) * z.sum() / n_valid, dl @ w64, dl.t() @ y64


def autograd_ce_cap(y, w, targets, loss_scale, z_coef, cap):
    """The same four results from float64 autograd of the objective on explicit logits."""
    y64 = y.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    x = float(cap) * torch.tanh((y64 @ w64.t()) / float(cap))
    ok = targets != IGN
    n_valid = max(1, int(ok.sum()))
    ce = torch.nn.functional.cross_entropy(x, targets, ignore_index=IGN, reduction="sum") / n_valid
    z = float(z_coef) * (torch.logsumexp(x, dim=-1)[ok] ** 2).sum() / n_valid
    (loss_scale * (ce + z)).backward()
    return ce.detach(), z.detach(), y64.grad, w64.grad
