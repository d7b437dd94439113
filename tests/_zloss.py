"""float64 oracle and fp32 twin of the lm-head cross-entropy with z-loss (``csrc/cross_entropy.hip`` Z kernels,
``ops.lm_head_ce(..., z_loss=)``), written from the formulae of docs/DESIGN.md "z-loss"; neither calls the code
under test.  Per row with a valid target t (ignored rows give 0 everywhere):

    lse = logsumexp(x)   p_j = exp(x_j - lse)   CE = lse - x_t   Z = lse^2
    dlogits_j = s * (p_j * (1 + 2 z_coef lse) - [j == t]),   s = loss_scale / n_valid

``tests/test_zloss_cpu.py`` checks the oracle against float64 autograd of the objective; ``tests/test_zloss_gpu.py``
uses it against the HIP kernels.
"""
import torch

IGN = -100


def _rows(x, targets, scale, z_coef):
    lse = torch.logsumexp(x, dim=-1)
    ok = targets != IGN
    safe = torch.where(ok, targets, torch.zeros_like(targets))
    zero = torch.zeros_like(lse)
    ce = torch.where(ok, lse - x.gather(1, safe[:, None])[:, 0], zero)
    z = torch.where(ok, lse * lse, zero)
    p = torch.exp(x - lse[:, None]) * (1.0 + 2.0 * z_coef * lse)[:, None]
    p.scatter_add_(1, safe[:, None], -torch.ones_like(p[:, :1]))
    return lse, ce, z, p * (ok[:, None].to(x.dtype) * scale)


def ce_z_rows(logits, targets, scale, z_coef):
    """float64 (lse, CE row, lse^2 row, dlogits); ``scale`` = s, ``z_coef`` the C float the kernel receives."""
    return _rows(logits.double(), targets, float(scale), float(z_coef))


def ce_z_rows_twin(logits32, targets, scale, z_coef):
    """The same formulae in fp32 PyTorch (``scale``: an fp32 tensor or a number)."""
    assert logits32.dtype == torch.float32
    return _rows(logits32, targets, scale, float(z_coef))


def lm_head_ce_z(y, w, targets, loss_scale, z_coef):
    """float64 oracle of the whole op on the operands as stored: (CE mean, weighted z term, dy, gW) with
    dy = dlogits W and gW = dlogits^T y, dlogits scaled by loss_scale / n_valid."""
    y64, w64 = y.double(), w.double()
    n_valid = max(1, int((targets != IGN).sum()))
    _, ce, z, dl = ce_z_rows(y64 @ w64.t(), targets, loss_scale / n_valid, z_coef)
    return ce.sum() / n_valid, float(z_coef) * z.sum() / n_valid, dl @ w64, dl.t() @ y64


def autograd_ce_z(y, w, targets, loss_scale, z_coef):
    """The same four results from float64 autograd of the objective on explicit logits."""
    y64 = y.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    x = y64 @ w64.t()
    ok = targets != IGN
    n_valid = max(1, int(ok.sum()))
    ce = torch.nn.functional.cross_entropy(x, targets, ignore_index=IGN, reduction="sum") / n_valid
    z = float(z_coef) * (torch.logsumexp(x, dim=-1)[ok] ** 2).sum() / n_valid
    (loss_scale * (ce + z)).backward()
    return ce.detach(), z.detach(), y64.grad, w64.grad
