"""``ops.sample`` off the GPU: the PyTorch twin against the contract in float64, its kept set against ``filter_logits``,
the ``sampler`` option and the argument checks.  ``thr64`` / ``cdf64`` are the float64 reference of the GPU tests too."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.generate import build_parser
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.models.llama import filter_logits

from .test_generate_cpu import CFG

TOL = 5e-5  # on a mass ratio: three fp32 roundings of an exponent argument |a| <= 40, times 3 (the issue's derivation)
# (top_k, top_p); top_k = None stands for V + 3
STAGES = [(0, 1.0), (1, 1.0), (50, 1.0), (0, 0.9), (50, 0.9), (None, 0.05)]


def thr64(row, temperature, top_k, p):
    """The smallest kept logit by the contract, in float64 (a sort of the values is allowed here)."""
    x = row.double().sort(descending=True).values
    if 0 < top_k < x.numel():
        x = x[x >= x[top_k - 1]]
    if p >= 1.0:
        return x[-1]
    m = ((x - x[0]) / temperature).exp()
    return x[(m.cumsum(0) - m) / m.sum() < p].min()


def cdf64(row, temperature, thr):
    """The index-order CDF over {i: row_i >= thr}, float64."""
    m = torch.where(row >= thr, ((row.double() - row.double().max()) / temperature).exp(), 0.0)
    return m.cumsum(0) / m.sum()


def brute_force_rows():
    """The rows of test_generate_cpu.test_filter_logits_against_brute_force (dyadic masses, ties)."""
    ln2 = torch.log(torch.tensor(2.0, dtype=torch.float64))
    base = (torch.tensor([-1.0, -2.0, -3.0, -4.0, -5.0, -6.0, -7.0, -7.0, -3.0, -2.0], dtype=torch.float64) * ln2).float()
    g = torch.Generator().manual_seed(0)
    return torch.stack([base, base[torch.randperm(10, generator=g)], torch.randn(10, generator=g),
                        torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0, -1.0, 2.0, 2.0, -3.0, 0.5])])


def check_rows(x, u, tok, thr, nkept, temperature, top_k, top_p):
    """Kept set and draw of every row against the float64 rules; returns the worst (G/Z, CDF) excess over them."""
    worst = [0.0, 0.0]
    for r in range(x.shape[0]):
        if top_p >= 1.0:
            assert thr[r].item() == thr64(x[r], temperature, top_k, 1.0).item()
        else:
            lo, hi = (thr64(x[r], temperature, top_k, top_p + s * TOL).item() for s in (1, -1))
            assert lo <= thr[r].item() <= hi, (r, lo, thr[r].item(), hi)
            # how far G/Z is on the wrong side of top_p at the threshold and at the next kept logit below it
            kept = x[r][x[r] >= thr64(x[r], temperature, top_k, 1.0)].double()
            m, low = ((kept - kept.max()) / temperature).exp(), kept[kept < thr[r]]
            above = lambda v: float(m[kept > v].sum() / m.sum())
            worst[0] = max(worst[0], above(thr[r]) - top_p, top_p - above(low.max()) if low.numel() else 0.0)
        assert int(nkept[r]) == int((x[r] >= thr[r]).sum())
        j, F = int(tok[r]), cdf64(x[r], temperature, thr[r])
        assert x[r, j] >= thr[r] and x[r, j] > float("-inf")
        below = float(F[j - 1]) if j else 0.0
        assert below - TOL <= float(u[r]) <= float(F[j]) + TOL, (r, j, below, float(u[r]), float(F[j]))
        worst[1] = max(worst[1], below - float(u[r]), float(u[r]) - float(F[j]))
    return worst


@pytest.mark.parametrize("V", [1, 7, 257])
@pytest.mark.parametrize("top_k,top_p", STAGES)
def test_twin_against_float64(V, top_k, top_p):
    g = torch.Generator().manual_seed(V)
    x = torch.randn(4, V, generator=g) * 4
    if V > 4:
        x[1, 1:V // 2] = float("-inf")
        x[2, :3] = x[2].max()  # ties at the top
    top_k = V + 3 if top_k is None else top_k
    for u in (torch.zeros(4), torch.full((4,), 1 - 2.0 ** -24), torch.rand(4, generator=g)):
        tok, thr, nkept = ops.sample(x, u, 0.7, top_k, top_p, return_stats=True)
        assert tok.dtype == torch.int64 and thr.dtype == torch.float32 and nkept.dtype == torch.int32
        check_rows(x, u, tok, thr, nkept, 0.7, top_k, top_p)
        assert torch.equal(tok, ops.sample(x, u, 0.7, top_k, top_p))


def test_twin_keeps_what_filter_logits_keeps():
    rows = brute_force_rows()
    for top_k in (0, 1, 2, 3, 5, 10, 50):
        for top_p in (1.0, 0.9, 0.5, 0.26, 0.05):
            _, thr, nkept = ops.sample(rows, torch.zeros(4), 1.0, top_k, top_p, return_stats=True)
            kept = filter_logits(rows, top_k, top_p) > float("-inf")
            assert torch.equal(rows >= thr[:, None], kept), (top_k, top_p)
            assert torch.equal(nkept.long(), kept.sum(-1))


def test_sampler_option():
    assert build_parser().parse_args(["--checkpoint", "x"]).sampler == "torch"
    assert build_parser().parse_args(["--checkpoint", "x", "--sampler", "fused"]).sampler == "fused"
    m = LlamaForCausalLM(LlamaConfig.from_dict(CFG)).init_weights(5)
    ids = torch.randint(3, CFG["vocab_size"], (2, 7), generator=torch.Generator().manual_seed(3))
    with pytest.raises(ValueError):
        m.generate(ids, max_new_tokens=2, sampler="nope")
    kw = dict(max_new_tokens=6, eos_token_id=None)
    greedy = m.generate(ids, **kw)
    assert torch.equal(m.generate(ids, temperature=0.8, top_k=1, sampler="fused", **kw), greedy)
    assert torch.equal(m.generate(ids, sampler="fused", **kw), greedy)
    a = m.generate(ids, temperature=1.0, top_k=20, seed=1, sampler="fused", **kw)
    assert torch.equal(a, m.generate(ids, temperature=1.0, top_k=20, seed=1, sampler="fused", **kw))
    assert not torch.equal(a, m.generate(ids, temperature=1.0, top_k=20, seed=2, sampler="fused", **kw))


@pytest.mark.parametrize("bad", [dict(logits=torch.zeros(2, 8, dtype=torch.float64)), dict(logits=torch.zeros(8)),
                                 dict(u=torch.zeros(3)), dict(u=torch.zeros(2, dtype=torch.float64)),
                                 dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")),
                                 dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1)])
def test_argument_errors(bad):
    kw = dict(logits=torch.zeros(2, 8), u=torch.zeros(2), temperature=1.0, top_k=0, top_p=1.0)
    with pytest.raises(ValueError):
        ops.sample(**{**kw, **bad})
