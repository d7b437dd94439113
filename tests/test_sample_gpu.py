"""The fused sampler on the GPU (csrc/sample.hip): kept set and draw of ``nd_sample_topk_topp`` against the float64
rules of test_sample_cpu.py (``thr64``, ``cdf64``, ``TOL`` and its derivation), invariance under the batch, the model.

Measured (docs/PARITY.md "Fused sampler"): the worst G/Z and CDF excess over the float64 rules are printed per case."""
import functools

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import _ext

from ._frames import assert_frame_intact, framed_flat
from .test_generate_gpu import _config
from .test_sample_cpu import STAGES, brute_force_rows, check_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
RES_MAX = 39936  # csrc/sample.hip: the longest row whose keys stay in LDS; one more takes the streaming variant
VS = [1, 7, 257, 4099, 32000, RES_MAX, RES_MAX + 1, 128256]
U_TOP = 1 - 2.0 ** -24  # the largest fp32 below 1


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    yield
    ops.set_backend("auto")


def rows(V, B, top_k):
    """Seeded randn * 4; with B = 5 also a row with a block of -inf and one with ties straddling the k-th place."""
    if V == 10:
        return brute_force_rows().to(DEV)
    g = torch.Generator(device=DEV).manual_seed(V + B)
    x = torch.randn(B, V, device=DEV, generator=g) * 4
    if B > 1 and V > 4:
        x[1, V // 4:V // 2] = float("-inf")
        kth = x[2].sort(descending=True).values[min(max(top_k, 1), V) - 1]
        x[2, torch.randperm(V, device=DEV, generator=g)[:3]] = kth
    return x


def launch(x, u, temperature, top_k, top_p):
    """``nd_sample_topk_topp`` into framed outputs (tok: an int64 view of a framed int32 buffer)."""
    B, V = x.shape
    (bt, t32), (bh, thr), (bn, nkept) = framed_flat(2 * B, torch.int32), framed_flat(B, torch.float32), \
        framed_flat(B, torch.int32)
    tok = t32.view(torch.int64)
    _ext.check(_ext.lib().nd_sample_topk_topp(x.data_ptr(), u.data_ptr(), tok.data_ptr(), thr.data_ptr(),
                                              nkept.data_ptr(), B, V, x.stride(0), temperature, top_k, top_p,
                                              _ext.stream_ptr(x.device)), "nd_sample_topk_topp")
    torch.cuda.synchronize()
    for big, view in ((bt, t32), (bh, thr), (bn, nkept)):
        assert_frame_intact(big, view)
    return tok.clone(), thr.clone(), nkept.clone()


@functools.lru_cache(maxsize=None)
def run(V, stage):
    """One case, launched once for the three u: (x, temperature, top_k, top_p, [(u, tok, thr, nkept)])."""
    top_k, top_p = STAGES[stage]
    top_k = V + 3 if top_k is None else top_k
    B, temperature = (5 if (VS + [10]).index(V) % 2 == stage % 2 else 1), (0.7, 1.0)[stage % 2]
    x = rows(V, B, top_k)
    if V == 257:  # a row stride > V
        x = torch.cat([x, torch.full((x.shape[0], 5), float("nan"), device=DEV)], dim=1)[:, :V]
    g = torch.Generator(device=DEV).manual_seed(stage)
    us = [torch.zeros(x.shape[0], device=DEV), torch.full((x.shape[0],), U_TOP, device=DEV),
          torch.rand(x.shape[0], device=DEV, generator=g)]
    return x, temperature, top_k, top_p, [(u,) + launch(x, u, temperature, top_k, top_p) for u in us]


CASES = [(V, s) for V in VS + [10] for s in range(len(STAGES))]


@pytest.mark.parametrize("V,stage", CASES)
def test_kept_set_and_draw(V, stage):
    x, temperature, top_k, top_p, outs = run(V, stage)
    worst = [0.0, 0.0]
    for u, tok, thr, nkept in outs:
        w = check_rows(x.cpu(), u.cpu(), tok.cpu(), thr.cpu(), nkept.cpu(), temperature, top_k, top_p)
        worst = [max(a, b) for a, b in zip(worst, w)]
        assert torch.equal(thr.view(torch.int32), outs[0][2].view(torch.int32)) and torch.equal(nkept, outs[0][3])
    print(f"\n[excess] V {V} k {top_k} p {top_p}: G/Z {worst[0]:.3g}, CDF {worst[1]:.3g} (allowed 5e-5)", end="")
    # the launcher gives what the raw call gave
    got = ops.sample(x, outs[2][0], temperature, top_k, top_p, return_stats=True)
    assert all(torch.equal(a, b) for a, b in zip(got, outs[2][1:]))


@pytest.mark.parametrize("V", [7, 32000])
def test_top1_is_the_argmax_and_ties_split_by_u(V):
    x = rows(V, 1, 1).repeat(4, 1).roll(1, 1) * torch.tensor([[1.0], [-1.0], [0.5], [2.0]], device=DEV)
    x[3, [V // 3, V - 2]] = x[3].max() + 1  # two tied maxima
    for u, at in ((0.0, V // 3), (U_TOP, V - 2), (0.37, None)):
        tok, _, nkept = launch(x, torch.full((4,), u, device=DEV), 0.7, 1, 1.0)
        assert torch.equal(tok[:3], x.argmax(-1)[:3]) and nkept.tolist() == [1, 1, 1, 2]
        assert int(tok[3]) in ((V // 3, V - 2) if at is None else (at,))


@pytest.mark.parametrize("V", [257, 32000, RES_MAX + 1])
def test_a_row_alone_equals_itself_in_a_batch(V):
    x, temperature, top_k, top_p, outs = run(V, 4)  # top-k 50 and top-p 0.9 on the B = 5 rows
    assert x.shape[0] == 5
    u, tok, thr, nkept = outs[2]
    for r in range(5):
        one = ops.sample(x[r:r + 1], u[r:r + 1], temperature, top_k, top_p, return_stats=True)
        for a, b in zip(one, (tok, thr, nkept)):
            assert torch.equal(a.view(torch.int32), b[r:r + 1].view(torch.int32))


def test_model_with_the_fused_sampler():
    cfg = _config("tiny")
    m = LlamaForCausalLM(cfg, DEV, torch.bfloat16).init_weights(7)
    ids = torch.randint(3, cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(12)).to(DEV)
    kw = dict(max_new_tokens=12, eos_token_id=None)
    assert torch.equal(m.generate(ids, temperature=0.8, top_k=1, sampler="fused", **kw), m.generate(ids, **kw))
    kw.update(temperature=1.0, top_k=20, sampler="fused")
    a, lg = m.generate(ids, seed=3, hip_graph=False, return_logits=True, **kw)
    assert torch.equal(a, m.generate(ids, seed=3, hip_graph=False, **kw))
    assert torch.equal(a, m.generate(ids, seed=3, hip_graph=True, **kw))
    assert not torch.equal(a, m.generate(ids, seed=4, hip_graph=False, **kw))
    # among the step's 20 best logits, by value: the bf16 head's logits tie, and ties at the 20th place are all kept
    assert bool((lg.gather(-1, a[:, 9:, None]) >= lg.topk(20, dim=-1).values[..., -1:]).all())
