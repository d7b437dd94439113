"""The float64 model oracle (tests/_model_oracle.py) is checked before anything is held against it: per parameter
against the project's PyTorch path on the CPU (fp32; tolerances of test_model_cpu.test_logits_loss_grads_match_hf),
against HF ``LlamaForCausalLM`` in float64, and one negative control per clause of the gradient rule."""
import pytest
import torch

from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM

from . import _model_oracle as mo

BASE = dict(hidden_size=64, intermediate_size=96, num_attention_heads=4, num_hidden_layers=2, vocab_size=101,
            rms_norm_eps=1e-5)
CASES = {
    "mha": dict(),
    "gqa42": dict(cfg=dict(num_key_value_heads=2)),
    "gqa41": dict(cfg=dict(num_key_value_heads=1)),
    "tied": dict(cfg=dict(tie_word_embeddings=True)),
    "left_pad": dict(cfg=dict(num_key_value_heads=2), pad="left"),
    "right_pad": dict(cfg=dict(num_key_value_heads=2), pad="right"),
    "doc_mask": dict(cfg=dict(num_key_value_heads=2), doc=True),
    "loss_scale": dict(cfg=dict(num_key_value_heads=2), loss_scale=0.25),
    "accumulate": dict(cfg=dict(num_key_value_heads=2), micro=2, loss_scale=0.5),
    "all_ignored": dict(ignore_all=True),
}
B, T = 3, 24


def _batch(c, seed, pad=None, doc=False, ignore_all=False):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, c.vocab_size, (B, T), generator=g)
    mask = None
    if pad:
        mask = torch.ones(B, T, dtype=torch.long)
        for b, n in enumerate([0, 5, 11]):
            if n and pad == "left":
                mask[b, :n] = 0
            elif n:
                mask[b, T - n:] = 0
        ids[mask == 0] = 2
    if doc:
        ids[:, 7] = c.eos_token_id  # an EOS inside the window: tokens 8.. never see tokens 0..7
        ids[1, 15] = c.eos_token_id
    labels = ids.clone()
    labels[0, 3:9] = -100  # a run of ignored targets
    labels[2, T - 4:] = -100
    if mask is not None:
        labels[mask == 0] = -100
    if ignore_all:
        labels[:] = -100
    return ids, labels, mask


def _project(c, batches, loss_scale, doc):
    m = LlamaForCausalLM(c, doc_mask=doc).init_weights(1)  # fp32 on the CPU: the shadow is the master
    losses = []
    for ids, labels, mask in batches:
        out = m(ids, labels=labels, attention_mask=mask, loss_scale=loss_scale)
        out.loss.backward()
        losses.append(out.loss.detach())
    return m, losses


@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_matches_torch_path(case):
    spec = CASES[case]
    c = LlamaConfig.from_dict({**BASE, **spec.get("cfg", {})})
    ls = spec.get("loss_scale", 1.0)
    batches = [_batch(c, 10 + i, spec.get("pad"), spec.get("doc", False), spec.get("ignore_all", False))
               for i in range(spec.get("micro", 1))]
    m, losses = _project(c, batches, ls, spec.get("doc", False))
    l64, g64 = mo.grads64_sum(m, [(i, l, mo.key_start(k) if k is not None else None) for i, l, k in batches], ls,
                              doc_mask=spec.get("doc", False))
    for a, b in zip(losses, l64):
        assert abs(float(a) - float(b)) < 1e-5, (case, float(a), float(b))
    assert set(g64) == set(m.store.names)
    for n in m.store.names:
        assert torch.allclose(m.store.grad_view(n).double(), g64[n], atol=2e-6, rtol=1e-4), (case, n)
    if spec.get("ignore_all"):
        assert float(l64[0]) == 0.0 and all(not bool(g.any()) for g in g64.values())
    else:
        assert all(bool(g.any()) for g in g64.values())
    if spec.get("doc"):  # the mask does something: the same batch without it has other gradients
        _, plain = mo.grads64_sum(m, [(i, l, None) for i, l, _ in batches], ls)
        assert not torch.allclose(plain["model.layers.0.self_attn.k_proj.weight"],
                                  g64["model.layers.0.self_attn.k_proj.weight"], rtol=1e-3, atol=0)


@pytest.mark.parametrize("case", ["mha", "gqa42", "tied"])
def test_oracle_matches_hf_float64(case):
    transformers = pytest.importorskip("transformers")
    cfgd = {**BASE, **CASES[case].get("cfg", {})}
    c = LlamaConfig.from_dict(cfgd)
    m = LlamaForCausalLM(c).init_weights(1)
    hf = transformers.LlamaForCausalLM(transformers.LlamaConfig(**cfgd, attn_implementation="eager")).double()
    hf.load_state_dict({k: v.clone().double() for k, v in m.state_dict().items()}, strict=False)
    if c.tie_word_embeddings:
        hf.tie_weights()
    ids, labels, _ = _batch(c, 10)
    ho = hf(input_ids=ids, labels=labels)
    # "float64" HF keeps three things in fp32 whatever the model's dtype: the RMSNorm statistics, the softmax of the
    # eager attention and the logits inside its loss function.  Each is a relative rounding of 2^-24 = 6e-8 per
    # element, so the comparison is made at rtol 1e-5 with an absolute floor 200 x below the fp32 comparison's
    # (test_model_cpu: rtol 1e-4, atol 2e-6), not at float64 rounding; the loss that is differentiated is stock
    # cross_entropy on HF's float64 logits.
    loss = torch.nn.functional.cross_entropy(ho.logits[:, :-1].reshape(-1, c.vocab_size), labels[:, 1:].reshape(-1),
                                             ignore_index=-100)
    assert loss.dtype == torch.float64
    loss.backward()
    l64, g64 = mo.grads64(m, ids, labels)
    assert abs(float(l64) - float(ho.loss.detach())) < 1e-6  # HF's own fp32 loss
    assert abs(float(l64) - float(loss.detach())) < 1e-8
    assert torch.allclose(mo.forward64(m, ids), ho.logits.detach(), atol=1e-7, rtol=1e-5)
    names = [n for n, _ in hf.named_parameters()]
    assert set(names) == set(g64)
    for n, p in hf.named_parameters():
        err = (p.grad - g64[n]).abs().max().item()
        print(f"[{case}] {n}: max |HF - oracle| = {err:.2e} at max |g| = {g64[n].abs().max().item():.2e}")
        assert torch.allclose(p.grad, g64[n], atol=1e-8, rtol=1e-5), (case, n)


# ------------------------------------------------------------------------------------------ the rule bites
def _rule_inputs():
    """An oracle gradient and two bf16-like neighbours of it (independent relative noise of 2^-8 of the tensor's
    rms): the twin, and an output that is inside the rule."""
    c = LlamaConfig.from_dict({**BASE, "num_key_value_heads": 2})
    m = LlamaForCausalLM(c).init_weights(1)
    ids, labels, _ = _batch(c, 10)
    _, g64 = mo.grads64(m, ids, labels)
    gen = torch.Generator().manual_seed(0)

    def noisy(g):
        return g + torch.randn(g.shape, generator=gen, dtype=torch.float64) * g.pow(2).mean().sqrt() * 2.0 ** -8

    return g64, {k: noisy(v) for k, v in g64.items()}, {k: noisy(v) for k, v in g64.items()}


NAME = "model.layers.1.post_attention_layernorm.weight"
MAT = "model.layers.0.self_attn.k_proj.weight"


def test_rule_accepts_the_twin_level_and_rejects_each_fault():
    g64, twin, out = _rule_inputs()
    report = {}
    mo.check_grads(out, g64, twin, margin=8.0, beta_bound=1e-2, report=report)
    assert set(report) == {".".join(p for p in n.split(".") if not p.isdigit()) for n in g64}
    assert all(0 < e["margin"] <= 8 and e["beta"] <= 1e-2 for e in report.values())
    unit = (twin[MAT] - g64[MAT]).abs().max()

    moved = {k: v.clone() for k, v in out.items()}  # one element moved: the per-element clause, and only it
    moved[MAT][3, 5] = g64[MAT][3, 5] + 9.0 * unit
    with pytest.raises(AssertionError) as e:
        mo.check_grads(moved, g64, twin, margin=8.0, beta_bound=1e-2)
    assert "per element: " + MAT in str(e.value) and "1 of" in str(e.value) and "projection" not in str(e.value)

    row = {k: v.clone() for k, v in out.items()}  # one row scaled by 2: the per-element clause
    row[MAT][7] *= 2.0
    with pytest.raises(AssertionError) as e:
        mo.check_grads(row, g64, twin, margin=8.0, beta_bound=1e-2)
    assert "per element: " + MAT in str(e.value) and "worst at (7," in str(e.value)

    for name in (NAME, MAT):  # the whole tensor scaled by 0.97: the projection clause
        scaled = {k: v.clone() for k, v in out.items()}
        scaled[name] *= 0.97
        with pytest.raises(AssertionError) as e:
            mo.check_grads(scaled, g64, twin, margin=8.0, beta_bound=1e-2)
        assert f"projection: {name}" in str(e.value) and "beta = -3" in str(e.value)


def test_loss_clause_and_spy_expectations():
    mo.check_loss(6.9010, 6.9, 6.9004, margin=8.0, floor=0.0)
    mo.check_loss(6.9001, 6.9, 6.9, margin=8.0, floor=2e-4)
    with pytest.raises(AssertionError):
        mo.check_loss(6.95, 6.9, 6.9004, margin=8.0, floor=2e-4)

    class Lib:
        def nd_a(self, x):
            return x + 1

        def nd_b(self):
            return 0

        def nd_c(self):
            return 1  # hipErrorInvalidValue: the launcher refused the shape

        def nd_c_splits(self):
            return 1  # a plan, not an error

    spy = mo.LauncherSpy(Lib())
    assert spy.nd_a(1) == 2 and spy.nd_a(2) == 3
    spy.expect(ran=["nd_a"], at_least=2, never=["nd_b"])
    with pytest.raises(AssertionError):
        spy.expect(ran=["nd_a"], at_least=3)
    spy.nd_b()
    with pytest.raises(AssertionError):
        spy.expect(never=["nd_b"])
    assert spy.nd_c() == 1 and spy.nd_c_splits() == 1
    spy.expect(ran=["nd_c_splits"], never=["nd_c"])  # a refused launch did not run
    with pytest.raises(AssertionError):
        spy.expect(ran=["nd_c"])
