"""Muon inner optimizer on the GPU: AdamW over a span table (csrc/muon.hip) bit for bit against ``nd_adamw_step``;
``FlatMuon`` under the PyTorch backend against a float64 oracle (judged by the test's own bf16-rounding twin) and
against ``FlatAdamW`` on the spans Muon does not own; the refusal under the HIP backend; and the trainer, whose
default optimizer must leave the bits of ``FlatAdamW`` driven directly."""
import math

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models.llama import LlamaForCausalLM
from nanodiloco_amd.optim import FlatAdamW, FlatMuon

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
NS = (3.4445, -4.7750, 2.0315)
MUON_SUFFIXES = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "o_proj.weight", "gate_proj.weight",
                 "up_proj.weight", "down_proj.weight")


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    yield
    ops.set_backend("auto")


def _is_muon(name):
    return ".layers." in name and name.endswith(MUON_SUFFIXES)


# ------------------------------------------------------------------------------------------------ AdamW spans
@pytest.mark.parametrize("bf16_shadow", [False, True])
def test_adamw_spans_bitwise_equal_full_step(bf16_shadow):
    """Spans of lengths 1, 5, 64, 257 and 4096 at 64-aligned starts: a scalar tail alone, a vector plus a tail, whole
    vectors, and more than one block."""
    n = 8192
    starts, lens = [64, 128, 256, 384, 1024], [1, 5, 64, 257, 4096]
    spans = [(s, s + l) for s, l in zip(starts, lens)]
    g = torch.Generator().manual_seed(2)
    master = (torch.randn(n, generator=g) * 0.1).to(DEV)
    grad = torch.randn(n, generator=g).to(DEV)  # norm ~ 90: the clip is active
    m = (torch.randn(n, generator=g) * 0.01).to(DEV)
    v = (torch.rand(n, generator=g) * 1e-3).to(DEV)
    sh = torch.full((n,), 7.0, dtype=BF16, device=DEV) if bf16_shadow else None
    ref = [t.clone() for t in (master, m, v)]
    ref_sh = sh.clone() if bf16_shadow else None
    norm_a, norm_b = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ops.adamw_step(ref[0], grad, ref[1], ref[2], ref_sh, 3, 1e-2, norm_out=norm_a)
    orig = [t.clone() for t in (master, m, v)]
    ops.adamw_step_spans(master, grad, m, v, sh, spans, 3, 1e-2, norm_out=norm_b)
    assert torch.equal(norm_a, norm_b)
    inside = torch.zeros(n, dtype=torch.bool, device=DEV)
    for a, b in spans:
        inside[a:b] = True
    for name, got, want, before in zip(("master", "exp_avg", "exp_avg_sq"), (master, m, v), ref, orig):
        assert torch.equal(got[inside].view(torch.int32), want[inside].view(torch.int32)), name
        assert torch.equal(got[~inside].view(torch.int32), before[~inside].view(torch.int32)), name
        assert not torch.equal(got[inside], before[inside]), name
    if bf16_shadow:
        assert torch.equal(sh[inside].view(torch.int16), ref_sh[inside].view(torch.int16))
        assert bool((sh[~inside] == 7.0).all())


def test_adamw_spans_skip_nonfinite_on_device():
    n = 1024
    master, m, v = torch.ones(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    grad = torch.ones(n, device=DEV)
    grad[900] = float("inf")  # outside the span: the norm is global
    skipped = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.adamw_step_spans(master, grad, m, v, None, [(0, 64)], 1, 1e-3, skip_nonfinite=True, skipped=skipped)
    assert int(skipped) == 1 and bool((master == 1.0).all()) and not m.any() and not v.any()


# ------------------------------------------------------------------------------------------------ FlatMuon
def _model(dtype=BF16):
    cfg = LlamaConfig(vocab_size=256, hidden_size=128, intermediate_size=320, num_attention_heads=4,
                      num_key_value_heads=2, num_hidden_layers=2, max_position_embeddings=64)
    return LlamaForCausalLM(cfg, DEV, dtype).init_weights(0)


def _fill_grad(store, seed, scale=0.05):
    g = torch.Generator().manual_seed(seed)
    store.grad.zero_()
    for n in store.names:
        v = store.grad_view(n)
        v.copy_((torch.randn(v.shape, generator=g) * scale).to(DEV))


def _x0(G):
    """The normalised, packed bf16 X0 of G [batch, m, n], by the PyTorch operations ``newton_schulz`` documents."""
    x = G.float()
    Y = x / (x.flatten(1).norm(dim=1).view(-1, 1, 1) + 1e-7)
    if G.shape[1] > G.shape[2]:
        Y = Y.transpose(1, 2)
    return Y.to(BF16).contiguous()


def _iterate64(x0, steps=5, rounded=False):
    """float64 Newton-Schulz from the bf16 X0; ``rounded``: the twin, one bf16 rounding at every store point."""
    a, b, c = NS
    rb = (lambda t: t.to(BF16).double()) if rounded else (lambda t: t)
    x = x0.double()
    for _ in range(steps):
        A = rb(x @ x.transpose(1, 2))
        B = rb(b * A + c * (A @ A.transpose(1, 2)))
        x = rb(a * x + B @ x)
    return x


def test_flat_muon_refuses_the_hip_backend():
    m = _model()
    opt = FlatMuon(m.store, lr=1e-3)
    _fill_grad(m.store, 1)
    w0 = m.store.master.clone()
    with pytest.raises(NotImplementedError, match="--ops torch"):
        opt.step(1e-3)
    assert torch.equal(m.store.master, w0)
    with pytest.raises(NotImplementedError):
        ops.newton_schulz(torch.randn(2, 16, 32, device=DEV, dtype=BF16))


def test_flat_muon_torch_backend_vs_oracle_and_adamw():
    """d = 128 with GQA (nh 4, nkv 2): k / v are 64 x 128 (m < n) next to the square q / o, gate / up 320 x 128
    take the transpose path.  One step from zero momentum, so U = (1 + mu) coef G is known to the oracle."""
    lr, wd, mu = 2e-3, 0.01, 0.95
    mt, ma = _model(), _model()
    shapes = {mt.store.shapes[n] for n in mt.store.names if _is_muon(n)}
    assert {(128, 128), (64, 128), (320, 128), (128, 320)} <= shapes
    ot, oa = FlatMuon(mt.store, lr=lr, skip_nonfinite=True), FlatAdamW(ma.store, lr=lr)
    w0 = mt.store.master.clone()
    _fill_grad(mt.store, 1)
    ma.store.grad.copy_(mt.store.grad)
    ops.set_backend("torch")
    ot.step(lr)
    oa.step(lr)
    st = mt.store
    assert torch.equal(ot.last_grad_norm, oa.last_grad_norm)
    coef = min(1.0, 1.0 / (float(ot.last_grad_norm) + 1e-6))
    assert coef < 1.0
    for n in st.names:
        a, b = st.range(n)
        if not _is_muon(n):  # AdamW's bits
            for x, y in ((st.master, ma.store.master), (ot.exp_avg, oa.exp_avg), (ot.exp_avg_sq, oa.exp_avg_sq),
                         (st.shadow, ma.store.shadow)):
                assert torch.equal(x[a:b], y[a:b]), n
            continue
        m_, n_ = st.shapes[n]
        G = st.grad_view(n)
        torch.testing.assert_close(ot.exp_avg[a:b].view(m_, n_), coef * G, rtol=1e-6, atol=1e-12)
        assert not ot.exp_avg_sq[a:b].any()
        x0 = _x0(((1.0 + mu) * coef * G.double()).float().unsqueeze(0))
        oracle, twin = _iterate64(x0), _iterate64(x0, rounded=True)
        if m_ > n_:
            oracle, twin = oracle.transpose(1, 2), twin.transpose(1, 2)
        scale = lr * 0.2 * math.sqrt(max(m_, n_))
        w_oracle = w0[a:b].view(m_, n_).double() * (1.0 - lr * wd) - scale * oracle[0]
        # the step's X may differ from the float64 twin's by fp32 summation order, which flips individual bf16
        # roundings: three times the twin's largest element error, scaled as the update is
        bound = scale * 3.0 * float((twin - oracle).abs().max())
        err = float((st.master_view(n).double() - w_oracle).abs().max())
        print(f"{n} [{m_}, {n_}]: |W - oracle| {err:.3e}, bound {bound:.3e}")
        assert err <= bound + 1e-7  # + fp32 rounding of W itself (|W| < 0.2: half an ulp is < 1e-8)
    assert torch.equal(st.shadow.view(torch.int16), st.master.to(BF16).view(torch.int16))
    # a non-finite gradient skips the whole step
    w1, m1, s1 = st.master.clone(), ot.exp_avg.clone(), st.shadow.clone()
    st.grad_view("model.layers.1.mlp.up_proj.weight")[3, 5] = float("nan")
    ot.step(lr)
    assert torch.equal(st.master, w1) and torch.equal(ot.exp_avg, m1) and torch.equal(st.shadow, s1)
    assert int(ot.skipped_steps) == 1


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer(**kw):
    from nanodiloco_amd.trainer import TrainArgs, Trainer

    base = dict(llama_config_file="configs/llama_tiny.json", batch_size=8, per_device_batch_size=4, seq_length=64,
                warmup_steps=1, total_steps=4, inner_steps=4, lr=2e-3, wandb="off", device="cuda", dtype="bf16",
                data="synthetic", log_every=0, deterministic=True)
    base.update(kw)
    t = Trainer(TrainArgs(**base))
    # one fixed micro-batch, repeated: learnable (the synthetic stream is uniform noise) and the same in every run
    ids = torch.randint(0, 512, (4, 64), generator=torch.Generator().manual_seed(11)).to(DEV)
    batch = {"input_ids": ids, "labels": ids}
    t.data = iter(lambda: batch, None)
    t.model.train()
    return t


def test_trainer_muon_needs_torch_ops_on_a_gpu():
    with pytest.raises(ValueError, match="--ops torch"):
        _trainer(inner_optimizer="muon")


def test_trainer_default_optimizer_is_flat_adamw_bits():
    """The default path is the parent's: the trainer's own optimizer and a FlatAdamW built directly here, driven
    by the same trainer steps, leave the same bits."""
    a, b = _trainer(), _trainer()
    assert type(a.diloco.inner_optimizer) is FlatAdamW
    args = a.args
    b.diloco.inner_optimizer = FlatAdamW(b.model.store, lr=args.lr, weight_decay=args.weight_decay,
                                         max_grad_norm=args.max_grad_norm, skip_nonfinite=args.skip_nonfinite)
    la = [float(a.inner_step()) for _ in range(4)]
    lb = [float(b.inner_step()) for _ in range(4)]
    assert la == lb and all(math.isfinite(x) for x in la) and la[-1] < la[0], (la, lb)
    assert torch.equal(a.model.store.master, b.model.store.master)
    assert torch.equal(a.diloco.inner_optimizer.exp_avg, b.diloco.inner_optimizer.exp_avg)
    assert torch.equal(a.diloco.inner_optimizer.exp_avg_sq, b.diloco.inner_optimizer.exp_avg_sq)
