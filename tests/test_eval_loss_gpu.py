"""Held-out evaluation on the GPU: ``nd_ce_loss`` alone against float64, ``ops.lm_head_loss`` on exactly known
logits, ``model.loss_stats`` leaving no trace in the training state, and a training run that evaluation does not
move.  The error rule is ``_oracle64.check`` (fp32 outputs: margin x the error of the fp32 PyTorch twin on the same
inputs, margin 8); ``row_hit`` is exact on the stored logits and has no tolerance."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import resolve_llama_config
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import _ext
from nanodiloco_amd.optim import FlatAdamW

from . import _oracle64 as o64
from ._frames import _ints, assert_frame_intact, framed_flat

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
IGN = -100
REPORT = {}


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    torch.manual_seed(0)
    yield
    ops.set_backend("auto")


@pytest.fixture(scope="module", autouse=True)
def _slack_report():
    yield
    for k in sorted(REPORT):
        print(f"\n[slack] {k}: needs margin {REPORT[k]:.3g} (allowed {o64.MARGIN})", end="")
    print()


def chk(out, ref64, twin32, name):
    o64.check(out, ref64, twin32, margin=o64.MARGIN, name=name, report=REPORT)


def S():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------ the kernel alone
CE_V = [8, 100, 1000, 1001, 8192, 8200, 32000, 32768, 32776, 50257]


def _ce_inputs(V, dt):
    """18 rows: three logit patterns (4 randn; one +60 among -60; constant) x six targets (0, V - 1, a column of
    the last partial chunk, a middle column, ignore_index, the row's arg-max)."""
    n = 18
    x = 4 * torch.randn(n, V, device=DEV)
    peak = [V - 1, 0, max(0, V - 3), V // 2, V // 3, (V - 1) // 8 * 8]
    for k, r in enumerate(range(1, n, 3)):
        x[r] = -60.0
        x[r, peak[k]] = 60.0
    x[2::3] = 1.5
    x = x.to(dt)
    tgt = torch.empty(n, dtype=torch.long, device=DEV)
    kinds = [0, V - 1, max(0, V - 3), V // 2, IGN, None]
    for r in range(n):
        k = kinds[(r // 3 + r % 3) % 6]  # every pattern meets every kind of target
        tgt[r] = int(x[r].float().argmax()) if k is None else k
    return x, tgt


def _twin(x32, tgt):
    """The fp32 PyTorch computation: (lse, row_loss)."""
    lse = torch.logsumexp(x32, dim=-1)
    ok = tgt != IGN
    safe = torch.where(ok, tgt, torch.zeros_like(tgt))
    return lse, torch.where(ok, lse - x32.gather(1, safe[:, None])[:, 0], torch.zeros_like(lse))


def _hit_ref(x, tgt):
    """valid & (x[target] == max x), on the stored values."""
    ok = tgt != IGN
    safe = torch.where(ok, tgt, torch.zeros_like(tgt))
    xf = x.float()
    return ok & (xf.gather(1, safe[:, None])[:, 0] == xf.max(-1).values)


def _run(x, tgt, full=True, pad=64, n=None):
    """nd_ce_loss on framed operands; the logits must come back bit for bit, every frame intact."""
    rows, V = x.shape
    n = rows if n is None else n
    big, flat = framed_flat(rows * V, x.dtype, pad=pad)
    logits = flat.view(rows, V)
    logits.copy_(x)
    rbig, loss = framed_flat(rows, F32)
    lbig, lse = framed_flat(rows, F32)
    hbig, hit = framed_flat(rows, torch.uint8)
    rc = _ext.lib().nd_ce_loss(logits.data_ptr(), _ext.dtcode(x), tgt.data_ptr(), n, V, IGN, loss.data_ptr(),
                               lse.data_ptr() if full else 0, hit.data_ptr() if full else 0, S())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(_ints(logits), _ints(x)), "the logits were written"
    assert_frame_intact(big, flat)
    wrote = n > 0
    assert_frame_intact(rbig, loss if wrote else None)
    assert_frame_intact(lbig, lse if (full and wrote) else None)
    assert_frame_intact(hbig, hit if (full and wrote) else None)
    return loss, lse, hit


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("V", CE_V)
def test_ce_loss_kernel_alone(V, dt):
    """row_loss and lse_out on every row against float64 (vector path where V % 8 == 0, scalar path otherwise),
    row_hit exact, ignored rows exactly 0, const logits, null outputs, repeatability, n = 0, a NaN row."""
    x, tgt = _ce_inputs(V, dt)
    # one more valid row with a NaN logit, away from its target
    extra = 4 * torch.randn(1, V, device=DEV)
    extra[0, V // 2] = float("nan")
    xn = torch.cat([x, extra.to(dt)])
    tn = torch.cat([tgt, torch.zeros(1, dtype=torch.long, device=DEV)])
    lse64, loss64, _ = o64.ce_rows(x, tgt, 1.0)
    lse32, loss32 = _twin(x.float(), tgt)
    loss, lse, hit = _run(xn, tn)
    name = ("ce_loss_vec" if V % 8 == 0 else "ce_loss_scalar") + ("_bf16" if dt == BF16 else "_f32")
    chk(lse[:18], lse64, lse32, name + ".lse")
    chk(loss[:18], loss64, loss32, name + ".row_loss")
    assert torch.equal(hit[:18].bool(), _hit_ref(x, tgt))
    assert int(hit[:18].sum()) >= 3  # the arg-max targets and the constant rows (ties count)
    ign = tgt == IGN
    assert bool(ign.any()) and not bool(loss[:18][ign].any()) and not bool(hit[:18][ign].any())
    assert bool(torch.isnan(loss[18])) and int(hit[18]) == 0 and bool(torch.isnan(lse[18]))
    # without the optional outputs: the same row_loss bits
    loss_b, _, _ = _run(xn, tn, full=False)
    assert torch.equal(_ints(loss_b), _ints(loss))
    # again: the same bits
    loss_c, lse_c, hit_c = _run(xn, tn)
    assert torch.equal(_ints(loss_c), _ints(loss)) and torch.equal(_ints(lse_c), _ints(lse))
    assert torch.equal(hit_c, hit)
    # n = 0: returns 0, writes nothing
    _run(xn, tn, n=0)
    # every row ignored
    loss_d, _, hit_d = _run(x, torch.full_like(tgt, IGN))
    assert not bool(loss_d.any()) and not bool(hit_d.any())


@pytest.mark.parametrize("dt", [BF16, F32])
def test_ce_loss_unaligned_base(dt):
    """V % 8 == 0 on a base that is not 16-byte aligned: the scalar path, the same numbers."""
    V = 1000
    x, tgt = _ce_inputs(V, dt)
    a = _run(x, tgt)
    b = _run(x, tgt, pad=3)
    lse64, loss64, _ = o64.ce_rows(x, tgt, 1.0)
    lse32, loss32 = _twin(x.float(), tgt)
    chk(b[0], loss64, loss32, "ce_loss_unaligned.row_loss")
    chk(b[1], lse64, lse32, "ce_loss_unaligned.lse")
    assert torch.equal(a[2], b[2])


def test_ce_loss_refuses_bad_arguments():
    x, tgt = _ce_inputs(8, F32)
    loss = torch.zeros(18, device=DEV)
    L = _ext.lib()
    assert L.nd_ce_loss(x.data_ptr(), 7, tgt.data_ptr(), 18, 8, IGN, loss.data_ptr(), 0, 0, S()) != 0
    assert L.nd_ce_loss(x.data_ptr(), 0, tgt.data_ptr(), 18, 0, IGN, loss.data_ptr(), 0, 0, S()) != 0
    assert L.nd_ce_loss(x.data_ptr(), 0, tgt.data_ptr(), 18, 8, IGN, 0, 0, 0, S()) != 0
    torch.cuda.synchronize()
    assert not bool(loss.any())


# ------------------------------------------------------------------------------------------ lm_head_loss, exact logits
def _exact_head(V, n=600, d=256):
    """y rows hold one +1 and one -1, W is in multiples of 1/8 with |w| <= 8: every logit is W[v, i] - W[v, j], a
    multiple of 1/8 of magnitude <= 16 (8 significant bits) -- exact in bf16 whatever the GEMM's summation order,
    so the float64 logits are known without trusting any GEMM."""
    g = torch.Generator().manual_seed(V)
    i = torch.randint(0, d, (n,), generator=g)
    j = (i + 1 + torch.randint(0, d - 1, (n,), generator=g)) % d
    y = torch.zeros(n, d)
    y[torch.arange(n), i] = 1.0
    y[torch.arange(n), j] = -1.0
    W = torch.randint(-64, 65, (V, d), generator=g).float() / 8
    logits64 = y.double() @ W.double().t()
    assert torch.equal(logits64.bfloat16().double(), logits64)
    tgt = torch.randint(0, V, (n,), generator=g)
    tgt[::5] = logits64.argmax(-1)[::5]  # hits (the coarse grid also gives tied maxima)
    tgt[7::11] = IGN
    tgt[256:512] = IGN  # with chunk_rows = 256: a chunk whose rows are all ignored
    return y.bfloat16().to(DEV), W.bfloat16().to(DEV), tgt.to(DEV), logits64.to(DEV)


@pytest.mark.parametrize("V", [1000, 8200])
def test_lm_head_loss_exact_logits(V):
    y, W, tgt, x64 = _exact_head(V)
    _, loss64, _ = o64.ce_rows(x64, tgt, 1.0)
    _, loss32 = _twin(x64.float(), tgt)
    hit_ref = _hit_ref(x64, tgt)
    assert 40 < int(hit_ref.sum()) < 300
    loss, hit = ops.lm_head_loss(y, W, tgt, chunk_rows=256)  # two full chunks and a ragged one
    assert loss.dtype == F32 and hit.dtype == torch.bool and loss.shape == hit.shape == (600,)
    chk(loss, loss64, loss32, f"lm_head_loss_V{V}.row_loss")
    assert torch.equal(hit, hit_ref)
    assert not bool(loss[tgt == IGN].any())
    one = ops.lm_head_loss(y, W, tgt)  # one chunk: the same rows
    assert torch.equal(one[0], loss) and torch.equal(one[1], hit)
    ops.set_backend("torch")
    try:
        tl, th = ops.lm_head_loss(y, W, tgt, chunk_rows=256)
    finally:
        ops.set_backend("hip")
    assert torch.equal(th, hit_ref)
    chk(tl, loss64, loss32, f"lm_head_loss_V{V}.twin_row_loss")


# ------------------------------------------------------------------------------------------ loss_stats leaves no trace
def _snapshot(m):
    s = {"grad": m.store.grad.clone(), "master": m.store.master.clone(), "shadow": m.store.shadow.clone()}
    if m.fp8 is not None:
        r = m.fp8.recipe
        s.update(amax=r.amax.clone(), hist=r.hist.clone(), scale=r.scale.clone(), inv=r.inv.clone(),
                 ready=list(r.ready), pos=r.pos, n=r.n,
                 wver={k: w.version for k, w in m.fp8.weights.items()})
    return s


def _same(a, b):
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(_ints(a[k].reshape(-1)), _ints(b[k].reshape(-1))), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("case", ["bf16", "residual_bf16", "fp8"])
def test_loss_stats_leaves_no_trace(case):
    cfg = resolve_llama_config("llama_tiny.json")
    B, T = 2, 64
    kw = dict(residual_dtype=BF16) if case == "residual_bf16" else dict(fp8=True) if case == "fp8" else {}
    m = LlamaForCausalLM(cfg, DEV, BF16, **kw).init_weights(4)
    opt = FlatAdamW(m.store, lr=1e-3)
    ids = torch.randint(0, cfg.vocab_size, (B, T), device=DEV)
    # a training step and a half first: optimizer-updated weights, a live grad buffer, fp8 history and amax partials
    for i in range(2):
        m(ids, labels=ids).loss.backward()
        if i == 0:
            opt.step()
            opt.zero_grad()
            if m.fp8 is not None:
                m.fp8.recipe.update()
    torch.cuda.synchronize()
    if m.fp8 is not None:
        assert any(m.fp8.recipe.ready) and bool(m.fp8.recipe.amax.any())
    assert bool(m.store.grad.any())
    before = _snapshot(m)
    ev = torch.randint(0, cfg.vocab_size, (B, T), device=DEV)
    for training in (True, False):
        m.training = training
        a = m.loss_stats(ev, ev)
        b = m.loss_stats(ev, ev)
        assert m.training is training
        assert a.dtype == torch.float64 and a.device.type == "cuda" and a.shape == (3,)
        assert torch.equal(a, b)
    m.train()
    torch.cuda.synchronize()
    _same(before, _snapshot(m))
    assert m.proj.lm_y8 is None
    s = a.tolist()
    assert s[1] == B * (T - 1) and 0 <= s[2] <= s[1] and s[0] / s[1] > 1.0
    # left-padded batch: the 9 pads carry label -100; position t predicts label t + 1, so labels 1..8 ignore 8
    # targets (label 0 is nobody's target) on top of the last position of each sequence
    mask = torch.ones(B, T, dtype=torch.long, device=DEV)
    mask[0, :9] = 0
    labels = torch.where(mask.bool(), ev, torch.full_like(ev, IGN))
    s = m.loss_stats(ev, labels, attention_mask=mask).tolist()
    assert s[1] == B * (T - 1) - 8 and s[0] == s[0]
    # packed documents
    md = LlamaForCausalLM(cfg, DEV, BF16, doc_mask=True, **kw).init_weights(4)
    evd = ev.clone()
    evd[:, 20] = cfg.eos_token_id
    s = md.loss_stats(evd, evd).tolist()
    assert s[1] == B * (T - 1) and s[0] == s[0]


# ------------------------------------------------------------------------------------------ evaluation does not move training
@pytest.mark.parametrize("fp8", [False, True])
def test_evaluation_does_not_move_training(fp8):
    from nanodiloco_amd.trainer import TrainArgs, Trainer

    def run(**kw):
        t = Trainer(TrainArgs(llama_config_file="configs/llama_tiny.json", batch_size=8, per_device_batch_size=4,
                              seq_length=64, warmup_steps=2, total_steps=6, inner_steps=3, wandb="off",
                              data="synthetic", deterministic=True, fp8=fp8, **kw))
        assert (t.graphed is not None) == (not fp8)  # --hip-graph auto is on for the bf16 run at this size
        out = t.train()
        torch.cuda.synchronize()
        return t.model.store.master.clone(), out

    try:
        p0, o0 = run()
        p1, o1 = run(eval_every=2, eval_batches=2)
    finally:
        ops.set_deterministic(False)
    assert "final_eval_loss" not in o0 and o1["final_eval_loss"] == o1["final_eval_loss"]
    assert torch.equal(_ints(p0), _ints(p1))
