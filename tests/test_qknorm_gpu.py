"""QK-norm on the MI355X: the three kernels of csrc/qk_norm.hip at their edges against the float64 oracle
(tests/_qknorm_oracle.py), the bitwise contracts of the fused forward, the whole model against the float64 model
oracle per parameter, generation, --hip-graph and --fp8.

The rule for every oracle comparison is ``_oracle64.check`` as it stands (half a bf16 ulp relative for bf16 outputs
plus 8 x the fp32 PyTorch twin's own error); the twin is ``ops.reference`` in fp32 on the same inputs, or, for the
model, the same model on stock PyTorch ops -- never the code under test.  Every case prints its figures before it
asserts; docs/PARITY.md (QK-norm) records them.
"""
import importlib
import json

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import _ext, reference as ref

from . import _model_oracle as mo
from . import _oracle64 as o64
from . import _qknorm_oracle as qo
from .test_model_grads_gpu import BETA_BOUND, LOSS_FLOOR, MARGIN

qkn = importlib.import_module("nanodiloco_amd.ops.qk_norm")  # ``ops.qk_norm`` itself is the function
attn = importlib.import_module("nanodiloco_amd.ops.attention")

pytestmark = pytest.mark.gpu

DEV, BF16, F32, EPS = "cuda", torch.bfloat16, torch.float32, 1e-5
NEW = ("nd_qk_norm", "nd_qk_norm_rope_fwd", "nd_qk_norm_bwd")
ROPE_ELSEWHERE = ("nd_gemm_pp_rope", "nd_gemm_pp_rope_f8", "nd_rope_inplace")
REPORT = {}


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    det = ops.deterministic()
    ops.set_backend("hip")
    yield
    ops.set_backend("auto")
    ops.set_deterministic(det)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------ kernel edges
HDS = (32, 64, 128)
HEADS = ((1, 1), (2, 1), (6, 3), (4, 2))  # heads per row that do and do not fill a wave: waves straddle rows
BTS = ((1, 1), (3, 5), (2, 67), (1, 2049))  # one row; row % T wraps; rows no multiple of a block; table index > 2048
_TABLES = {}


def _tables(T, hd):
    if (T, hd) not in _TABLES:
        c, s = ref.rope_tables(T, hd, 10000.0, None, device="cpu")
        _TABLES[(T, hd)] = (c.to(DEV).contiguous(), s.to(DEV).contiguous())
    return _TABLES[(T, hd)]


def _inputs(hd, nh, nkv, B, T, dtype):
    """Spiked rows with |x| <= 1e4 and one all-zero head, weights in [0.5, 1.5] with one exact 0, a spiked gradient."""
    torch.manual_seed(hd * 1000 + nh * 100 + nkv * 10 + B + T)
    N, W = B * T, (nh + 2 * nkv) * hd
    x = o64.spiked(N, W, DEV, scale=1e3)
    assert float(x.abs().max()) <= 1e4
    zr, zh = N // 2, nh + nkv - 1  # the last k head of a middle row
    x[zr, zh * hd:(zh + 1) * hd] = 0
    wq = 0.5 + torch.rand(hd, device=DEV)
    wk = 0.5 + torch.rand(hd, device=DEV)
    wq[hd // 2 + 1] = 0.0
    dy = o64.spiked(N, W, DEV, scale=1.0, start=3)
    return x.to(dtype), wq, wk, dy.to(dtype), (zr, zh)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,T", BTS, ids=[f"{b}x{t}" for b, t in BTS])
@pytest.mark.parametrize("nh,nkv", HEADS, ids=[f"h{a}k{b}" for a, b in HEADS])
@pytest.mark.parametrize("hd", HDS)
def test_kernels_at_their_edges(hd, nh, nkv, B, T, dtype):
    x, wq, wk, dy, (zr, zh) = _inputs(hd, nh, nkv, B, T, dtype)
    N, nqk = B * T, (nh + nkv) * hd
    cos, sin = _tables(T, hd)
    tag = "bf16" if dtype == BF16 else "fp32"
    r64 = qo.qk_norm(x, wq, wk, nh, nkv, hd, EPS, dy=dy)
    xf, dyf = x.float(), dy.float()
    twin_y = ref.qk_norm(xf, wq, wk, nh, nkv, hd, EPS)
    twin_dx, twin_dwq, twin_dwk = ref.qk_norm_backward(dyf, xf, wq, wk, nh, nkv, hd, EPS)
    heads = xf[:, :nqk].reshape(N, nh + nkv, hd)
    twin_rstd = torch.rsqrt(heads.pow(2).mean(-1) + EPS)

    # 1. the norm alone, every element; v untouched
    y = ops.qk_norm(x.clone(), wq, wk, nh, nkv, hd, EPS)
    assert y.dtype == dtype
    o64.check(y, r64["y"], twin_y, name=f"qk_norm.y.{tag}", report=REPORT, note=f"hd{hd} h{nh}k{nkv} {B}x{T}")
    assert _same(y[:, nqk:], x[:, nqk:])
    assert not bool(y[zr, zh * hd:(zh + 1) * hd].any())  # the all-zero head: rstd = rsqrt(eps), output 0

    # 2. the fused forward: bitwise the composition, v bitwise the input, rstd by the fp32 rule
    fused = x.clone()
    rstd, raw = qkn.qk_norm_rope_fwd_launch(fused, wq, wk, cos, sin, T, nh, nkv, hd, EPS, save=True)
    comp = y.clone()
    attn._rope(comp, cos, sin, B, T, nh, nkv, hd, inverse=False)
    assert _same(fused, comp), f"fused != rope(qk_norm): {int((_bits(fused) != _bits(comp)).sum())} elements differ"
    assert _same(fused[:, nqk:], x[:, nqk:])
    assert _same(raw, x[:, :nqk])
    o64.check(rstd, r64["rstd"], twin_rstd, name="qk_norm.rstd", report=REPORT, note=f"hd{hd} h{nh}k{nkv} {B}x{T}")
    assert abs(float(rstd[zr, zh]) - EPS ** -0.5) <= 1e-3 * EPS ** -0.5
    out, rotated = ops.qk_norm_rope(x, wq, wk, None, None, cos, sin, T, nh, nkv, hd, EPS)  # the op, out of place
    assert rotated is True and _same(out, fused) and out.data_ptr() != x.data_ptr()

    # 3. the backward: dx every element, dw accumulated into a non-zero buffer, v gradient untouched, repeatable
    start_q = ((torch.arange(hd, device=DEV) % 5).float() - 2.0) * 0.25
    start_k = ((torch.arange(hd, device=DEV) % 3).float() - 1.0) * 0.5
    runs = []
    for _ in range(2):
        gwq, gwk, d = start_q.clone(), start_k.clone(), dy.clone()
        qkn.qk_norm_bwd_launch(d, raw, rstd, wq, wk, gwq, gwk, nh, nkv, hd)
        runs.append((d, gwq, gwk))
    dx, gwq, gwk = runs[0]
    note = f"hd{hd} h{nh}k{nkv} {B}x{T}"
    o64.check(dx, r64["dx"], twin_dx, name=f"qk_norm.dx.{tag}", report=REPORT, note=note)
    assert bool(torch.isfinite(dx.float()).all())
    assert _same(dx[:, nqk:], dy[:, nqk:])
    o64.check(gwq, start_q.double() + r64["dwq"], start_q + twin_dwq, name=f"qk_norm.dwq.{tag}", report=REPORT, note=note)
    o64.check(gwk, start_k.double() + r64["dwk"], start_k + twin_dwk, name=f"qk_norm.dwk.{tag}", report=REPORT, note=note)
    for a, b in zip(runs[0], runs[1]):
        assert _same(a, b)
    print(f"[qk-norm] hd{hd} h{nh}k{nkv} {B}x{T} {tag}: margins needed so far "
          + ", ".join(f"{k} {v:.2f}" for k, v in sorted(REPORT.items())))


def test_autograd_function_routes_the_kernels():
    """``ops.qk_norm_rope`` through autograd: the gradient and the accumulated weight gradients are what the launchers
    give, the caller's tensors are not overwritten (inplace=False)."""
    hd, nh, nkv, B, T = 64, 4, 2, 2, 33
    x, wq, wk, dy, _ = _inputs(hd, nh, nkv, B, T, BF16)
    cos, sin = _tables(T, hd)
    x0, dy0 = x.clone(), dy.clone()
    gwq, gwk = torch.zeros(hd, device=DEV), torch.zeros(hd, device=DEV)
    xin = x.clone().requires_grad_(True)
    with mo.spying() as spy:
        out, rotated = ops.qk_norm_rope(xin, wq, wk, gwq, gwk, cos, sin, T, nh, nkv, hd, EPS)
        out.backward(dy)
    assert rotated and spy.ran("nd_qk_norm_rope_fwd") == 1 and spy.ran("nd_qk_norm_bwd") == 1
    assert _same(xin.detach(), x0) and _same(dy, dy0)
    f = x.clone()
    rstd, raw = qkn.qk_norm_rope_fwd_launch(f, wq, wk, cos, sin, T, nh, nkv, hd, EPS, save=True)
    g2q, g2k, d = torch.zeros(hd, device=DEV), torch.zeros(hd, device=DEV), dy.clone()
    qkn.qk_norm_bwd_launch(d, raw, rstd, wq, wk, g2q, g2k, nh, nkv, hd)
    assert _same(out.detach(), f) and _same(xin.grad, d) and _same(gwq, g2q) and _same(gwk, g2k)


def test_unsupported_head_dim_is_refused():
    x = torch.zeros(4, 3 * 48, dtype=BF16, device=DEV)
    w = torch.ones(48, device=DEV)
    with pytest.raises(ValueError, match="head_dim 48"):
        ops.qk_norm(x, w, w, 1, 1, 48, EPS)


def test_attention_takes_the_fused_output_as_rotated():
    """``attention(fused, rotated=True)`` is bitwise ``attention(qk_norm(x), rotated=False)``: the fused forward hands
    the attention kernels the q|k they would have rotated themselves."""
    hd, nh, nkv, B, T = 32, 4, 2, 2, 64
    torch.manual_seed(5)
    x = torch.randn(B * T, (nh + 2 * nkv) * hd, device=DEV).to(BF16)
    wq, wk = 0.5 + torch.rand(hd, device=DEV), 0.5 + torch.rand(hd, device=DEV)
    cos, sin = _tables(T, hd)
    fused, rotated = ops.qk_norm_rope(x, wq, wk, None, None, cos, sin, T, nh, nkv, hd, EPS)
    a = ops.attention(fused, cos, sin, B, T, nh, nkv, hd, rotated=rotated, inplace=True)
    b = ops.attention(ops.qk_norm(x.clone(), wq, wk, nh, nkv, hd, EPS), cos, sin, B, T, nh, nkv, hd, rotated=False,
                      inplace=False)
    assert bool(a.any()) and _same(a, b)


# ------------------------------------------------------------------------------------------ the model
MODELS = {
    "hd32": dict(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_key_value_heads=2),
    "hd64": dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=4),
    "hd128": dict(hidden_size=256, intermediate_size=512, num_attention_heads=2, num_key_value_heads=1),
}
L, T_MODEL, V = 2, 64, 512


def _config(name, qk_norm=True):
    return LlamaConfig.from_dict(dict(MODELS[name], num_hidden_layers=L, vocab_size=V, rms_norm_eps=EPS,
                                      max_position_embeddings=256, **({"qk_norm": True} if qk_norm else {})))


def _build(name, backend, qk_norm=True, seed=3, **kw):
    ops.set_backend(backend)
    m = LlamaForCausalLM(_config(name, qk_norm), DEV, BF16, **kw).init_weights(seed)
    if qk_norm:  # ones would hide a q / k weight mix-up
        g = torch.Generator().manual_seed(11)
        for n in m.store.names:
            if "q_norm" in n or "k_norm" in n:
                v = m.store.master_view(n)
                v.copy_((0.5 + torch.rand(v.shape, generator=g)).to(DEV))
        m.store.sync_shadow()
    return m


def _batch(kind, c, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    B = 3 if kind == "left" else 2
    ids = torch.randint(3, c.vocab_size, (B, T_MODEL), generator=g)
    mask = None
    if kind == "left":
        mask = torch.ones(B, T_MODEL, dtype=torch.long)
        for b, npad in enumerate([0, 5, 11]):
            mask[b, :npad] = 0
        ids[mask == 0] = 2
    else:
        for b in range(B):
            ids[b, 17 + 13 * b] = c.eos_token_id
            ids[b, 40] = c.eos_token_id
    labels = ids.clone()
    labels[0, 20:27] = -100
    if mask is not None:
        labels[mask == 0] = -100
    return ids.to(DEV), labels.to(DEV), mask.to(DEV) if mask is not None else None


def _step(m, batch):
    ids, labels, mask = batch
    out = m(ids, labels=labels, attention_mask=mask)
    out.loss.backward()
    torch.cuda.synchronize()
    return float(out.loss.detach()), mo.model_grads(m)


@pytest.mark.parametrize("kind", ["left", "doc"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_gradients_against_float64(name, kind):
    c = _config(name)
    doc = kind == "doc"
    batch = _batch(kind, c)
    l_twin, g_twin = _step(_build(name, "torch", doc_mask=doc), batch)
    with mo.spying() as spy:
        m = _build(name, "hip", doc_mask=doc)
        loss, grads = _step(m, batch)
    ids, labels, mask = batch
    l64, g64 = qo.grads64(m, ids, labels, kstart=mo.key_start(mask) if mask is not None else None, doc_mask=doc)
    case = f"qk_norm/{name}/{kind}"
    report, err = {}, None
    try:
        mo.check_grads(grads, g64, g_twin, MARGIN, BETA_BOUND, report, case)
    except AssertionError as e:
        err = e
    worst = max(report.items(), key=lambda kv: (kv[1]["margin"] != kv[1]["margin"], kv[1]["margin"]))
    wb = max(report.items(), key=lambda kv: kv[1]["beta"])
    print(f"[qk-norm model] {case}: margin {worst[1]['margin']:.2f} ({worst[0]}), |beta| {wb[1]['beta']:.2e} "
          f"({wb[0]}), q_norm margin {report['model.layers.self_attn.q_norm.weight']['margin']:.2f}, k_norm margin "
          f"{report['model.layers.self_attn.k_norm.weight']['margin']:.2f}, loss err {abs(loss - float(l64)):.2e}, twin "
          f"loss err {abs(l_twin - float(l64)):.2e}; launchers {dict(sorted(spy.calls.items()))}")
    if err is not None:
        raise err
    mo.check_loss(loss, l64, l_twin, MARGIN, LOSS_FLOOR, case)
    assert spy.ran("nd_qk_norm_rope_fwd") == L and spy.ran("nd_qk_norm_bwd") == L, dict(spy.calls)
    spy.expect(never=ROPE_ELSEWHERE + ("nd_qk_norm",), case=case)
    assert not spy.refused["nd_qk_norm_rope_fwd"] and not spy.refused["nd_qk_norm_bwd"]


def test_checkpointed_and_hooked_backward_is_the_plain_one():
    """Activation checkpointing recomputes the in-place forward; the layer hook still fires once per layer after the
    layer's gradients (q_norm / k_norm among them) are final."""
    ops.set_deterministic(True)
    c = _config("hd64")
    batch = _batch("left", c)
    _, g0 = _step(_build("hd64", "hip"), batch)
    m = _build("hd64", "hip", activation_checkpointing=True)
    fired, seen = [], {}

    def hook(i):
        fired.append(i)
        seen[i] = m.store.grad_view(f"model.layers.{i}.self_attn.k_norm.weight").clone()

    m.layer_hook = hook
    _, g1 = _step(m, batch)
    assert fired == [1, 0]
    for n in g0:
        assert _same(g0[n], g1[n]), n
    for i in range(L):
        assert bool(seen[i].any()) and _same(seen[i], g1[f"model.layers.{i}.self_attn.k_norm.weight"])


def test_default_path_launches_nothing_new_and_repeats_bitwise():
    ops.set_deterministic(True)
    c = _config("hd64", qk_norm=False)
    batch = _batch("left", c)
    with mo.spying() as spy:
        l0, g0 = _step(_build("hd64", "hip", qk_norm=False), batch)
    spy.expect(ran=["nd_gemm_pp_rope"], at_least=L, never=NEW, case="default path")
    l1, g1 = _step(_build("hd64", "hip", qk_norm=False), batch)
    assert l0 == l1 and set(g0) == set(g1) and not any("q_norm" in n or "k_norm" in n for n in g0)
    for n in g0:
        assert _same(g0[n], g1[n]), n


# ------------------------------------------------------------------------------------------ generation
N_NEW = 13


def _gen_model(memorise=None):
    c = LlamaConfig.from_dict(dict(MODELS["hd32"], num_hidden_layers=L, vocab_size=1024, rms_norm_eps=EPS,
                                   max_position_embeddings=512, qk_norm=True))
    ops.set_backend("hip")
    m = LlamaForCausalLM(c, DEV, BF16).init_weights(7)
    g = torch.Generator().manual_seed(11)
    for n in m.store.names:
        if "q_norm" in n or "k_norm" in n:
            v = m.store.master_view(n)
            v.copy_((0.5 + torch.rand(v.shape, generator=g)).to(DEV))
    m.store.sync_shadow()
    if memorise is not None:
        from nanodiloco_amd.optim import FlatAdamW
        ids, mask = memorise
        labels = ids.masked_fill(mask == 0, -100)
        opt = FlatAdamW(m.store, lr=1e-2)
        for _ in range(60):
            m(ids, labels=labels, attention_mask=mask).loss.backward()
            opt.step()
            m.store.zero_grad()
    return m


def _sequences(c, B=3, T=9, n=N_NEW):
    """Left-padded rows of T + n tokens (6, 0 and 4 pads) and their attention mask."""
    g = torch.Generator().manual_seed(12)
    ids = torch.randint(3, c.vocab_size, (B, T + n), generator=g).to(DEV)
    mask = torch.ones(B, T + n, dtype=torch.long, device=DEV)
    mask[0, :6] = 0
    mask[2, :4] = 0
    return ids, mask


def test_generation_cache_and_graph():
    """Greedy generation with the KV cache, eager and graphed, and without it.  The cached and the recomputed logits
    differ by bf16 rounding (two attention kernels, as tests/test_generate_gpu.py says of the model without QK-norm),
    and a freshly initialised model's 1024 logits are nearly flat: the gap between its top two is a small fraction of
    their spread, the order of that rounding, so over 3 x 13 tokens one flipped argmax is to be expected whatever the
    code does (a first version of this test on such a model: 31 of 39 equal, one row parting at its ninth token).
    The model therefore first memorises the three sequences (60 AdamW steps, through the QK-norm backward) and
    continues their first 9 tokens: its choices are decisive, and the tokens must be equal."""
    seq, full_mask = _sequences(LlamaConfig.from_dict(dict(MODELS["hd32"], vocab_size=1024)))
    m = _gen_model(memorise=(seq, full_mask))
    ids, mask = seq[:, :9].contiguous(), full_mask[:, :9].contiguous()
    kw = dict(max_new_tokens=N_NEW, eos_token_id=None, return_logits=True)
    with mo.spying() as spy:
        a, la = m.generate(ids, mask, hip_graph=False, **kw)
    assert spy.ran("nd_qk_norm_rope_fwd") == L and spy.ran("nd_qk_norm") == L * 12, dict(spy.calls)
    spy.expect(never=ROPE_ELSEWHERE + ("nd_qk_norm_bwd",), case="generate")
    b, lb = m.generate(ids, mask, hip_graph=True, **kw)
    assert torch.equal(a, b) and torch.equal(la.view(torch.int32), lb.view(torch.int32))  # graphed == eager, bitwise
    c, lc = m.generate(ids, mask, use_cache=False, **kw)
    print(f"[qk-norm generate] cached vs recomputed logits: max |diff| {float((la - lc).abs().max()):.3e}; tokens "
          f"{a[:, ids.shape[1]:].tolist()} vs {c[:, ids.shape[1]:].tolist()}")
    top2 = lc.topk(2, dim=-1).values
    print(f"[qk-norm generate] memorised continuation reproduced at {int((a[:, 9:] == seq[:, 9:]).sum())} of "
          f"{a[:, 9:].numel()} positions; smallest top-2 gap of the recomputed logits "
          f"{float((top2[..., 0] - top2[..., 1]).min()):.3f}")
    assert torch.equal(a, c)  # greedy tokens with the cache == without it


def test_decode_step_stores_the_key_a_prefill_stores():
    """The rounding contract where it matters: for the same projection row, the key a decode step appends at slot T
    (``qk_norm`` in place, then the decode kernel's rotation) is bitwise the key the prefill of T + 1 tokens stores
    there (the fused norm + RoPE forward, then ``cache_fill``); v likewise.  Both start from one projection buffer,
    so that the comparison is of these kernels and not of two GEMM shapes."""
    m = _gen_model()
    c = m.config
    nh, nkv, hd = c.num_attention_heads, c.num_key_value_heads, c.head_dim
    B, T = 3, 37
    torch.manual_seed(3)
    raw = (torch.randn(B, T + 1, (nh + 2 * nkv) * hd, device=DEV) * 3).to(BF16)
    wq = m.store.master_view("model.layers.0.self_attn.q_norm.weight")
    wk = m.store.master_view("model.layers.0.self_attn.k_norm.weight")
    cos, sin = ops.rope_cache(T + 1, hd, c.rope_theta, c.rope_scaling, m.device)
    full = m.new_cache(B, T + 1)
    buf, rotated = ops.qk_norm_rope(raw.view(B * (T + 1), -1), wq, wk, None, None, cos, sin, T + 1, nh, nkv, hd, EPS)
    ops.cache_fill(full, 0, buf, B, T + 1, cos, sin, rotated=rotated)
    step = m.new_cache(B, T + 1)
    step.set_positions([T] * B)
    row = raw[:, T].contiguous()
    ops.qk_norm(row, wq, wk, nh, nkv, hd, EPS)
    ops.attention_decode(row, step, 0, cos, sin)
    torch.cuda.synchronize()
    assert bool(full.k[0][:, :, T].any())
    assert _same(step.k[0][:, :, T], full.k[0][:, :, T])
    assert _same(step.v[0][:, :, T], full.v[0][:, :, T])


# ------------------------------------------------------------------------------------------ trainer
def _train(tmp_path, tag, extra):
    from nanodiloco_amd.main import parse_args
    from nanodiloco_amd.trainer import Trainer
    log = tmp_path / f"{tag}.jsonl"
    args = parse_args(["--llama-config-file", "configs/llama_tiny.json", "--batch-size", "8",
                       "--per-device-batch-size", "4", "--seq-length", "64", "--total-steps", "3", "--inner-steps", "3",
                       "--warmup-steps", "1", "--lr", "3e-3", "--wandb", "off", "--data", "synthetic", "--qk-norm",
                       "--deterministic", "--log-file", str(log), "--log-every", "1"] + extra)
    t = Trainer(args)
    t.train()
    torch.cuda.synchronize()
    return t, [json.loads(line)["loss"] for line in open(log) if "loss" in json.loads(line)]


def test_hip_graph_on_equals_off(tmp_path):
    on, l_on = _train(tmp_path, "on", ["--hip-graph", "on"])
    assert on.graphed is not None and on.graphed.graph is not None and on.model.config.qk_norm
    off, l_off = _train(tmp_path, "off", ["--hip-graph", "off"])
    assert off.graphed is None
    print(f"[qk-norm] --hip-graph on {l_on} off {l_off}")
    assert len(l_on) == 3 and l_on == l_off


def test_fp8_composes():
    """--fp8 with QK-norm: the non-fused fp8 q|k|v GEMM, the norm kernels on its bf16 output.  One step on the smallest
    shape the fp8 GEMMs take."""
    from nanodiloco_amd.ops.gemm import pp_f8_supported
    c = _config("hd32")  # K = 128: the smallest the fp8 GEMM takes
    m = _build("hd32", "hip", fp8=True)
    ids = torch.randint(3, V, (2, 64), device=DEV)
    assert not pp_f8_supported(torch.empty(ids.numel(), 64, dtype=torch.float8_e4m3fn, device=DEV),
                               torch.empty(c.q_size + 2 * c.kv_size, 64, dtype=torch.float8_e4m3fn, device=DEV))
    assert pp_f8_supported(torch.empty(ids.numel(), c.hidden_size, dtype=torch.float8_e4m3fn, device=DEV),
                           torch.empty(c.q_size + 2 * c.kv_size, c.hidden_size, dtype=torch.float8_e4m3fn, device=DEV))
    with mo.spying() as spy:
        out = m(ids, labels=ids)
        out.loss.backward()
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out.loss))
    for i in range(L):
        for k in ("q_norm", "k_norm"):
            g = m.store.grad_view(f"model.layers.{i}.self_attn.{k}.weight")
            assert bool(torch.isfinite(g).all()) and bool(g.any()), (i, k)
    assert spy.ran("nd_qk_norm_rope_fwd") == L and spy.ran("nd_qk_norm_bwd") == L and spy.ran("nd_gemm_pp_f8") >= L
    spy.expect(never=ROPE_ELSEWHERE, case="fp8")
