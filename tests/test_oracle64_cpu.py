"""The float64 oracles of tests/_oracle64.py against the project's torch twins (the ``--ops torch`` path of the
same ``ops.*`` call on CPU tensors), edge cases included, and the error rule against the failure it is for:
the proof that the oracles are right before a GPU sees them (T3, no GPU needed)."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import reference as ref

from . import _oracle64 as o64


@pytest.fixture(autouse=True)
def _seed():
    ops.set_backend("auto")
    torch.manual_seed(0)


def close(twin, ref64, tol=2e-5):
    """fp32 twin vs float64 oracle: every element within tol * max|ref| (fp32 rounding and summation order)."""
    ref64 = ref64.double()
    assert twin.shape == ref64.shape
    lim = tol * max(ref64.abs().max().item(), 1e-30)
    err = (twin.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    assert err <= lim, (err, lim)


def bf16_close(twin, ref64, tol=2e-5):
    ref64 = ref64.double()
    err = (twin.double() - ref64).abs() - o64.BF16_HALF_ULP * ref64.abs()
    assert err.max().item() <= tol * ref64.abs().max().item()


# ------------------------------------------------------------------------------------------ the rule itself
def test_spikes_walk_every_column():
    order = o64.spike_columns(1032)
    assert order[:8] == list(range(1024, 1032)) and order[8:11] == [0, 512, 1]
    assert sorted(order) == list(range(1032))
    x = o64.spiked(1032, 1032, "cpu")
    cols = x.abs().argmax(-1)
    assert sorted(cols.tolist()) == list(range(1032))
    assert torch.all(x.abs().max(-1).values == 8.0)


@pytest.mark.parametrize("cols", [1024, 2048])
def test_rule_sees_a_dropped_chunk_that_the_norm_ratio_accepts(cols):
    """An RMSNorm whose sum of squares drops the last 8-column chunk passes ``rel < 5e-3`` on randn rows and
    fails the per-element rule on spiked rows; the correctly rounded bf16 result passes with margin to spare."""
    eps = 1e-5
    w = 1 + 0.1 * torch.randn(cols)
    plain = torch.randn(64, cols)
    ss = plain[:, :cols - 8].pow(2).sum(-1, keepdim=True)
    y_bad = (w * plain * torch.rsqrt(ss / cols + eps)).bfloat16()
    good = o64.rmsnorm(plain, w, eps)["y"]
    rel = ((y_bad.double() - good).norm() / good.norm()).item()
    assert rel < 5e-3  # what the whole-tensor ratio lets through

    x = o64.spiked(64, cols, "cpu")
    r = o64.rmsnorm(x, w, eps)
    twin = ref.rmsnorm(x, w, eps)
    y_ok = twin.bfloat16()
    o64.check(y_ok, r["y"], twin, name="y")
    assert o64.excess_ratio(y_ok, r["y"], twin) <= 1.0
    ss = x[:, :cols - 8].pow(2).sum(-1, keepdim=True)
    y_bad = (w * x * torch.rsqrt(ss / cols + eps)).bfloat16()
    with pytest.raises(AssertionError, match=r"worst at \(\d+, \d+\): out=.* ref64="):
        o64.check(y_bad, r["y"], twin, name="y")


def test_rule_counts_nan_and_fp32_outputs():
    ref64 = torch.linspace(-1, 1, 32, dtype=torch.float64)
    twin = ref64.float()
    out = twin.clone()
    o64.check(out, ref64, twin, name="fp32")
    out[7] = float("nan")
    with pytest.raises(AssertionError, match=r"worst at \(7,\)"):
        o64.check(out, ref64, twin, name="fp32")
    out = twin.clone()
    out[3] += 1e-5
    with pytest.raises(AssertionError, match=r"worst at \(3,\)"):
        o64.check(out, ref64, twin, name="fp32")


# ------------------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("rows,cols", [(1, 8), (3, 72), (5, 520), (3, 1032)])
@pytest.mark.parametrize("mode", ["plain", "res", "add"])
def test_rmsnorm_oracle_vs_torch_twin(rows, cols, mode):
    eps = 1e-5
    h = o64.spiked(rows, cols, "cpu")
    a = o64.spiked(rows, cols, "cpu", 0.5, start=3) if mode == "add" else None
    w = 1 + 0.1 * torch.randn(cols)
    dy, dres = torch.randn(rows, cols), torch.randn(rows, cols)
    gw0 = torch.randn(cols)
    gw = gw0.clone()
    hx = h.clone().requires_grad_(True)
    if mode == "plain":
        y = ops.rmsnorm(hx, w, gw, eps, torch.float32)
        y.backward(dy)
        r = o64.rmsnorm(h, w, eps, dy=dy)
    elif mode == "res":
        y, hn = ops.rmsnorm_res(hx, w, gw, eps, torch.float32)
        torch.autograd.backward((y, hn), (dy, dres))
        r = o64.rmsnorm(h, w, eps, dy=dy, dres=dres)
    else:
        ax = a.clone().requires_grad_(True)
        y, hn = ops.add_rmsnorm(hx, ax, w, gw, eps, torch.float32)
        torch.autograd.backward((y, hn), (dy, dres))
        r = o64.rmsnorm(h, w, eps, a=a, dy=dy, dres=dres)
        close(hn, r["h_new"])
        close(ax.grad, r["da"])
    close(y, r["y"])
    close(hx.grad, r["dx"])
    close(gw - gw0, r["dw"], 1e-4)  # accumulated into gw; the difference cancels fp32 digits
    hn64 = r["h_new"]
    close(torch.rsqrt(hn64.float().pow(2).mean(-1) + eps), r["rstd"])


def test_rmsnorm_oracle_bf16_residual_rounds_before_the_statistics():
    rows, cols, eps = 3, 520, 1e-5
    h = o64.spiked(rows, cols, "cpu").bfloat16()
    a = o64.spiked(rows, cols, "cpu", 0.5, start=3).bfloat16()
    w = 1 + 0.1 * torch.randn(cols)
    dy, dres = torch.randn(rows, cols).bfloat16(), torch.randn(rows, cols).bfloat16()
    hx, ax = h.clone().requires_grad_(True), a.clone().requires_grad_(True)
    gw = torch.zeros(cols)
    y, hn = ops.add_rmsnorm(hx, ax, w, gw, eps, torch.bfloat16)
    torch.autograd.backward((y, hn), (dy, dres))
    r = o64.rmsnorm(h, w, eps, a=a, round_hnew=True, dy=dy, dres=dres)
    assert torch.equal(hn, r["h_new"].float().bfloat16()) and torch.equal(hn.double(), r["h_new"])
    unrounded = o64.rmsnorm(h, w, eps, a=a)
    assert not torch.equal(unrounded["h_new"], r["h_new"])
    bf16_close(y, r["y"])
    bf16_close(hx.grad, r["dx"])
    assert torch.equal(hx.grad, ax.grad)
    close(gw, r["dw"], 1e-4)


def test_colsum_and_transpose_oracles():
    part, out = torch.randn(17, 68), torch.randn(68)
    close(out + part.sum(0), o64.colsum_add(part, out))
    x = torch.randn(65, 63).bfloat16()
    assert torch.equal(o64.transpose(x).float().bfloat16(), x.t())


# ------------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("hd,nh,nkv,B,T", [(8, 4, 4, 1, 1), (32, 4, 1, 3, 5), (64, 4, 2, 2, 96), (128, 4, 4, 3, 5)])
def test_rope_oracle_vs_reference(hd, nh, nkv, B, T):
    ld = (nh + 2 * nkv) * hd
    qkv = o64.spiked(B * T, ld, "cpu")
    cos, sin = ref.rope_tables(T, hd, 10000.0)
    q, k, v = ref.split_qkv(qkv, B, T, nh, nkv, hd)
    tw = torch.cat([ref.apply_rope(q, cos, sin).transpose(1, 2).reshape(B * T, -1),
                    ref.apply_rope(k, cos, sin).transpose(1, 2).reshape(B * T, -1),
                    v.transpose(1, 2).reshape(B * T, -1)], dim=1)
    r = o64.rope(qkv, cos, sin, B, T, nh, nkv, hd)
    close(tw, r)
    assert torch.equal(r[:, (nh + nkv) * hd:], qkv.double()[:, (nh + nkv) * hd:])
    back = o64.rope(r, cos, sin, B, T, nh, nkv, hd, inverse=True)
    close(back, qkv.double(), 5e-7)  # the fp32 tables are orthogonal to 2^-23 only


# ------------------------------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("n,F", [(1, 8), (3, 72)])
def test_swiglu_oracle_vs_torch_twin(n, F):
    gu = o64.spiked(n, 2 * F, "cpu")
    gu[0, :5] = torch.tensor([100.0, -100.0, 20.0, -20.0, 0.0])
    dy = torch.randn(n, F)
    x = gu.clone().requires_grad_(True)
    y = ops.swiglu(x)
    y.backward(dy)
    fwd, bwd = o64.swiglu_fwd(gu), o64.swiglu_bwd(dy, gu)
    assert torch.isfinite(fwd).all() and torch.isfinite(bwd).all()
    close(y, fwd)
    close(x.grad, bwd)
    close(ref.swiglu_backward(dy, gu), bwd)


# ------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16])
def test_embedding_oracle_vs_torch_twin_and_masks_bad_ids(odt):
    V, d, n = 50, 100, 37
    W = torch.randn(V, d)
    base = torch.randn(V, d)
    ids = torch.randint(0, V, (n,))
    ids[::5] = 7
    gW = base.clone()
    out = ops.embedding(ids, W, gW, out_dtype=odt)
    dy = torch.randn(n, d).to(odt)
    out.backward(dy)
    assert torch.equal(out, o64.embedding_fwd(ids, W).float().to(odt))
    close(gW, o64.embedding_bwd(ids, dy, V, base))
    # out-of-range ids: zero rows forward, no contribution backward (the twin would raise on them)
    bad = ids.clone()
    bad[1], bad[2], bad[30] = -1, V, V + 5
    keep = torch.ones(n, dtype=torch.bool)
    keep[[1, 2, 30]] = False
    f = o64.embedding_fwd(bad, W)
    assert torch.equal(f[keep], o64.embedding_fwd(ids, W)[keep]) and not f[~keep].any()
    assert torch.equal(o64.embedding_bwd(bad, dy, V, base), o64.embedding_bwd(ids[keep], dy[keep], V, base))


# ------------------------------------------------------------------------------------------ cross-entropy
def _ce_case(V, n=18):
    x = 4 * torch.randn(n, V)
    x[1::3] = -60.0
    x[1::3, V // 3] = 60.0
    x[2::3] = 1.5
    return x


@pytest.mark.parametrize("V", [8, 100])
@pytest.mark.parametrize("all_ignored", [False, True])
def test_ce_oracle_vs_lm_head_ce_twin(V, all_ignored):
    """The torch branch of ``ops.lm_head_ce`` with W = I (logits = y exactly): loss and d(logits)."""
    x = _ce_case(V)
    n = x.shape[0]
    tgt = torch.randint(0, V, (n,))
    tgt[0], tgt[1], tgt[2], tgt[3] = 0, V - 1, -100, x[3].argmax()
    if all_ignored:
        tgt[:] = -100
    scale = 0.25
    y = x.clone().requires_grad_(True)
    gW = torch.zeros(V, V)
    loss = ops.lm_head_ce(y, torch.eye(V), gW, tgt, loss_scale=scale)
    loss.backward()
    nvalid = max(int((tgt != -100).sum()), 1)
    lse, rows, dl = o64.ce_rows(x, tgt, scale / nvalid)
    close(torch.logsumexp(x, -1), lse)
    assert abs(loss.item() - rows.sum().item() / nvalid) <= 2e-6 * max(1.0, rows.sum().item() / nvalid)
    close(y.grad, dl) if not all_ignored else None
    assert not rows[tgt == -100].any() and not dl[tgt == -100].any()
    if all_ignored:
        assert loss.item() == 0.0 and not y.grad.any() and not dl.any()
    else:
        p = torch.softmax(x.double(), -1)
        assert torch.allclose(dl.sum(-1)[tgt != -100], torch.zeros(1, dtype=torch.float64), atol=1e-12)
        assert torch.allclose(dl[0] / (scale / nvalid) + torch.nn.functional.one_hot(tgt[0], V), p[0], atol=1e-12)


# ------------------------------------------------------------------------------------------ optimizer
@pytest.mark.parametrize("n", [1, 5, 1027])
@pytest.mark.parametrize("max_norm,wd", [(None, 0.0), (1.0, 0.01), (1e9, 0.01)])
def test_adamw_oracle_vs_torch_twin(n, max_norm, wd):
    p32, m32, v32 = torch.randn(n), torch.zeros(n), torch.zeros(n)
    p64, m64, v64 = p32.double(), m32.double(), v32.double()
    norm = torch.zeros(1)
    sh = torch.zeros(n, dtype=torch.bfloat16)
    for step in (1, 2, 3):
        g = o64.spiked(1, n, "cpu", 3.0)[0] if n >= 8 else 3 * torch.randn(n)
        ops.adamw_step(p32, g.clone(), m32, v32, sh, step, 1e-3, (0.9, 0.999), 1e-8, wd, max_norm, norm_out=norm)
        p64, m64, v64, n64 = o64.adamw(p64, g, m64, v64, step, 1e-3, (0.9, 0.999), 1e-8, wd, max_norm)
        close(p32, p64, 1e-6)
        close(m32, m64, 1e-6)
        close(v32, v64, 1e-6)
        assert abs(norm.item() - n64.item()) <= 1e-6 * n64.item()
        assert torch.equal(sh, p32.bfloat16())
    if n == 1027:  # the same three steps through torch.optim.AdamW + clip_grad_norm_
        torch.manual_seed(0)
        q = torch.nn.Parameter(torch.randn(n))
        opt = torch.optim.AdamW([q], lr=1e-3, weight_decay=wd)
        for step in (1, 2, 3):
            q.grad = o64.spiked(1, n, "cpu", 3.0)[0]
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_([q], max_norm)
            opt.step()
        close(q.detach(), p64, 1e-6)


@pytest.mark.parametrize("comm", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("drift", [False, True])
def test_outer_step_oracles_vs_torch_twin(comm, drift):
    n = 259
    sync = torch.randn(n)
    local = sync - 0.01 * torch.randn(n)
    delta = torch.empty(n, dtype=comm)
    ops.pseudograd(sync, local, delta)
    assert torch.equal(delta, o64.pseudograd(sync, local).float().to(comm))
    master32, sync32, mom32 = local.clone(), sync.clone(), torch.full((n,), 7.0)
    master64, sync64, mom64 = local.double(), sync.double(), mom32.double()
    sh = torch.zeros(n, dtype=torch.bfloat16)
    for first in (True, False):
        dsum = (4 * delta.float() + 0.003 * torch.randn(n)).to(comm)
        base = 0.01 * torch.randn(n) if drift else None
        ops.outer_nesterov(master32, sync32, dsum, mom32, sh, 0.25, 0.7, 0.9, first, drift_base=base)
        master64, sync64, mom64 = o64.outer_nesterov(master64, sync64, dsum, mom64, 0.25, 0.7, 0.9, first, base)
        close(master32, master64, 1e-6)
        close(sync32, sync64, 1e-6)
        close(mom32, mom64, 1e-6)
        assert torch.equal(sh, master32.bfloat16())
        if not drift:
            assert torch.equal(master64, sync64)


# ------------------------------------------------------------------------------------------ attention
ATTN = dict(B=2, T=70, nh=4, nkv=2, hd=16)
ATTN_MODES = ["none", "kstart", "doc"]


def _attn_case(mode, dtype=torch.float64):
    B, T, nh, nkv, hd = (ATTN[k] for k in ("B", "T", "nh", "nkv", "hd"))
    raw = torch.randn(B * T, (nh + 2 * nkv) * hd, dtype=torch.float64)
    raw[T // 2, nh * hd:(nh + 1) * hd] *= 20  # a late key with a large score
    cos, sin = ref.rope_tables(T, hd, 10000.0)
    dO = o64.spiked(B * T, nh * hd, "cpu").double()
    kstart = doc = None
    if mode == "kstart":
        kstart = torch.tensor([0, 13], dtype=torch.int32)
    if mode == "doc":
        ids = torch.full((B, T), 7)
        ids[0, 30] = ids[1, 0] = ids[1, 63] = ids[1, 64] = 2
        doc = ops.doc_bounds(ids, 2)
    return raw.to(dtype), cos, sin, dO, kstart, doc


@pytest.mark.parametrize("mode", ATTN_MODES)
def test_attention_oracle_matches_reference_autograd(mode):
    """o64.attention on the rotated rows against ref.attention_block (float64 inputs, autograd) on the raw rows, GQA:
    the output and, through ``rope_out``, the three gradients with respect to the raw rows, 1e-10 of the tensor's
    maximum.  Fully masked rows (SDPA gives NaN or 0 for them, the oracle 0) are compared to 0 and take no dO."""
    B, T, nh, nkv, hd = (ATTN[k] for k in ("B", "T", "nh", "nkv", "hd"))
    raw, cos, sin, dO, kstart, doc = _attn_case(mode)
    rot = o64.rope(raw, cos, sin, B, T, nh, nkv, hd)
    r = o64.attention(rot, B, T, nh, nkv, hd, hd ** -0.5, kstart=kstart, doc_start=doc[0] if doc else None, dO=dO,
                      rope_out=True, cos=cos, sin=sin, o_saved=None)
    seen = r["seen"].reshape(-1)
    assert bool(seen.all()) == (mode != "kstart") and int((~seen).sum()) == (13 if mode == "kstart" else 0)
    x = raw.clone().requires_grad_(True)
    o = ref.attention_block(x, cos.double(), sin.double(), B, T, nh, nkv, hd, kstart=kstart, doc_bounds=doc)
    close(o.detach()[seen], r["o"][seen], 1e-10)
    assert not bool(r["o"][~seen].any())
    # the oracle's delta uses o rounded to bf16; autograd's does not: give the oracle the unrounded o to compare
    r = o64.attention(rot, B, T, nh, nkv, hd, hd ** -0.5, kstart=kstart, doc_start=doc[0] if doc else None, dO=dO,
                      rope_out=True, cos=cos, sin=sin, o_saved=r["o"])
    (o[seen] * dO[seen]).sum().backward()
    nq, nk = nh * hd, nkv * hd
    g = x.grad.nan_to_num(0.0) if mode == "kstart" else x.grad
    close(g[:, :nq], r["dq"], 1e-10)
    close(g[:, nq:nq + nk], r["dk"], 1e-10)
    close(g[:, nq + nk:], r["dv"], 1e-10)
    assert torch.equal(r["dqkv"], torch.cat([r["dq"], r["dk"], r["dv"]], 1))
    lse = torch.logsumexp((rot.view(B, T, -1)[..., :hd] @ rot.view(B, T, -1)[..., nq:nq + hd].transpose(1, 2) * hd ** -0.5)
                          .masked_fill(~r["mask"][:, 0], float("-inf")), -1)
    close(r["lse2"][:, 0][r["seen"]], lse[r["seen"]] * o64.LOG2E, 1e-12)
    assert bool((r["lse2"][:, 0][~r["seen"]] == float("-inf")).all())


def test_attention_oracle_masks_and_masked_rows():
    B, T = 3, 67
    ks = torch.tensor([0, 65, T], dtype=torch.int32)
    assert torch.equal(o64.attention_mask(B, T, "cpu", kstart=ks), ref.padded_causal_mask(ks, T))
    ids = torch.randint(0, 5, (B, T))
    ds, _ = ops.doc_bounds(ids, 2)
    assert torch.equal(o64.attention_mask(B, T, "cpu", doc_start=ds), ref.doc_causal_mask(ds, T))
    t = torch.arange(T)
    assert torch.equal(o64.attention_mask(1, T, "cpu")[0, 0], t[None, :] <= t[:, None])
    # an all-pad sequence: everything 0 and finite, lse -inf
    nh, nkv, hd = 2, 1, 8
    x = torch.randn(B * T, (nh + 2 * nkv) * hd).bfloat16()
    dO = torch.randn(B * T, nh * hd).bfloat16()
    for fn in (o64.attention, o64.attention_twin):
        r = fn(x, B, T, nh, nkv, hd, 0.3, kstart=ks, dO=dO)
        assert torch.equal(r["seen"], t[None, :] >= ks[:, None].long())
        pad = ~r["seen"].reshape(-1)
        for k in ("o", "dq", "dk", "dv"):
            assert bool(torch.isfinite(r[k]).all()) and not bool(r[k][pad].any()), k
        assert not bool(r["delta"].transpose(1, 2).reshape(B * T, nh)[pad].any())
        assert bool((r["lse2"].transpose(1, 2).reshape(B * T, nh)[pad] == float("-inf")).all())
        assert bool(torch.isfinite(r["lse2"].transpose(1, 2).reshape(B * T, nh)[~pad]).all())


@pytest.mark.parametrize("mode", ATTN_MODES)
def test_attention_twin_is_a_bf16_operand_model(mode):
    """The twin's distance from the oracle (the unit of the GPU tests' slack) is non-zero and below 2^-6 of the
    tensor's maximum, for every output: a sanity bound on the model, not on a kernel."""
    B, T, nh, nkv, hd = (ATTN[k] for k in ("B", "T", "nh", "nkv", "hd"))
    raw, cos, sin, dO, kstart, doc = _attn_case(mode)
    rot = o64.rope(raw, cos, sin, B, T, nh, nkv, hd).bfloat16()
    kw = dict(kstart=kstart, doc_start=doc[0] if doc else None, dO=dO.bfloat16(), rope_out=True, cos=cos, sin=sin)
    r = o64.attention(rot, B, T, nh, nkv, hd, hd ** -0.5, **kw)
    tw = o64.attention_twin(rot, B, T, nh, nkv, hd, hd ** -0.5, **kw)
    for k in ("o", "dq", "dk", "dv", "lse2", "delta"):
        a, b = tw[k].double(), r[k]
        fin = torch.isfinite(b)
        assert torch.equal(torch.isfinite(a), fin), k
        d = (a[fin] - b[fin]).abs().max().item()
        assert 0.0 < d < 2.0 ** -6 * b[fin].abs().max().item(), (k, d, b[fin].abs().max().item())
    assert tw["lse2"].dtype == torch.float32 and tw["delta"].dtype == torch.float32


# ------------------------------------------------------------------------------------------ fp8 code tables
FP8_DT = {0: torch.float8_e4m3fn, 1: torch.float8_e5m2}
FP8_SCALES = [1.0, 2.0 ** -3, 2.0 ** 5, 37.5]


@pytest.mark.parametrize("fmt", [0, 1])
def test_fp8_code_table(fmt):
    """The table from the format definition: 256 values, sign symmetry, FMAX, the smallest subnormal, the NaN /
    inf codes, strictly increasing finite codes -- and the same values torch decodes (decoding is exact)."""
    c = o64.fp8_codes(fmt)
    assert c.shape == (256,) and c.dtype == torch.float64
    fin = torch.isfinite(c)
    assert c[fin].abs().max().item() == o64.FP8_FMAX[fmt]
    assert c[1].item() == (2.0 ** -9 if fmt == 0 else 2.0 ** -16) and c[0].item() == 0.0
    assert bool(torch.signbit(c[128])) and c[128].item() == 0.0
    assert torch.equal(c[128:][fin[128:]], -c[:128][fin[:128]])
    nan = [b for b in range(256) if c[b] != c[b]]
    assert nan == ([0x7F, 0xFF] if fmt == 0 else [0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF])
    assert (fmt == 0 and not torch.isinf(c).any()) or (c[0x7C].item() == float("inf") and c[0xFC].item() == -float("inf"))
    f = c[:128][fin[:128]]
    assert f.numel() == (127 if fmt == 0 else 124) and bool((f[1:] > f[:-1]).all())
    dec = torch.arange(256, dtype=torch.uint8).view(FP8_DT[fmt]).double()
    assert torch.equal(dec.nan_to_num(nan=12345.0), c.nan_to_num(nan=12345.0))
    assert torch.equal(torch.signbit(dec)[~torch.isnan(c)], torch.signbit(c)[~torch.isnan(c)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fmt", [0, 1])
def test_fp8_probes_hold_what_they_claim(fmt, dtype):
    p = o64.fp8_probes(fmt, dtype)
    assert p.dtype == dtype and p.numel() == (1018 if fmt == 0 else 994) and not torch.isnan(p).any()
    c = o64.fp8_codes(fmt)
    f = c[:128][torch.isfinite(c[:128])]
    have = set(p.double().tolist())
    for v in f.tolist() + ((f[:-1] + f[1:]) / 2).tolist():
        assert v in have and -v in have
    half = f[1].item() / 2  # half the smallest subnormal and its two neighbours
    nb = torch.tensor([half], dtype=dtype)
    for v in (half, o64._ulp_step(nb, True).item(), o64._ulp_step(nb, False).item()):
        assert v in have
    assert o64._ulp_step(torch.tensor([o64.FP8_FMAX[fmt]], dtype=dtype), True).item() in have
    assert float("inf") in have and -float("inf") in have
    assert int((p == 0).sum()) == 4 and int(torch.signbit(p[p == 0]).sum()) == 2


@pytest.mark.parametrize("scale", FP8_SCALES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fmt", [0, 1])
def test_fp8_quantise_matches_torch_on_the_probes(fmt, dtype, scale):
    """The oracle (a search in the code table) == torch's multiply, clamp and float8 conversion, byte for byte, on
    every probe; for the power-of-two scales ``probe / scale`` is passed so that the product is the probe."""
    p = o64.fp8_probes(fmt, dtype)
    x = (p.double() / scale).to(dtype) if scale != 37.5 else p
    if scale != 37.5:
        fin = torch.isfinite(p) & ((p.double() / scale).abs() < 3e38)
        assert torch.equal((x.double() * scale)[fin], p.double()[fin])  # exact: lands on the probe
    F = o64.FP8_FMAX[fmt]
    ref = x.float().mul(scale).clamp(-F, F).to(FP8_DT[fmt]).view(torch.uint8)
    got = o64.fp8_quantise(x, scale, fmt)
    assert got.dtype == torch.uint8 and got.shape == x.shape
    bad = (got != ref).nonzero().reshape(-1).tolist()
    assert not bad, [(x[i].item(), hex(got[i]), hex(ref[i])) for i in bad[:8]]
    assert not o64.fp8_is_nan(got, fmt).any()
    # the rules, stated once without torch: ties to the even code, sign of zero, saturation
    one = lambda v: int(o64.fp8_quantise(torch.tensor([v], dtype=torch.float32), 1.0, fmt)[0])  # noqa: E731
    c = o64.fp8_codes(fmt)
    assert one(-0.0) == 0x80 and one(0.0) == 0
    assert one((c[1].item() + c[2].item()) / 2) == 2 and one((c[2].item() + c[3].item()) / 2) == 2
    assert one(c[1].item() / 2) == 0 and one(-c[1].item() / 2) == 0x80
    top = 0x7E if fmt == 0 else 0x7B
    assert one(float("inf")) == top and one(-1e30) == top | 0x80 and one(F) == top


@pytest.mark.parametrize("fmt", [0, 1])
def test_fp8_quantise_nan(fmt):
    """NaN in, a NaN code out -- in the oracle and in torch's conversion (clamp keeps NaN), whatever the byte."""
    x = torch.tensor([1.0, float("nan"), -float("nan"), 3.0])
    F = o64.FP8_FMAX[fmt]
    for scale in FP8_SCALES:
        got = o64.fp8_quantise(x, scale, fmt)
        ref = x.mul(scale).clamp(-F, F).to(FP8_DT[fmt])
        assert o64.fp8_is_nan(got, fmt).tolist() == [False, True, True, False]
        assert o64.fp8_is_nan(ref, fmt).tolist() == [False, True, True, False]
        assert torch.isnan(ref.float()).tolist() == [False, True, True, False]
        assert bool(o64.fp8_same(got, ref, fmt).all())


@pytest.mark.parametrize("fmt", [0, 1])
def test_fp8_quantise_matches_torch_on_random_products(fmt):
    """Off the probes: 200 000 random fp32 values over the whole range of the format at scale 37.5, where the product
    is inexact and its one rounding to fp32 (not the float64 product) decides the side of a midpoint."""
    g = torch.Generator().manual_seed(1)
    F = o64.FP8_FMAX[fmt]
    x = torch.randn(200000, generator=g) * torch.exp2(torch.randint(-20, 12, (200000,), generator=g).float())
    ref = x.mul(37.5).clamp(-F, F).to(FP8_DT[fmt]).view(torch.uint8)
    assert torch.equal(o64.fp8_quantise(x, 37.5, fmt), ref)
    assert torch.equal(o64.fp8_quantise(x, torch.tensor([37.5]), fmt), ref)  # the scale as a one-element tensor
