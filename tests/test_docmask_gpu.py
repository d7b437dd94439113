"""Document-masked flash attention (``ops.attention(..., doc_bounds=...)``, ``--doc-mask``) on the GPU: the three
LDS-DMA kernels' document mode against fp32 math under an explicit boolean mask, exact isolation of documents,
determinism, the error paths, the model flag and HIP-graph replay."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
EOS = 2


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    torch.manual_seed(0)
    yield
    ops.set_backend("auto")


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def bounds(T, starts_per_row):
    """(doc_start, doc_end) through the public path: EOS right before every listed document start."""
    ids = torch.full((len(starts_per_row), T), 7, dtype=torch.long)
    for b, starts in enumerate(starts_per_row):
        for s in starts:
            assert 0 < s < T
            ids[b, s - 1] = EOS
    ds, de = ops.doc_bounds(ids.to(DEV), EOS)
    ops.check_doc_bounds(ds, de)
    return ds, de


def boundary_sets(T):
    g = torch.Generator().manual_seed(1234)
    rnd = sorted(set((torch.randperm(T - 1, generator=g)[:max(2, T // 48)] + 1).tolist()))
    sets = {
        "none": [],
        "aligned": [s for s in (64, 128, 256) if s < T],
        "off_by_one": sorted({s for s in (1, 63, 65, 127, 129, T - 1) if 0 < s < T}),
        "one_token_docs": [s for s in range(62, 68) if s < T],
        "random": rnd,
    }
    return sets


SHAPES = [(2, 64, 2, 2, 64), (2, 128, 2, 1, 64), (1, 256, 2, 2, 64), (2, 512, 4, 1, 64), (1, 256, 2, 2, 32),
          (1, 512, 2, 2, 128), (1, 1024, 2, 1, 64)]
SETS = ["none", "aligned", "off_by_one", "one_token_docs", "random"]


def rows_for(T, B, name):
    """Row 0 gets the named set; a second row gets the next one in the list, so the rows differ."""
    sets = boundary_sets(T)
    return [sets[SETS[(SETS.index(name) + b) % len(SETS)]] for b in range(B)]


def fp32_masked(qkv, cos, sin, B, T, nh, nkv, hd, mask):
    """Plain fp32 math: softmax(q k^T / sqrt(hd) + mask) v with an explicit boolean [B, 1, T, T] mask."""
    q, k, v = ref.split_qkv(qkv, B, T, nh, nkv, hd)
    q, k = ref.apply_rope(q, cos[:T], sin[:T]), ref.apply_rope(k, cos[:T], sin[:T])
    if nkv != nh:
        k = k.repeat_interleave(nh // nkv, dim=1)
        v = v.repeat_interleave(nh // nkv, dim=1)
    s = torch.matmul(q, k.transpose(-1, -2)) * hd ** -0.5
    p = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1)
    return torch.matmul(p, v).transpose(1, 2).reshape(B * T, nh * hd)


def grads_close(g, gr, nh, nkv, hd, tag):
    nq, nk = nh * hd, nkv * hd
    for name, a, b in (("dq", g[:, :nq], gr[:, :nq]), ("dk", g[:, nq:nq + nk], gr[:, nq:nq + nk]),
                       ("dv", g[:, nq + nk:], gr[:, nq + nk:])):
        e = rel(a, b)
        print(f"{tag} {name} rel {e:.3e}")
        assert e < 3e-2, (tag, name, e)


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("B,T,nh,nkv,hd", SHAPES)
def test_doc_attention_matches_fp32_mask(B, T, nh, nkv, hd, name):
    """Forward and all three gradients against fp32 attention under the explicit block-diagonal causal mask.
    T = 256 with a start in 64..127 gives the second query block an odd first tile; T = 512 with nh/nkv = 4
    shortens the dK/dV walk under GQA; one-token documents straddle the 64-key tile edge."""
    from nanodiloco_amd.ops.attention import rope_cache

    rows = rows_for(T, B, name)
    ds, de = bounds(T, rows)
    t = torch.arange(T, device=DEV)
    mask = ((t[None, :] <= t[:, None])[None] & (t.view(1, 1, T) >= ds.view(B, T, 1))).unsqueeze(1)
    assert torch.equal(mask, ref.doc_causal_mask(ds, T))
    qkv = torch.randn(B * T, (nh + 2 * nkv) * hd, device=DEV).bfloat16()
    cos, sin = rope_cache(T, hd, 10000.0, None, DEV)
    x = qkv.clone().requires_grad_(True)
    o = ops.attention(x, cos, sin, B, T, nh, nkv, hd, doc_bounds=(ds, de))
    xr = qkv.float().requires_grad_(True)
    orf = fp32_masked(xr, cos, sin, B, T, nh, nkv, hd, mask)
    assert torch.isfinite(o.float()).all()
    e = rel(o, orf)
    print(f"{(B, T, nh, nkv, hd)} {name} out rel {e:.3e}")
    assert e < 1e-2, e
    do = torch.randn_like(orf)
    o.backward(do.bfloat16())
    orf.backward(do.bfloat16().float())
    assert torch.isfinite(x.grad.float()).all()
    grads_close(x.grad.float(), xr.grad, nh, nkv, hd, f"{(B, T, nh, nkv, hd)} {name}")


LEAK = dict(B=2, T=256, nh=2, nkv=1, hd=64)
LEAK_ROWS = [[100], [65, 190]]  # document A = [0, 100) / [0, 65); row 1's document B = [65, 190)


def test_no_leak_forward_bitwise():
    """A finite perturbation of document A's K and V rows leaves every output row of the later documents bitwise
    unchanged (the tiles they share with A contribute exact zeros, the others are never read)."""
    from nanodiloco_amd.ops.attention import rope_cache

    B, T, nh, nkv, hd = (LEAK[k] for k in ("B", "T", "nh", "nkv", "hd"))
    ds, de = bounds(T, LEAK_ROWS)
    qkv = torch.randn(B * T, (nh + 2 * nkv) * hd, device=DEV).bfloat16()
    cos, sin = rope_cache(T, hd, 10000.0, None, DEV)
    other = qkv.clone().view(B, T, -1)
    for b, rows in enumerate(LEAK_ROWS):
        other[b, :rows[0], nh * hd:] += 3.0  # K and V of document A
    other = other.view(B * T, -1)
    with torch.no_grad():
        o1 = ops.attention(qkv, cos, sin, B, T, nh, nkv, hd, doc_bounds=(ds, de)).view(B, T, -1)
        o2 = ops.attention(other, cos, sin, B, T, nh, nkv, hd, doc_bounds=(ds, de)).view(B, T, -1)
    for b, rows in enumerate(LEAK_ROWS):
        assert torch.equal(o1[b, rows[0]:], o2[b, rows[0]:]), b
        assert not torch.equal(o1[b, 1:rows[0]], o2[b, 1:rows[0]]), b  # the perturbation is seen inside A


def test_no_leak_backward_exact_zero():
    """dO non-zero only inside document B: dq, dk and dv are exactly zero on every row outside B."""
    from nanodiloco_amd.ops.attention import rope_cache

    B, T, nh, nkv, hd = (LEAK[k] for k in ("B", "T", "nh", "nkv", "hd"))
    ds, de = bounds(T, LEAK_ROWS)
    inside = torch.zeros(B, T, dtype=torch.bool, device=DEV)
    inside[0, 100:] = True      # row 0: B = [100, T)
    inside[1, 65:190] = True    # row 1: B = [65, 190), documents before and after it
    qkv = torch.randn(B * T, (nh + 2 * nkv) * hd, device=DEV).bfloat16()
    cos, sin = rope_cache(T, hd, 10000.0, None, DEV)
    x = qkv.clone().requires_grad_(True)
    o = ops.attention(x, cos, sin, B, T, nh, nkv, hd, doc_bounds=(ds, de))
    do = torch.randn_like(o) * inside.view(B * T, 1)
    o.backward(do)
    g = x.grad.view(B, T, -1)
    assert torch.isfinite(g.float()).all()
    assert (g[~inside] == 0).all()
    assert (g[inside].float().abs().sum(-1) > 0).all()


def test_backward_is_deterministic():
    from nanodiloco_amd.ops.attention import rope_cache

    B, T, nh, nkv, hd = 2, 512, 4, 1, 64
    ds, de = bounds(T, [boundary_sets(T)["random"], boundary_sets(T)["off_by_one"]])
    qkv = torch.randn(B * T, (nh + 2 * nkv) * hd, device=DEV).bfloat16()
    cos, sin = rope_cache(T, hd, 10000.0, None, DEV)
    do = torch.randn(B * T, nh * hd, device=DEV).bfloat16()

    def run():
        x = qkv.clone().requires_grad_(True)
        ops.attention(x, cos, sin, B, T, nh, nkv, hd, doc_bounds=(ds, de)).backward(do)
        return x.grad

    assert torch.equal(run(), run())


@pytest.mark.parametrize("B,T,nh,nkv,hd", [(2, 256, 4, 2, 64), (1, 192, 2, 2, 128)])
def test_single_document_agrees_with_plain_causal(B, T, nh, nkv, hd):
    """doc_start = 0, doc_end = T is plain causal attention (not bitwise: the masked forward uses the plain
    softmax variant, as the left-pad mode does)."""
    from nanodiloco_amd.ops.attention import rope_cache

    ds = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    de = torch.full((B, T), T, dtype=torch.int32, device=DEV)
    qkv = torch.randn(B * T, (nh + 2 * nkv) * hd, device=DEV).bfloat16()
    cos, sin = rope_cache(T, hd, 10000.0, None, DEV)
    do = torch.randn(B * T, nh * hd, device=DEV).bfloat16()
    x1, x2 = qkv.clone().requires_grad_(True), qkv.clone().requires_grad_(True)
    o1 = ops.attention(x1, cos, sin, B, T, nh, nkv, hd, doc_bounds=(ds, de))
    o2 = ops.attention(x2, cos, sin, B, T, nh, nkv, hd)
    assert rel(o1, o2) < 1e-2, rel(o1, o2)
    o1.backward(do)
    o2.backward(do)
    grads_close(x1.grad.float(), x2.grad.float(), nh, nkv, hd, "single document")


def test_errors():
    from nanodiloco_amd.ops.attention import rope_cache

    B, nh, nkv, hd = 1, 2, 2, 64
    for T, kw in ((96, {}), (128, {"kstart": torch.zeros(B, dtype=torch.int32, device=DEV)})):
        ds, de = bounds(T, [[40]])
        qkv = torch.randn(B * T, (nh + 2 * nkv) * hd, device=DEV).bfloat16()
        cos, sin = rope_cache(T, hd, 10000.0, None, DEV)
        with pytest.raises(ValueError):
            ops.attention(qkv, cos, sin, B, T, nh, nkv, hd, doc_bounds=(ds, de), **kw)


def _packed_ids(B, T, vocab, eos_rows, seed):
    ids = torch.randint(3, vocab, (B, T), generator=torch.Generator().manual_seed(seed))
    for b, pos in enumerate(eos_rows):
        ids[b, pos] = EOS
    return ids.to(DEV)


@pytest.mark.parametrize("ckpt", [False, True])
def test_model_doc_mask_hip_vs_torch_fp32(ckpt):
    """The tiny config with doc_mask on the HIP path (bf16) against the same weights on the torch reference path
    in fp32: loss and the flat gradient."""
    from nanodiloco_amd.config import resolve_llama_config
    from nanodiloco_amd.models import LlamaForCausalLM

    cfg = resolve_llama_config("llama_tiny.json")
    ids = _packed_ids(2, 128, cfg.vocab_size, [[20, 63, 64, 100], [5, 90]], seed=5)
    res = {}
    for backend, dt in (("torch", torch.float32), ("hip", torch.bfloat16)):
        ops.set_backend(backend)
        m = LlamaForCausalLM(cfg, DEV, dt, doc_mask=True,
                             activation_checkpointing=ckpt and backend == "hip").init_weights(3)
        out = m(ids, labels=ids)
        out.loss.backward()
        torch.cuda.synchronize()
        res[backend] = (out.loss.item(), m.store.grad.clone())
    ops.set_backend("hip")
    (l_t, g_t), (l_h, g_h) = res["torch"], res["hip"]
    e = rel(g_h, g_t)
    print(f"ckpt={ckpt} loss torch {l_t:.6f} hip {l_h:.6f} rel {abs(l_t - l_h) / abs(l_t):.3e} grad rel {e:.3e}")
    assert abs(l_t - l_h) < 2e-3 * abs(l_t), (l_t, l_h)
    assert e < 3e-2, e


def test_hip_graph_replay_follows_each_batch():
    """GraphedMicroStep on a doc_mask model: the bounds are derived on the device from the captured ids buffer,
    so every replay masks by its own micro-batch's EOS positions."""
    from nanodiloco_amd.config import resolve_llama_config
    from nanodiloco_amd.models import LlamaForCausalLM
    from nanodiloco_amd.utils.graphs import GraphedMicroStep

    cfg = resolve_llama_config("llama_tiny.json")
    ops.set_deterministic(True)
    try:
        m = LlamaForCausalLM(cfg, DEV, torch.bfloat16, doc_mask=True).init_weights(3)
        plain = LlamaForCausalLM(cfg, DEV, torch.bfloat16, store=m.store)
        g = GraphedMicroStep(m)
        base = _packed_ids(2, 128, cfg.vocab_size, [[], []], seed=9)
        batches = []
        for eos_rows in ([[30, 64], [100]], [[1, 65, 66], [40, 41, 127]]):
            ids = base.clone()
            for b, pos in enumerate(eos_rows):
                ids[b, pos] = EOS
            batches.append(ids)
        for _ in range(g.warmup):
            g(batches[0], batches[0])
        assert g.graph is None
        losses = []
        for ids in batches + batches[:1]:
            l = float(g(ids, ids).clone())
            assert g.graph is not None and g.eager_fallbacks == 0
            with torch.no_grad():
                eager = float(m(ids, labels=ids).loss)
                nomask = float(plain(ids, labels=ids).loss)
            assert l == eager, (l, eager)
            assert l != nomask
            losses.append(l)
        assert losses[0] != losses[1] and losses[0] == losses[2]
    finally:
        ops.set_deterministic(False)
