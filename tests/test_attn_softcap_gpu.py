"""Attention logit soft-capping on the HIP path per element against the dense float64 formula of
``tests/_attn_softcap.py``, by the rule of ``_oracle64.check`` (margin 8; docs/PARITY.md has the measured margins).
RoPE runs with the identity tables (cos = 1, sin = 0), which rotate and un-rotate exactly.  C = 1 saturates tanh (the
x20 late key sits deep in it, 1 - t^2 towards 0), C = 50 keeps the plain rows in ``cap_tanh``'s series branch."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops.decode import attn_decode_launch, decode_split, decode_workspace

from . import _attn_softcap as ac
from . import _oracle64 as o64

pytestmark = pytest.mark.gpu
DEV, BF16 = "cuda", torch.bfloat16


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    yield
    ops.set_backend("auto")


def inputs(B, T, nh, nkv, hd, spike, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * T, (nh + 2 * nkv) * hd, generator=g)
    if spike:  # a x20 late key
        qkv[T - 3, nh * hd:(nh + nkv) * hd] *= 20.0
    return qkv.to(DEV, BF16), torch.randn(B * T, nh * hd, generator=g).to(DEV, BF16)


def mask_args(kind, B, T):
    """(kwargs of ops.attention, the oracle's boolean mask)"""
    if kind == "kstart":
        ks = torch.tensor([5] + [0] * (B - 1), dtype=torch.int32, device=DEV)  # queries 0..4 of row 0 see no key
        return dict(kstart=ks), ac.mask(B, T, DEV, kstart=ks)
    if kind == "doc":
        ids = torch.ones(B, T, dtype=torch.long, device=DEV)
        ids[0, T // 2 - 1] = ids[1, 40] = 0  # a document ends on a tile edge, another inside a wave's rows
        ds, de = ops.doc_bounds(ids, 0)
        return dict(doc_bounds=(ds, de)), ac.mask(B, T, DEV, doc_start=ds)
    if kind == "window":
        return dict(window=33), ac.mask(B, T, DEV, window=33)
    return {}, ac.mask(B, T, DEV)


def tables(T, hd):
    return torch.ones(T, hd, device=DEV), torch.zeros(T, hd, device=DEV)


def cases():
    """(T, hd, nh, nkv, C, mask): every T % 64 == 0 with every mask (forward and fused backward), head_dim, the GQA
    ratio and the cap rotating across them; then the ragged T of the register-staged forward (no gradient there)."""
    pairs = [(T, k) for T in (64, 128, 192) for k in ("none", "kstart", "doc", "window")]
    return [(T, (32, 64, 128)[i % 3], *((2, 2), (4, 2))[(i // 2) % 2], (1.0, 50.0)[(i + i // 4) % 2], k)
            for i, (T, k) in enumerate(pairs)] + [(1, 32, 2, 2, 1.0, "none"), (33, 64, 4, 2, 50.0, "window"),
                                                  (130, 128, 2, 2, 1.0, "kstart"), (130, 64, 4, 2, 50.0, "none")]


@pytest.mark.parametrize("T,hd,nh,nkv,C,kind", cases())
def test_against_float64(T, hd, nh, nkv, C, kind):
    B, grad = 2, T % 64 == 0
    qkv, dO = inputs(B, T, nh, nkv, hd, spike=C == 1.0 and T > 3, seed=T + hd)
    kw, ok = mask_args(kind, B, T)
    note = f"T={T} hd={hd} nh={nh} nkv={nkv} C={C} {kind}"
    x = qkv.clone().requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        o = ops.attention(x, *tables(T, hd), B, T, nh, nkv, hd, softcap=C, **kw)
    ref, tw = ac.oracle_and_twin(qkv, B, T, nh, nkv, hd, C, ok, dO=dO if grad else None)
    o64.check(o.detach(), ref["o"], tw["o"], name="attn.cap.o", note=note)
    dead = ~ref["seen"].reshape(-1)  # fully masked rows: o = 0, lse = -inf, no gradient into their q
    assert not bool(o[dead].any()), note
    if not grad:
        return
    lse, seen = o.grad_fn.saved_tensors[2], ref["seen"][:, None, :].expand(B, nh, T)
    o.backward(dO)
    o64.check(lse[seen], ref["lse"][seen], tw["lse"][seen], name="attn.cap.lse", note=note)
    assert bool((lse[~seen] == float("-inf")).all()) and not bool(x.grad[dead][:, :nh * hd].any()), note
    nq, nk = nh * hd, nkv * hd
    for name, sl in (("dq", slice(0, nq)), ("dk", slice(nq, nq + nk)), ("dv", slice(nq + nk, None))):
        o64.check(x.grad[:, sl], ref["dqkv"][:, sl], tw["dqkv"][:, sl], name="attn.cap." + name, note=note)


def test_gradient_at_ragged_T_is_refused():
    qkv, _ = inputs(1, 65, 2, 2, 64, False, 0)
    with pytest.raises(ValueError, match="T % 64"):
        ops.attention(qkv.requires_grad_(True), *tables(65, 64), 1, 65, 2, 2, 64, softcap=2.0)


def test_cap_is_live():
    B, T, nh, nkv, hd = 2, 128, 2, 2, 64
    qkv, _ = inputs(B, T, nh, nkv, hd, True, 3)
    with torch.no_grad():
        plain = ops.attention(qkv, *tables(T, hd), B, T, nh, nkv, hd)
    ref, tw = ac.oracle_and_twin(qkv, B, T, nh, nkv, hd, 1.0, ac.mask(B, T, DEV))
    with pytest.raises(AssertionError, match="outside the rule"):
        o64.check(plain, ref["o"], tw["o"], name="uncapped against the capped oracle")


@pytest.mark.parametrize("rep,hd,window,C", [(1, 32, None, 1.0), (2, 64, 40, 50.0), (8, 128, None, 50.0),
                                             (8, 64, 40, 1.0), (2, 128, None, 1.0), (1, 64, 40, 50.0)])
def test_decode(rep, hd, window, C):
    split = decode_split()
    nkv, B, s_max = 2, 2, 2 * split + 32
    nh = nkv * rep
    pos = torch.tensor([split - 1, split], dtype=torch.int32, device=DEV)  # a chunk's last slot, the next one's first
    g = torch.Generator().manual_seed(rep + hd)
    kc = torch.randn(B, nkv, s_max, hd, generator=g).to(DEV, BF16)
    vc = torch.randn(B, nkv, s_max, hd, generator=g).to(DEV, BF16)
    kc[0, :, 7] *= 20.0
    qkv = torch.randn(B, (nh + 2 * nkv) * hd, generator=g).to(DEV, BF16)
    k0, v0 = kc.clone(), vc.clone()
    out = attn_decode_launch(qkv, *tables(s_max, hd), pos, None, kc, vc, *decode_workspace(B, nh, hd, s_max, DEV),
                             nh, nkv, hd, window=window, softcap=C)

    def dense(dt):
        res = []
        for b in range(B):
            p, x = int(pos[b]), qkv[b].to(dt)
            lo = max(0, p - window + 1) if window else 0
            kk = torch.cat([k0[b, :, :p].to(dt), x[nh * hd:(nh + nkv) * hd].view(nkv, 1, hd)], dim=1)[:, lo:]
            vv = torch.cat([v0[b, :, :p].to(dt), x[(nh + nkv) * hd:].view(nkv, 1, hd)], dim=1)[:, lo:]
            z = C * torch.tanh((x[:nh * hd].view(nkv, rep, hd) @ kk.transpose(-1, -2)) * (hd ** -0.5 / C))
            res.append((torch.softmax(z, dim=-1) @ vv).reshape(nh * hd))
        return torch.stack(res)

    o64.check(out, dense(torch.float64), dense(torch.float32).bfloat16(), name="attn.cap.decode",
              note=f"rep={rep} hd={hd} window={window} C={C}")


def test_model_decode_matches_forward_and_trains():
    cfg = LlamaConfig.from_dict(dict(hidden_size=128, intermediate_size=256, num_attention_heads=4,
                                     num_key_value_heads=2, num_hidden_layers=2, vocab_size=512, rms_norm_eps=1e-5,
                                     max_position_embeddings=256, attn_logit_softcapping=2.0))
    m = LlamaForCausalLM(cfg, DEV, BF16).init_weights(7)
    B, T, n = 2, 16, 6
    ids = torch.randint(3, cfg.vocab_size, (B, T + n), generator=torch.Generator().manual_seed(11)).to(DEV)
    m.training = False
    with torch.no_grad():
        cache = m.new_cache(B, T + n)
        m.prefill(ids[:, :T], None, cache)
        for j in range(n):  # teacher forcing: token T + j goes in, the logits for T + j + 1 come out
            cached = m.decode_step(ids[:, T + j].contiguous(), cache).float()
            full = m(ids[:, :T + j + 1]).logits[:, -1].float()
            ops.set_backend("torch")  # the PyTorch path of every op on the same weights: the reference
            ref = m(ids[:, :T + j + 1]).logits[:, -1].float()
            ops.set_backend("hip")
            e_full, e_cached = float((full - ref).abs().max()), float((cached - ref).abs().max())
            assert e_cached <= 2.0 * e_full, (j, e_cached, e_full)  # the ratio test_generate_gpu.py allows
    m.training = True
    x = ids.repeat(1, 3)[:, :64]  # one training step's forward and backward (the capped backward: T % 64 == 0)
    loss = m(x, labels=x).loss
    loss.backward()
    q_grad = m.store.grad_view("model.layers.0.self_attn.q_proj.weight").float()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(q_grad).all()) and float(q_grad.abs().sum()) > 0
