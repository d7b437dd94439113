"""The fp8 KV cache on the GPU (csrc/attn_kv8.hip): the three writers bit for bit against ``ops.decode.kv8_quantize``,
``nd_attn_decode_kv8`` and ``nd_attn_extend_kv8`` per element against the float64 oracles of the bf16 kernels' tests on
the DEQUANTISED caches (the kernels' operands are exact, so rule and margin are theirs), invariance, the model.

Inputs: ``Step`` / ``State`` of test_decode_attn_gpu.py / test_extend_attn_gpu.py (spiked data, NaN in every slot
outside ``[kstart, pos)``) quantised with ``kv8_quantize``; a dead slot becomes the NaN code 0x7f with exponent 100.
The reference's new rows are ``kv8_dequantize(kv8_quantize(rotated row))``: the definition, not the kernel's output.
docs/PARITY.md ("fp8 KV cache") has the measured margins and logit differences."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import decode
from nanodiloco_amd.ops.attention import _rope, rope_cache

from . import _oracle64 as o64
from ._decode_oracle import _last_row_fp32, assemble, rotated_row
from ._frames import _ints, assert_frame_intact, framed_flat
from ._kv8 import edge_rows
from .test_decode_attn_gpu import HDS, HEADS, S, Step, pos_sets, rope_bits, s_max
from .test_extend_attn_gpu import State, oracle
from .test_generate_gpu import _config

pytestmark = pytest.mark.gpu
DEV, BF16 = "cuda", torch.bfloat16
REPORT = {}
quant, dequant = decode.kv8_quantize, decode.kv8_dequantize


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    yield
    ops.set_backend("auto")


@pytest.fixture(scope="module", autouse=True)
def _slack_report():
    yield
    for k in sorted(REPORT):
        print(f"\n[slack] {k}: needs margin {REPORT[k]:.3g} (allowed {o64.MARGIN})", end="")
    print()


def quant_cache(c):
    """A bf16 cache with NaN sentinels -> (codes, exps); the sentinel slots read code 0x7f, exponent 100."""
    q, e = quant(c)
    e[torch.isnan(c).any(-1)] = 100
    return q, e


# ------------------------------------------------------------------------------------------ the writers, bitwise
def write(writer, hd, qkv, cos, sin, c, nh, nkv, pos):
    L, pos_t = qkv.shape[0] // len(pos), torch.tensor(pos, dtype=torch.int32, device=DEV)
    if writer == "fill":
        return decode.kv8_fill_launch(qkv, *c, L, nh, nkv, hd)
    ws = (decode.decode_workspace if writer == "decode" else decode.extend_workspace)(len(pos), nh, hd, c[0].shape[2], DEV)
    if writer == "decode":
        return decode.attn_decode_kv8_launch(qkv, cos, sin, pos_t, None, *c, *ws, nh, nkv, hd)
    return decode.attn_extend_kv8_launch(qkv, cos, sin, pos_t, None, *c, *ws, L, nh, nkv, hd)


# rows per sequence and positions: the decode append, an extend append across a chunk edge, a fill of SPLIT + 1 rows
WRITERS = {"decode": (1, lambda: (S() - 1, 0, S())), "extend": (3, lambda: (S() - 2, 0)), "fill": (None, lambda: (0,))}


@pytest.mark.parametrize("writer", list(WRITERS))
@pytest.mark.parametrize("hd", HDS)
def test_writers_store_the_definitions_bits(hd, writer):
    L, pos = WRITERS[writer]
    pos, nh, nkv, sm = pos(), 8, 4, s_max()
    L, B = L or S() + 1, len(pos)
    torch.manual_seed(hd + L)
    qkv = o64.spiked(B * L, (nh + 2 * nkv) * hd, DEV).bfloat16()
    heads, edge = qkv.view(B * L, nh + 2 * nkv, hd), edge_rows(hd, DEV)
    heads[0, nh + nkv:], heads[1, nh + nkv:nh + nkv + 3] = edge[:4], edge[4:]  # v rows are stored as they come
    if writer == "fill":  # its k columns are rotated already: the edge rows reach the k cache too
        heads[-1, nh:nh + nkv], heads[-2, nh:nh + 3] = edge[:4], edge[4:]
    cos, sin = rope_cache(sm, hd, 10000.0, None, DEV)
    rot = qkv.clone()
    if writer != "fill":
        for b, p in enumerate(pos):
            _rope(rot[b * L:(b + 1) * L], cos[p:], sin[p:], 1, L, nh, nkv, hd, inverse=False)
    bigs, views = zip(*(framed_flat(B * nkv * sm * n, dt) for n, dt in ((hd, torch.uint8), (1, torch.int8)) * 2))
    kq, ke, vq, ve = (v.view(B, nkv, sm, -1) if i % 2 == 0 else v.view(B, nkv, sm) for i, v in enumerate(views))
    want = [b.clone() for b in bigs]
    for b, p in enumerate(pos):  # the expected buffers: the sentinel everywhere but in the written slots
        rows = rot[b * L:(b + 1) * L, nh * hd:].view(L, 2, nkv, hd).permute(1, 2, 0, 3)  # [k|v, nkv, L, hd]
        for j, (codes, exps) in enumerate((quant(rows[0]), quant(rows[1]))):
            want[2 * j][16:-16].view(B, nkv, sm, hd)[b, :, p:p + L] = codes
            want[2 * j + 1][16:-16].view(B, nkv, sm)[b, :, p:p + L] = exps
    write(writer, hd, qkv.clone(), cos, sin, (kq, ke, vq, ve), nh, nkv, pos)
    for name, got, exp in zip(("k codes", "k exps", "v codes", "v exps"), bigs, want):
        assert torch.equal(_ints(got), _ints(exp)), f"{name}: {int((_ints(got) != _ints(exp)).sum())} bytes differ"


# ------------------------------------------------------------------------------------------ decode against float64
def decode_case(st, window=None):
    """(out, ref64, twin32) of one fp8 decode step on ``Step`` st's quantised caches."""
    hd, nh, nkv = st.hd, st.nh, st.nkv
    (kq, ke), (vq, ve) = quant_cache(st.k), quant_cache(st.v)
    kd, vd = dequant(kq, ke, BF16), dequant(vq, ve, BF16)
    ref, twin = [], []
    for b, p in enumerate(st.pos):
        want = rotated_row(st.qkv[b], st.cos, st.sin, p, nh, nkv, hd).bfloat16()[0]
        assert torch.equal(_ints(want), _ints(rope_bits(st.qkv[b], st.cos, st.sin, p, nh, nkv, hd))), "pick another seed"
        ks = max(st.ks[b], p - window + 1) if window else st.ks[b]
        rows = assemble(st.qkv[b], kd[b], vd[b], p, ks, nh, nkv, hd, st.cos, st.sin)
        new = quant(rows[p, nh * hd:].view(2 * nkv, hd))
        rows[p, nh * hd:] = dequant(*new).double().view(-1)
        ref.append(o64.attention(rows, 1, p + 1, nh, nkv, hd, hd ** -0.5, kstart=torch.tensor([ks], device=DEV))["o"][-1])
        twin.append(_last_row_fp32(rows, ks, nh, nkv, hd, hd ** -0.5) if ks <= p else torch.zeros(nh * hd, device=DEV))
    o = decode.attn_decode_kv8_launch(st.qkv, st.cos, st.sin, st.pos_t, st.ks_t, kq, ke, vq, ve, st.part_o, st.part_ml,
                                      nh, nkv, hd, out=st.out, window=window)
    assert bool(torch.isfinite(o.float()).all()), "a sentinel slot was read"
    assert_frame_intact(st.obig, st.out.view(-1))
    return o, torch.stack(ref), torch.stack(twin)


@pytest.mark.parametrize("mode", ["null", "mid", "self"])
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("hd", HDS)
def test_decode_matches_oracle(hd, nh, nkv, mode):
    for i, pos in enumerate(pos_sets()):
        o, ref, twin = decode_case(Step(hd, nh, nkv, pos, mode, seed=i))
        o64.check(o, ref, twin, name="kv8.decode.o", report=REPORT, note=f"hd {hd} nh {nh} nkv {nkv} pos {pos} ({mode})")


def test_decode_window_starting_mid_chunk():
    for i, pos in enumerate(pos_sets()):
        o, ref, twin = decode_case(Step(64, 4, 2, pos, "zero", seed=i), window=S() // 2 + 3)
        o64.check(o, ref, twin, name="kv8.decode.window", report=REPORT, note=f"pos {pos}")


@pytest.mark.parametrize("i", range(3))
def test_decode_batch_invariant_and_deterministic(i):
    st = Step(64, 8, 1, pos_sets()[i], "mid")
    (kq, ke), (vq, ve) = quant_cache(st.k), quant_cache(st.v)

    def run(sl):
        c = [t[sl].clone() for t in (kq, ke, vq, ve)]
        po, pm = decode.decode_workspace(c[0].shape[0], 8, 64, st.SM, DEV)
        o = decode.attn_decode_kv8_launch(st.qkv[sl].clone(), st.cos, st.sin, st.pos_t[sl].clone(), st.ks_t[sl].clone(),
                                          *c, po, pm, 8, 1, 64)
        return [o] + c

    whole = run(slice(None))
    assert all(torch.equal(_ints(x), _ints(y)) for x, y in zip(whole, run(slice(None)))), "two runs differ"
    for b in range(st.B):
        assert all(torch.equal(_ints(x[b:b + 1]), _ints(y)) for x, y in zip(whole, run(slice(b, b + 1)))), f"sequence {b}"


# ------------------------------------------------------------------------------------------ extend against float64
def extend_launch(st, caches, qkv, L, pos_t):
    hd, nh, nkv, *_, window, _ = st.a
    return decode.attn_extend_kv8_launch(qkv, st.cos, st.sin, pos_t, st.ks_t, *caches, st.part_o, st.part_ml, L, nh, nkv,
                                         hd, window=window)


@pytest.mark.parametrize("L,mode", [(1, "null"), (33, "null"), (65, "null"), (33, "mid")])
@pytest.mark.parametrize("nh,nkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("hd", [64, 128])
def test_extend_matches_oracle(hd, nh, nkv, L, mode):
    assert decode.extend_qblock() + 1 == 65
    pos = (S() - (L + 1) // 2, 2 * S() - 1, 0)  # the new rows straddle a chunk edge (L = 1: sit on either side of one)
    st = State(hd, nh, nkv, L, pos, mode)
    (kq, ke), (vq, ve) = quant_cache(st.k), quant_cache(st.v)
    kd, vd = dequant(kq, ke, BF16), dequant(vq, ve, BF16)
    o = extend_launch(st, (kq, ke, vq, ve), st.qkv.clone(), L, st.pos_t)
    for b, (p, ks) in enumerate(zip(pos, st.ks)):
        rot, ob = st.rot[b * L:(b + 1) * L].clone(), o[b * L:(b + 1) * L]
        new = quant(rot[:, nh * hd:].reshape(L * 2 * nkv, hd))
        rot[:, nh * hd:] = dequant(*new, BF16).view(L, -1)
        ref, twin = (oracle(rot, kd[b], vd[b], p, ks, L, nh, nkv, hd, None, None, t) for t in (False, True))
        real = (p + torch.arange(L, device=DEV)) >= ks
        assert bool((ob[~real] == 0).all()), "a pad query must give zeros"
        o64.check(ob[real], ref[real], twin[real], name="kv8.extend.o", report=REPORT, note=f"b {b} pos {p}")


def test_extend_bits_do_not_depend_on_how_the_run_is_cut():
    hd, nh, nkv, L, pos = 64, 8, 1, 40, (S() - 8, 0, 2 * S() + 1)
    st = State(hd, nh, nkv, L, pos, "mid")
    base = quant_cache(st.k) + quant_cache(st.v)

    def run(cuts):
        caches, pos_t, out, t0 = [t.clone() for t in base], st.pos_t.clone(), [], 0
        for n in cuts:
            rows = st.qkv.view(3, L, -1)[:, t0:t0 + n].reshape(3 * n, -1).clone()
            out.append(extend_launch(st, caches, rows, n, pos_t).view(3, n, -1))
            pos_t += n
            t0 += n
        return [torch.cat(out, 1)] + caches

    assert all(torch.equal(_ints(x), _ints(y)) for x, y in zip(run([L]), run([7, 33])))


# ------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("name", ["tiny", "gqa"])
def test_generate_with_an_fp8_cache(name):
    cfg = _config(name)
    m = LlamaForCausalLM(cfg, DEV, BF16).init_weights(7)
    ids = torch.randint(3, cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(12)).to(DEV)
    mask = torch.ones(3, 9, dtype=torch.long, device=DEV)
    mask[0, :8] = 0
    mask[2, :4] = 0
    kw = dict(max_new_tokens=21, eos_token_id=None, return_logits=True)
    a, la = m.generate(ids, mask, hip_graph=False, kv_dtype="fp8", **kw)
    b, lb = m.generate(ids, mask, hip_graph=True, kv_dtype="fp8", **kw)
    assert torch.equal(a, b) and torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert bool(torch.isfinite(la).all())
    a16, l16 = m.generate(ids, mask, hip_graph=False, **kw)
    # printed, not asserted (it depends on the model): the steps at which both runs had drawn the same tokens so far
    same = torch.cat([torch.ones_like(a[:, :1]), (a[:, 9:-1] == a16[:, 9:-1]).long().cumprod(1)], 1).bool()
    print(f"\n[{name}] max |logits_fp8 - logits_bf16| over {int(same.sum())} of {same.numel()} steps on the same prefix: "
          f"{float(((la - l16).abs().amax(-1) * same).max()):.4f} (max |logits_bf16| {float(l16.abs().max()):.2f})")
    size = lambda c: sum(t.numel() * t.element_size() for ts in (c.k, c.v, c.k_exp or [], c.v_exp or []) for t in ts)
    assert size(m.new_cache(2, 40, kv_dtype="fp8")) * 2 * cfg.head_dim == size(m.new_cache(2, 40)) * (cfg.head_dim + 1)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_before_launch():
    st = Step(64, 4, 2, (3, 4, 5), "zero")
    (kq, ke), (vq, ve) = quant_cache(st.k), quant_cache(st.v)
    args = dict(qkv=st.qkv, cos=st.cos, sin=st.sin, pos=st.pos_t, kstart=st.ks_t, kcodes=kq, kexp=ke, vcodes=vq, vexp=ve,
                part_o=st.part_o, part_ml=st.part_ml, nh=4, nkv=2, hd=64)
    flat = torch.zeros(kq.numel() + 16, dtype=torch.uint8, device=DEV)
    wide = torch.zeros(3, 2, st.SM, 128, dtype=torch.uint8, device=DEV)
    bad = {"uint8": dict(kcodes=st.k), "int8": dict(vexp=ve.to(torch.uint8)), "aligned": dict(kcodes=flat[8:8 + kq.numel()].view_as(kq)),
           "contiguous": dict(vcodes=wide[..., :64]), "head_dim": dict(hd=48), "nh / nkv": dict(nh=36),
           "exponents": dict(kexp=ke[:, :, :-1].contiguous())}
    for match, kw in bad.items():
        with pytest.raises(ValueError, match=match):
            decode.attn_decode_kv8_launch(**{**args, **kw})
        with pytest.raises(ValueError, match=match):
            decode.attn_extend_kv8_launch(**{**args, **kw}, L=1)
    cfg = _config("gqa")
    cfg.attn_logit_softcapping = 5.0
    with pytest.raises(ValueError, match="softcapping"):
        ops.KVCache(cfg, 2, 16, DEV, BF16, kv_dtype="fp8")
