"""``nd_attn_decode_win`` (csrc/attn_decode.hip): a decode step with a sliding window.

The partition of the key range depends on SPLIT and the key index alone, so the windowed step must be BITWISE the
plain step with the effective key start ``max(kstart, pos - W + 1)`` (``_window_oracle.kstart_eff``) -- in o and in
both caches.  Beside that: the float64 decode oracle with the same effective start under the rule of
``test_decode_attn_gpu.py`` (``_oracle64.check``, margin 8); every slot outside ``[kstart_eff, pos)`` holds the NaN
sentinel of ``_frames``, so a read of a chunk below the window shows; graph replay and batch invariance; the last row
of the windowed training forward lies inside the rule of the same oracle.

S_max 300 (three chunks of SPLIT = 128, the last of 44 keys); pos in {0, 1, 127, 128, 129, 255, 299};
W in {1, 32, 128, 129, 300}; hd 32 / 64 / 128; (nh, nkv) (4, 4), (8, 1), (4, 2); with and without a key start.
"""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.ops import decode
from nanodiloco_amd.ops.attention import _rope, rope_cache

from . import _oracle64 as o64
from ._decode_oracle import assemble, decode_refs, rotated_row
from ._frames import _PATTERN, _ints
from ._window_oracle import kstart_eff, window_doc_start
from .test_decode_attn_gpu import rope_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
SM = 300
POS = [0, 1, 127, 128, 129, 255, 299]
WINDOWS = [1, 32, 128, 129, 300]
HDS = [32, 64, 128]
HEADS = [(4, 4), (8, 1), (4, 2)]
REPORT = {}


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


def kstart_of(p, with_ks):
    """A key start inside the sequence: a third of the way to pos (0 for the first positions)."""
    return p // 3 if with_ks else 0


class Step:
    """One windowed decode step of B = len(POS) sequences, one per position.  Live slots [kstart_eff, pos) hold spiked
    data with one large earlier key; every other slot holds the NaN sentinel (``fill_below``: finite data in the slots
    below the window instead, for the never-read comparison)."""

    def __init__(self, hd, nh, nkv, W, with_ks, seed=0, fill_below=False, pos=POS):
        self.hd, self.nh, self.nkv, self.W = hd, nh, nkv, W
        self.pos = list(pos)
        self.B = B = len(self.pos)
        self.width = (nh + 2 * nkv) * hd
        self.ks = [kstart_of(p, with_ks) for p in self.pos]
        self.pos_t = torch.tensor(self.pos, dtype=torch.int32, device=DEV)
        self.ks_t = torch.tensor(self.ks, dtype=torch.int32, device=DEV) if with_ks else None
        self.lo = kstart_eff(self.pos_t, W, self.ks_t).tolist()
        torch.manual_seed(1000 * hd + 10 * nh + nkv + 7 * seed + W)
        self.k = torch.empty(B, nkv, SM, hd, dtype=BF16, device=DEV)
        self.v = torch.empty(B, nkv, SM, hd, dtype=BF16, device=DEV)
        _ints(self.k).fill_(_PATTERN[2])
        _ints(self.v).fill_(_PATTERN[2])
        kd = o64.spiked(B * nkv * SM, hd, DEV).view(B, nkv, SM, hd)
        vd = o64.spiked(B * nkv * SM, hd, DEV, start=3).view(B, nkv, SM, hd)
        for b, (p, lo, ks) in enumerate(zip(self.pos, self.lo, self.ks)):
            if p > lo:
                kd[b, :, lo + (3 * (p - lo)) // 4] *= 3.0
            first = ks if fill_below else lo
            self.k[b, :, first:p] = kd[b, :, first:p].bfloat16()
            self.v[b, :, first:p] = vd[b, :, first:p].bfloat16()
        self.qkv = o64.spiked(B, self.width, DEV).bfloat16()
        self.cos, self.sin = rope_cache(SM, hd, 10000.0, None, DEV)
        self.part_o, self.part_ml = decode.decode_workspace(B, nh, hd, SM, DEV)
        self.part_o.fill_(float("nan"))  # an unwritten partial must never be read
        self.out = torch.empty(B, nh * hd, dtype=BF16, device=DEV)

    def rotation_agrees(self):
        """The oracle's float64 rotation of the new rows has the bits ``nd_rope_inplace`` gives (a property of the
        draw, not of the kernel under test; see test_decode_attn_gpu.py)."""
        for b, p in enumerate(self.pos):
            want = rotated_row(self.qkv[b], self.cos, self.sin, p, self.nh, self.nkv, self.hd).bfloat16()[0]
            got = rope_bits(self.qkv[b], self.cos, self.sin, p, self.nh, self.nkv, self.hd)
            if not torch.equal(want.view(torch.int16), got.view(torch.int16)):
                return False
        return True

    def launch(self, window="own", kstart="own"):
        return decode.attn_decode_launch(self.qkv, self.cos, self.sin, self.pos_t,
                                         self.ks_t if kstart == "own" else kstart, self.k, self.v, self.part_o,
                                         self.part_ml, self.nh, self.nkv, self.hd, out=self.out,
                                         window=self.W if window == "own" else window)


def cases():
    """(hd, nh, nkv, W, with_ks): every W with and without a key start; hd and the heads rotate."""
    out = []
    for i, W in enumerate(WINDOWS):
        for j, with_ks in enumerate((False, True)):
            out.append((HDS[(i + j) % 3], *HEADS[(i + 2 * j) % 3], W, with_ks))
    return out + [(128, 8, 1, 32, True), (32, 4, 2, 129, False), (64, 4, 4, 128, True)]


def bits(t):
    return _ints(t)


@pytest.mark.parametrize("hd,nh,nkv,W,with_ks", cases())
def test_bitwise_twin_and_oracle(hd, nh, nkv, W, with_ks):
    """nd_attn_decode_win(kstart, W) == nd_attn_decode(max(kstart, pos - W + 1)) bit for bit, o and both caches; the
    oracle with that effective start; slots below the window hold NaN sentinels and the output is finite."""
    for seed in range(8):
        st = Step(hd, nh, nkv, W, with_ks, seed=seed)
        if st.rotation_agrees():
            break
    else:
        pytest.fail("no draw whose float64 and fp32 rotations agree")
    ref, twin = decode_refs(st.qkv, st.k, st.v, st.pos, st.lo, nh, nkv, hd, st.cos, st.sin)
    plain = Step(hd, nh, nkv, W, with_ks, seed=seed)
    assert torch.equal(bits(plain.k), bits(st.k)) and torch.equal(bits(plain.qkv), bits(st.qkv))
    o = st.launch().clone()
    o_plain = plain.launch(window=None, kstart=torch.tensor(st.lo, dtype=torch.int32, device=DEV)).clone()
    assert bool(torch.isfinite(o.float()).all()), "a slot outside the window was read"
    assert torch.equal(bits(o), bits(o_plain)), "windowed step differs from the plain step with the effective start"
    assert torch.equal(bits(st.k), bits(plain.k)) and torch.equal(bits(st.v), bits(plain.v))
    o64.check(o, ref, twin, margin=o64.MARGIN, name="decode.win.o", report=REPORT,
              note=f"hd {hd} nh {nh} nkv {nkv} W {W} kstart {st.ks}")
    # the append: slot pos holds the rotated k row and the v row
    for b, p in enumerate(st.pos):
        rot = rope_bits(st.qkv[b], st.cos, st.sin, p, nh, nkv, hd)
        assert torch.equal(bits(st.k[b, :, p]), bits(rot[nh * hd:(nh + nkv) * hd].view(nkv, hd)))
        assert torch.equal(bits(st.v[b, :, p]), bits(st.qkv[b, (nh + nkv) * hd:].view(nkv, hd)))


@pytest.mark.parametrize("hd,nh,nkv,W", [(64, 4, 2, 32), (128, 4, 4, 1), (32, 8, 1, 129)])
def test_below_window_never_read(hd, nh, nkv, W):
    """NaN sentinels in every slot below the window leave o finite and bitwise what finite data there gives."""
    nan = Step(hd, nh, nkv, W, True)
    fin = Step(hd, nh, nkv, W, True, fill_below=True)
    for b, (p, lo, ks) in enumerate(zip(nan.pos, nan.lo, nan.ks)):
        if lo > ks:
            assert bool(torch.isnan(nan.k[b, :, ks:lo].float()).all()) and bool(torch.isfinite(fin.k[b, :, ks:lo].float()).all())
    assert any(lo >= 128 for lo in nan.lo), "no chunk lies wholly below a window in this set"
    o_nan, o_fin = nan.launch().clone(), fin.launch().clone()
    assert bool(torch.isfinite(o_nan.float()).all())
    assert torch.equal(bits(o_nan), bits(o_fin))


def test_graph_replay_and_batch_invariance():
    """A captured windowed step (attention + ``pos += 1``) replayed over positions that cross a chunk edge equals the
    eager steps; a sequence alone gives the bits it gives in the batch."""
    hd, nh, nkv, W = 64, 8, 2, 32
    start = [126, 254, 0, 140]
    rows = [o64.spiked(len(start), (nh + 2 * nkv) * hd, DEV, start=j).bfloat16() for j in range(3)]

    def fresh():
        st = Step(hd, nh, nkv, W, False, pos=start)
        for b, p in enumerate(start):  # every slot a later step may see is finite
            st.k[b, :, max(0, p - W):p + 3] = torch.randn(nkv, min(p, W) + 3, hd, device=DEV,
                                                          generator=torch.Generator(DEV).manual_seed(b)).bfloat16()
            st.v[b, :, max(0, p - W):p + 3] = st.k[b, :, max(0, p - W):p + 3]
        return st

    eager, st = fresh(), fresh()
    outs = []
    for j in range(3):
        eager.qkv.copy_(rows[j])
        outs.append(eager.launch().clone())
        eager.pos_t += 1
    st.qkv.copy_(rows[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st.launch()
        st.pos_t += 1
    for j in range(3):
        st.qkv.copy_(rows[j])
        g.replay()
        assert torch.equal(bits(st.out), bits(outs[j])), f"step {j}"
    torch.cuda.synchronize()
    assert torch.equal(st.pos_t, eager.pos_t)
    assert torch.equal(bits(st.k), bits(eager.k)) and torch.equal(bits(st.v), bits(eager.v))
    # batch invariance
    full = Step(hd, nh, nkv, W, True)
    o = full.launch().clone()
    for b in (0, 3, 6):
        one = Step(hd, nh, nkv, W, True)
        o1 = decode.attn_decode_launch(one.qkv[b:b + 1].clone(), one.cos, one.sin, one.pos_t[b:b + 1].clone(),
                                       one.ks_t[b:b + 1].clone(), one.k[b:b + 1].clone(), one.v[b:b + 1].clone(),
                                       *decode.decode_workspace(1, nh, hd, SM, DEV), nh, nkv, hd, window=W)
        assert torch.equal(bits(o1), bits(o[b:b + 1])), f"sequence {b} alone differs"


@pytest.mark.parametrize("T,W", [(1, 1), (65, 32), (200, 64), (200, 129)])
@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 4, 4), (32, 8, 1)])
def test_consistent_with_windowed_training_forward(T, W, hd, nh, nkv):
    """The last row of the windowed ``ops.attention`` on a packed window (under no_grad: the register-staged forward
    at these T) and the windowed decode step on the cache built from its first T - 1 rows both lie inside the rule of
    the same oracle, each with its own documented twin (see test_decode_attn_gpu.py)."""
    B = 2
    width = (nh + 2 * nkv) * hd
    cfg = LlamaConfig.from_dict(dict(hidden_size=nh * hd, num_attention_heads=nh, num_key_value_heads=nkv, head_dim=hd,
                                     num_hidden_layers=1, intermediate_size=64, vocab_size=64,
                                     max_position_embeddings=256, sliding_window=W))
    cos, sin = rope_cache(210, hd, 10000.0, None, DEV)
    for seed in range(8):
        torch.manual_seed(T + hd + nh + 100 * seed)
        qkv = o64.spiked(B * T, width, DEV).bfloat16()
        rot = qkv.clone()
        _rope(rot, cos, sin, B, T, nh, nkv, hd, inverse=False)
        last = qkv.view(B, T, width)[:, -1].contiguous()
        if all(torch.equal(rotated_row(last[b], cos, sin, T - 1, nh, nkv, hd).bfloat16()[0].view(torch.int16),
                           rot.view(B, T, width)[b, -1].view(torch.int16)) for b in range(B)):
            break
    else:
        pytest.fail("no draw whose float64 and fp32 rotations agree")
    cache = ops.KVCache(cfg, B, 210, DEV, BF16)
    assert cache.window == W
    if T > 1:
        ops.cache_fill(cache, 0, rot.view(B, T, width)[:, :T - 1].reshape(B * (T - 1), width), B, T - 1)
    cache.set_positions([T - 1] * B)
    lo = max(0, T - W)
    ref, twin = decode_refs(last, cache.k[0], cache.v[0], [T - 1] * B, [lo] * B, nh, nkv, hd, cos, sin)
    o_dec = ops.attention_decode(last, cache, 0, cos, sin)
    with torch.no_grad():
        o_trn = ops.attention(qkv, cos, sin, B, T, nh, nkv, hd, window=W).view(B, T, nh * hd)[:, -1]
    o64.check(o_dec, ref, twin, margin=o64.MARGIN, name="decode.win.vs_training.decode", report=REPORT, note=f"T {T} W {W}")
    ds = window_doc_start(1, T, W, DEV)
    twin_mfma = torch.stack([
        o64.attention_twin(assemble(last[b], cache.k[0][b], cache.v[0][b], T - 1, lo, nh, nkv, hd, cos, sin),
                           1, T, nh, nkv, hd, hd ** -0.5, doc_start=ds)["o"][-1] for b in range(B)])
    o64.check(o_trn, ref, twin_mfma, margin=o64.MARGIN, name="decode.win.vs_training.training", report=REPORT,
              note=f"T {T} W {W}")


def test_window_refused_before_launch():
    st = Step(64, 4, 2, 32, False)
    before = bits(st.k).clone()
    for bad in (0, -1):
        with pytest.raises(ValueError, match="window"):
            st.launch(window=bad)
        with pytest.raises(ValueError, match="window"):
            decode.attention_decode_torch(st.qkv, st.cos, st.sin, st.pos_t, None, st.k, st.v, 4, 2, 64, window=bad)
    with pytest.raises(ValueError, match="head_dim"):  # the existing checks still run first
        k48 = torch.zeros(st.B, 2, SM, 48, dtype=BF16, device=DEV)
        decode.attn_decode_launch(torch.zeros(st.B, 8 * 48, dtype=BF16, device=DEV), st.cos, st.sin, st.pos_t, None,
                                  k48, k48.clone(), st.part_o, st.part_ml, 4, 2, 48, window=32)
    assert torch.equal(bits(st.k), before)
