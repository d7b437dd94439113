"""``nd_attn_decode`` (csrc/attn_decode.hip) per element against the float64 decode oracle (``_decode_oracle``).

Shapes: S = ``nd_attn_decode_split()``, S_max = 3 S + 5 (four chunks, the last one of 5 keys), B = 3 with ragged
positions drawn from {0, 1, S-1, S, S+1, 2S+1, S_max-1}, hd 32 / 64 / 128, rep = nh / nkv 1, 2 and 8, and the key
starts null / 0 / mid-chunk / = pos (the query sees itself alone) / a whole chunk padded.  Inputs are spiked
(``_oracle64.spiked``) and one earlier key per sequence is scaled up, so that a dropped or doubled key shows.  Every
cache slot outside ``[kstart, pos)`` holds the NaN sentinel of ``_frames`` -- slot pos itself before the append, the
pad slots and everything beyond pos: a stray read shows as NaN, a stray write as a changed bit pattern.

The rule is ``_oracle64.check`` with margin 8 (docs/PARITY.md, decode table, has the measured ratios).  The oracle
rotates the new row in float64; the kernel (like ``nd_rope_inplace``) in fp32.  Where the two land on different
sides of a bf16 rounding boundary the oracle's INPUT would differ from the kernel's by a bf16 ulp, which no margin
on the output covers, so every case first asserts -- on ``nd_rope_inplace`` and the oracle alone, not on the kernel
under test -- that its seed gives the same rotated bits.
"""
import functools

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import _ext, decode
from nanodiloco_amd.ops.attention import _rope, rope_cache

from . import _oracle64 as o64
from ._decode_oracle import assemble, decode_refs, rotated_row
from ._frames import _PATTERN, _ints, assert_frame_intact, framed, framed_flat

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
REPORT = {}
MARGINS = {}


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
        print(f"\n[slack] {k}: needs margin {REPORT[k]:.3g} (allowed {MARGINS.get(k, o64.MARGIN)})", end="")
    print()


def chk(out, ref64, twin, name, note=""):
    o64.check(out, ref64, twin, margin=MARGINS.get(name, o64.MARGIN), name=name, report=REPORT, note=note)


@functools.lru_cache(None)
def S():
    return decode.decode_split()


def s_max():
    return 3 * S() + 5


def pos_sets():
    s, m = S(), s_max()
    return [(0, s, m - 1), (1, s - 1, 2 * s + 1), (s + 1, 0, s)]


KSTART_MODES = ["null", "zero", "mid", "self", "chunk"]


def kstart_for(mode, p):
    s = S()
    if mode in ("null", "zero"):
        return 0
    if mode == "mid":  # inside a chunk, keys on both sides of it
        return max(0, p - (s // 2 + 3))
    if mode == "self":
        return p
    return s if p >= s else p  # chunk 0 padded as a whole


def rope_bits(row, cos, sin, p, nh, nkv, hd):
    """``nd_rope_inplace`` on a copy of one packed row at position ``p``."""
    x = row.reshape(1, -1).clone()
    _rope(x, cos[p:], sin[p:], 1, 1, nh, nkv, hd, inverse=False)
    return x[0]


class Step:
    """One decode step's inputs: framed caches (live slots spiked data, every other slot the NaN sentinel), a framed
    strided qkv, device pos / kstart, the workspace."""

    def __init__(self, hd, nh, nkv, pos, mode, seed=0, B=None):
        self.hd, self.nh, self.nkv, self.pos, self.mode = hd, nh, nkv, list(pos), mode
        self.B = B = len(pos)
        self.SM = SM = s_max()
        self.W = W = (nh + 2 * nkv) * hd
        self.ks = [kstart_for(mode, p) for p in pos]
        torch.manual_seed(1000 * hd + 10 * nh + nkv + 7 * seed + sum(pos))
        n = B * nkv * SM * hd
        self.kbig, kflat = framed_flat(n, BF16)
        self.vbig, vflat = framed_flat(n, BF16)
        self.k, self.v = kflat.view(B, nkv, SM, hd), vflat.view(B, nkv, SM, hd)
        kd = o64.spiked(B * nkv * SM, hd, DEV).view(B, nkv, SM, hd)
        vd = o64.spiked(B * nkv * SM, hd, DEV, start=3).view(B, nkv, SM, hd)
        for b, (p, ks) in enumerate(zip(pos, self.ks)):
            if p > ks:
                kd[b, :, ks + (3 * (p - ks)) // 4] *= 3.0  # one earlier key with large scores
                self.k[b, :, ks:p] = kd[b, :, ks:p].bfloat16()
                self.v[b, :, ks:p] = vd[b, :, ks:p].bfloat16()
        self.qbig, self.qkv = framed(B, W, BF16)
        self.qkv.copy_(o64.spiked(B, W, DEV).bfloat16())
        self.cos, self.sin = rope_cache(SM, hd, 10000.0, None, DEV)
        self.pos_t = torch.tensor(pos, dtype=torch.int32, device=DEV)
        self.ks_t = None if mode == "null" else torch.tensor(self.ks, dtype=torch.int32, device=DEV)
        self.part_o, self.part_ml = decode.decode_workspace(B, nh, hd, SM, DEV)
        self.part_o.fill_(float("nan"))  # an unwritten partial must never be read
        self.obig, oflat = framed_flat(B * nh * hd, BF16)
        self.out = oflat.view(B, nh * hd)

    def refs(self):
        # precondition on the inputs (module doc): the oracle's rotated row has the bits nd_rope_inplace gives
        for b, p in enumerate(self.pos):
            want = rotated_row(self.qkv[b], self.cos, self.sin, p, self.nh, self.nkv, self.hd).bfloat16()[0]
            got = rope_bits(self.qkv[b], self.cos, self.sin, p, self.nh, self.nkv, self.hd)
            assert torch.equal(want.view(torch.int16), got.view(torch.int16)), \
                "float64 and fp32 rotation round differently for this draw: pick another seed"
        return decode_refs(self.qkv, self.k, self.v, self.pos, self.ks, self.nh, self.nkv, self.hd, self.cos, self.sin)

    def launch(self, out=None):
        return decode.attn_decode_launch(self.qkv, self.cos, self.sin, self.pos_t, self.ks_t, self.k, self.v,
                                         self.part_o, self.part_ml, self.nh, self.nkv, self.hd,
                                         out=self.out if out is None else out)

    def alone(self, b):
        """Sequence b as a batch of one, on copies."""
        st = Step.__new__(Step)
        st.__dict__.update(self.__dict__)
        st.B = 1
        st.k, st.v = self.k[b:b + 1].clone(), self.v[b:b + 1].clone()
        st.qkv = self.qkv[b:b + 1].clone()
        st.pos_t = self.pos_t[b:b + 1].clone()
        st.ks_t = None if self.ks_t is None else self.ks_t[b:b + 1].clone()
        st.part_o, st.part_ml = decode.decode_workspace(1, self.nh, self.hd, self.SM, DEV)
        st.out = torch.empty(1, self.nh * self.hd, dtype=BF16, device=DEV)
        return st


HDS = [32, 64, 128]
HEADS = [(4, 4), (4, 2), (8, 1)]


# ------------------------------------------------------------------------------------------ the error rule
@pytest.mark.parametrize("mode", KSTART_MODES)
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("hd", HDS)
def test_decode_matches_oracle(hd, nh, nkv, mode):
    for i, pos in enumerate(pos_sets()):
        st = Step(hd, nh, nkv, pos, mode, seed=i)
        ref, twin = st.refs()  # from the caches before the step
        o = st.launch()
        assert bool(torch.isfinite(o.float()).all()), "a sentinel slot was read"
        chk(o, ref, twin, "decode.o", note=f"hd {hd} nh {nh} nkv {nkv} pos {pos} kstart {st.ks} ({mode})")
        assert_frame_intact(st.obig, st.out.view(-1))


# ------------------------------------------------------------------------------------------ append
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("hd", HDS)
def test_append_writes_one_slot(hd, nh, nkv):
    for i, pos in enumerate(pos_sets()):
        st = Step(hd, nh, nkv, pos, "mid", seed=i)
        k0, v0, q0 = _ints(st.kbig).clone(), _ints(st.vbig).clone(), _ints(st.qbig).clone()
        st.launch()
        for b, p in enumerate(pos):
            rot = rope_bits(st.qkv[b], st.cos, st.sin, p, nh, nkv, hd)
            want_k = rot[nh * hd:(nh + nkv) * hd].view(nkv, hd)
            want_v = st.qkv[b, (nh + nkv) * hd:].view(nkv, hd)
            assert torch.equal(st.k[b, :, p].view(torch.int16), want_k.view(torch.int16)), (b, p)
            assert torch.equal(st.v[b, :, p].view(torch.int16), want_v.view(torch.int16)), (b, p)
            # back to the sentinel: whatever else differs from the snapshot is a stray write
            _ints(st.k)[b, :, p] = _PATTERN[2]
            _ints(st.v)[b, :, p] = _PATTERN[2]
        assert torch.equal(_ints(st.kbig), k0) and torch.equal(_ints(st.vbig), v0)
        assert torch.equal(_ints(st.qbig), q0), "the input row was modified"


# ------------------------------------------------------------------------------------------ batch invariance
@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 4), (64, 8, 1), (32, 4, 2), (128, 4, 2)])
def test_batch_invariant_and_deterministic(hd, nh, nkv):
    for i, pos in enumerate(pos_sets()):
        st = Step(hd, nh, nkv, pos, "mid", seed=i)
        singles = [st.alone(b) for b in range(st.B)]  # copies of the state before the step
        again = Step(hd, nh, nkv, pos, "mid", seed=i)
        o = st.launch().clone()
        o2 = again.launch()
        assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), "two runs differ"
        assert torch.equal(_ints(st.k), _ints(again.k)) and torch.equal(_ints(st.v), _ints(again.v))
        for b, one in enumerate(singles):
            ob = one.launch()
            assert torch.equal(ob.view(torch.int16), o[b:b + 1].view(torch.int16)), f"sequence {b} alone differs"


# ------------------------------------------------------------------------------------------ graph
def test_graph_replay_equals_eager():
    """A captured step (attention + ``pos += 1``) replayed for 3 consecutive positions that cross a chunk edge."""
    hd, nh, nkv = 64, 8, 2
    s = S()
    start = (s - 2, 2 * s - 1, 0)
    st = Step(hd, nh, nkv, start, "zero")
    rows = [o64.spiked(st.B, st.W, DEV, start=j).bfloat16() for j in range(3)]
    eager = Step(hd, nh, nkv, start, "zero")
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
        assert torch.equal(st.out.view(torch.int16), outs[j].view(torch.int16)), f"step {j}"
    torch.cuda.synchronize()
    assert torch.equal(st.pos_t, eager.pos_t)
    assert torch.equal(_ints(st.kbig), _ints(eager.kbig)) and torch.equal(_ints(st.vbig), _ints(eager.vbig))


# ------------------------------------------------------------------------------------------ training kernels
@pytest.mark.parametrize("T", [1, 65])
@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 4, 4), (32, 8, 1)])
def test_consistent_with_training_attention(T, hd, nh, nkv):
    """The last row of ``ops.attention`` on a packed window and the decode kernel on the cache built from the
    window's first T-1 rows both lie inside the rule of the same oracle.  The slack of each is its own documented
    twin's distance from that oracle: fp32 PyTorch for the decode kernel (fp32 VALU throughout), the bf16-operand
    twin ``_oracle64.attention_twin`` for the MFMA kernel (P rounded to bf16 before P V), as in
    test_attention_edges_gpu.py."""
    B = 2
    W = (nh + 2 * nkv) * hd
    torch.manual_seed(T + hd + nh)
    qkv = o64.spiked(B * T, W, DEV).bfloat16()
    cfgd = dict(hidden_size=nh * hd, num_attention_heads=nh, num_key_value_heads=nkv, head_dim=hd,
                num_hidden_layers=1, intermediate_size=64, vocab_size=64, max_position_embeddings=128)
    from nanodiloco_amd.config import LlamaConfig
    cache = ops.KVCache(LlamaConfig.from_dict(cfgd), B, 70, DEV, BF16)
    cos, sin = rope_cache(70, hd, 10000.0, None, DEV)
    rot = qkv.clone()
    _rope(rot, cos, sin, B, T, nh, nkv, hd, inverse=False)  # rows of a window: position = row % T
    if T > 1:
        first = rot.view(B, T, W)[:, :T - 1].reshape(B * (T - 1), W)
        ops.cache_fill(cache, 0, first, B, T - 1)
    cache.set_positions([T - 1] * B)
    last = qkv.view(B, T, W)[:, -1].contiguous()
    for b in range(B):
        want = rotated_row(last[b], cos, sin, T - 1, nh, nkv, hd).bfloat16()[0]
        assert torch.equal(want.view(torch.int16), rot.view(B, T, W)[b, -1].view(torch.int16)), "pick another seed"
    ref, twin = decode_refs(last, cache.k[0], cache.v[0], [T - 1] * B, None, nh, nkv, hd, cos, sin)
    o_dec = ops.attention_decode(last, cache, 0, cos, sin)
    o_trn = ops.attention(qkv, cos, sin, B, T, nh, nkv, hd).view(B, T, nh * hd)[:, -1]
    chk(o_dec, ref, twin, "decode.vs_training.decode", note=f"T {T}")
    twin_mfma = torch.stack([
        o64.attention_twin(assemble(last[b], cache.k[0][b], cache.v[0][b], T - 1, 0, nh, nkv, hd, cos, sin),
                           1, T, nh, nkv, hd, hd ** -0.5)["o"][-1] for b in range(B)])
    chk(o_trn, ref, twin_mfma, "decode.vs_training.training", note=f"T {T}")


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_before_launch():
    """Every refusal is raised in Python; nothing here reaches the device."""
    st = Step(64, 4, 2, (3, 4, 5), "zero")

    def launch(**kw):
        a = dict(qkv=st.qkv, cos=st.cos, sin=st.sin, pos=st.pos_t, kstart=st.ks_t, kcache=st.k, vcache=st.v,
                 part_o=st.part_o, part_ml=st.part_ml, nh=4, nkv=2, hd=64)
        a.update(kw)
        return decode.attn_decode_launch(**a)

    B, SM = st.B, st.SM
    with pytest.raises(ValueError, match="head_dim"):
        k48 = torch.zeros(B, 2, SM, 48, dtype=BF16, device=DEV)
        launch(hd=48, kcache=k48, vcache=k48.clone(), qkv=torch.zeros(B, 8 * 48, dtype=BF16, device=DEV))
    with pytest.raises(ValueError, match="nh / nkv"):
        k1 = torch.zeros(B, 1, SM, 64, dtype=BF16, device=DEV)
        launch(nh=16, nkv=1, kcache=k1, vcache=k1.clone(), qkv=torch.zeros(B, 18 * 64, dtype=BF16, device=DEV))
    with pytest.raises(ValueError, match="nh % nkv"):
        launch(nh=5, nkv=2, qkv=torch.zeros(B, 9 * 64, dtype=BF16, device=DEV))
    flat = torch.zeros(B * st.W + 8, dtype=BF16, device=DEV)
    with pytest.raises(ValueError, match="aligned"):
        launch(qkv=flat[1:1 + B * st.W].view(B, st.W))
    kflat = torch.zeros(st.k.numel() + 8, dtype=BF16, device=DEV)
    with pytest.raises(ValueError, match="aligned"):
        launch(kcache=kflat[4:4 + st.k.numel()].view_as(st.k))
    with pytest.raises(ValueError, match="contiguous"):
        launch(vcache=torch.zeros(B, 2, SM, 128, dtype=BF16, device=DEV)[..., :64])
    with pytest.raises(ValueError, match="stride"):
        launch(qkv=torch.zeros(B, st.W + 4, dtype=BF16, device=DEV)[:, :st.W])
    with pytest.raises(ValueError, match="table"):
        launch(cos=st.cos[:SM - 1])
    with pytest.raises(ValueError, match="workspace"):
        launch(part_o=st.part_o[:-1])
    # positions: the cache keeps a host-side bound, so a full cache is refused without reading the device
    from nanodiloco_amd.config import LlamaConfig
    cfg = LlamaConfig.from_dict(dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                                     num_hidden_layers=1, intermediate_size=64, vocab_size=64,
                                     max_position_embeddings=16))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        ops.KVCache(cfg, 2, 17, DEV, BF16)
    cache = ops.KVCache(cfg, 2, 16, DEV, BF16)
    with pytest.raises(ValueError, match="pos must lie"):
        cache.set_positions([3, 17])
    cache.set_positions([3, 16])  # sequence 1 is full
    cos, sin = rope_cache(16, 64, 10000.0, None, DEV)
    with pytest.raises(ValueError, match="full"):
        ops.attention_decode(torch.zeros(2, 8 * 64, dtype=BF16, device=DEV), cache, 0, cos, sin)
