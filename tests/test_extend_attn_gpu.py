"""``nd_attn_extend`` (csrc/attn_extend.hip) per element against a float64 oracle of L new rows on a KV cache.

S = ``decode_split()``, S_max = 3 S + 5, B = 3 with ragged positions.  ``oracle`` is plain float64 over the rotated bf16
rows; the twin handed to ``_oracle64.check`` is the same with the kernel's documented roundings (P to bf16 before P V,
o to bf16).  Spiked inputs, one earlier key scaled up; every cache slot outside ``[kstart, pos)`` and the workspace
hold NaN.  Rows whose float64 and fp32 rotations round to different bf16 bits are redrawn, then the equality is
asserted -- on ``nd_rope_inplace`` and the oracle alone, never on the kernel under test."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import decode
from nanodiloco_amd.ops.attention import _rope, rope_cache

from . import _oracle64 as o64
from ._frames import _ints, framed_flat

pytestmark = pytest.mark.gpu
DEV, BF16 = "cuda", torch.bfloat16


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    yield
    ops.set_backend("auto")


S = 128  # asserted against decode_split() in every case
SM = 3 * S + 5


# kstart: none / inside a chunk, keys on both sides / inside the new block (its first queries are pads) / chunk 0 padded
KSTART = {"null": lambda p, L: 0, "mid": lambda p, L: max(0, p - (S // 2 + 3)), "block": lambda p, L: p + min(3, L - 1),
          "chunk": lambda p, L: S if p >= S else p}


def rotate(qkv, cos, sin, pos, L, nh, nkv, hd):  # (float64 rotation rounded to bf16, nd_rope_inplace) at pos[b] + i
    want, got = [], qkv.clone()
    for b, p in enumerate(pos):
        want.append(o64.rope(qkv[b * L:(b + 1) * L], cos[p:], sin[p:], 1, L, nh, nkv, hd).bfloat16())
        _rope(got[b * L:(b + 1) * L], cos[p:], sin[p:], 1, L, nh, nkv, hd, inverse=False)
    return torch.cat(want), got


def oracle(rot, kc, vc, p, ks, L, nh, nkv, hd, window, cap, twin):
    """o [L, nh * hd] of one sequence in float64: cache slots [ks, p) and the L rotated rows ``rot``."""
    n, rep = p + L, nh // nkv
    q = rot[:, :nh * hd].double().view(L, nh, hd).transpose(0, 1)
    k = torch.cat([kc[:, :p].double(), rot[:, nh * hd:(nh + nkv) * hd].double().view(L, nkv, hd).transpose(0, 1)], 1)
    v = torch.cat([vc[:, :p].double(), rot[:, (nh + nkv) * hd:].double().view(L, nkv, hd).transpose(0, 1)], 1)
    t, hi = torch.arange(n, device=DEV), p + torch.arange(L, device=DEV)
    lo = torch.clamp(hi - window + 1, min=ks) if window else torch.full_like(hi, ks)
    ok = (t[None] >= lo[:, None]) & (t[None] <= hi[:, None])
    dead = (t < ks)[None, :, None]  # sentinel slots: exact-zero probabilities must not meet a NaN
    k, v = k.masked_fill(dead, 0.0).repeat_interleave(rep, 0), v.masked_fill(dead, 0.0).repeat_interleave(rep, 0)
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5
    if cap:
        s = cap * torch.tanh(s / cap)
    s = s.masked_fill(~ok, float("-inf"))
    m = s.amax(-1, keepdim=True)
    pr = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    l = pr.sum(-1, keepdim=True)
    o = ((pr.bfloat16().double() if twin else pr) @ v) / torch.where(l > 0, l, torch.ones_like(l))
    o = o.transpose(0, 1).reshape(L, nh * hd)
    return o.bfloat16().double() if twin else o


class State:
    """Caches (live slots spiked data, every other slot the NaN sentinel), rotation-safe qkv, positions, workspace."""

    def __init__(self, hd, nh, nkv, L, pos, mode="null", window=None, cap=None):
        assert decode.decode_split() == S and all(p + L <= SM for p in pos)
        self.a = (hd, nh, nkv, L, pos, mode, window, cap)
        B, W = len(pos), (nh + 2 * nkv) * hd
        self.ks = [KSTART[mode](p, L) for p in pos]
        torch.manual_seed(hd + 10 * nh + nkv + L + sum(pos))
        self.kbig, kf = framed_flat(B * nkv * SM * hd, BF16)
        self.vbig, vf = framed_flat(B * nkv * SM * hd, BF16)
        self.k, self.v = kf.view(B, nkv, SM, hd), vf.view(B, nkv, SM, hd)
        kd = o64.spiked(B * nkv * SM, hd, DEV).view(B, nkv, SM, hd)
        vd = o64.spiked(B * nkv * SM, hd, DEV, start=3).view(B, nkv, SM, hd)
        for b, (p, ks) in enumerate(zip(pos, self.ks)):
            if p > ks:
                kd[b, :, ks + (3 * (p - ks)) // 4] *= 3.0  # one earlier key with large scores
                self.k[b, :, ks:p] = kd[b, :, ks:p].bfloat16()
                self.v[b, :, ks:p] = vd[b, :, ks:p].bfloat16()
        self.cos, self.sin = rope_cache(SM, hd, 10000.0, None, DEV)
        self.qkv = o64.spiked(B * L, W, DEV).bfloat16()
        for _ in range(8):  # redraw the rows whose float64 and fp32 rotations round differently (module doc)
            want, got = rotate(self.qkv, self.cos, self.sin, pos, L, nh, nkv, hd)
            bad = (want.view(torch.int16) != got.view(torch.int16)).any(1)
            if not bool(bad.any()):
                break
            self.qkv[bad] = o64.spiked(int(bad.sum()), W, DEV).bfloat16()
        assert torch.equal(want.view(torch.int16), got.view(torch.int16)), "rotations still round differently"
        self.rot = got
        self.pos_t = torch.tensor(pos, dtype=torch.int32, device=DEV)
        self.ks_t = None if mode == "null" else torch.tensor(self.ks, dtype=torch.int32, device=DEV)
        self.part_o, self.part_ml = decode.extend_workspace(B, nh, hd, SM, DEV)
        self.part_o.fill_(float("nan"))
        self.part_ml.fill_(float("nan"))

    def launch(self, qkv=None, L=None, sl=slice(None)):
        hd, nh, nkv, L0, _, _, window, cap = self.a
        return decode.attn_extend_launch(self.qkv.clone() if qkv is None else qkv, self.cos, self.sin, self.pos_t[sl],
                                         None if self.ks_t is None else self.ks_t[sl], self.k[sl], self.v[sl],
                                         self.part_o, self.part_ml, L or L0, nh, nkv, hd, window=window, softcap=cap)


# hd, nh, nkv, L, pos, kstart mode, window, softcap: every value of every axis; window x kstart, softcap x window
CASES = [(64, 4, 4, 5, (0, S - 8, 2 * S + 1), "null", None, None),
         (32, 6, 2, 33, (S - 8, 0, S), "mid", None, None),            # the block straddles a chunk boundary
         (128, 8, 1, 70, (0, S, 2 * S + 1), "null", None, None),      # two attention launches
         (64, 6, 2, 32, (SM - 32, S, 0), "chunk", None, None),        # ends exactly at S_max
         (128, 4, 4, 1, (0, S, 2 * S + 1), "null", S + 2, None),
         (32, 8, 1, 33, (S, S - 8, 2 * S + 1), "block", None, 5.0),
         (64, 8, 1, 70, (2 * S + 1, S, S - 8), "mid", 8, None),       # window x kstart, window < L
         (128, 6, 2, 5, (2 * S + 1, S, S - 8), "chunk", S + 2, 5.0),  # softcap x window, crossing a chunk
         (64, 4, 4, 32, (S - 8, 0, S), "block", 8, 5.0)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_extend_matches_oracle_and_appends(case):
    hd, nh, nkv, L, pos, mode, window, cap = case
    st = State(*case)
    k0, v0 = _ints(st.kbig).clone(), _ints(st.vbig).clone()
    o = st.launch()
    for b, (p, ks) in enumerate(zip(pos, st.ks)):
        rot, ob = st.rot[b * L:(b + 1) * L], o[b * L:(b + 1) * L]
        ref, twin = (oracle(rot, st.k[b], st.v[b], p, ks, L, nh, nkv, hd, window, cap, t) for t in (False, True))
        real = (p + torch.arange(L, device=DEV)) >= ks
        assert bool((ob[~real] == 0).all()), "a pad query must give zeros"
        o64.check(ob[real], ref[real], twin[real], name="extend.o", note=f"{case} b {b}")
        for c, new in ((st.k, rot[:, nh * hd:(nh + nkv) * hd]), (st.v, rot[:, (nh + nkv) * hd:])):  # the append, bitwise
            assert torch.equal(_ints(c[b, :, p:p + L].contiguous()), _ints(new.reshape(L, nkv, hd).transpose(0, 1).contiguous()))
    for b, p in enumerate(pos):  # restore the snapshot's bits in the appended slots, then compare everything
        _ints(st.k)[b, :, p:p + L] = k0[16:-16].view(st.k.shape)[b, :, p:p + L]
        _ints(st.v)[b, :, p:p + L] = v0[16:-16].view(st.v.shape)[b, :, p:p + L]
    assert torch.equal(_ints(st.kbig), k0) and torch.equal(_ints(st.vbig), v0), "a stray cache write"


@pytest.mark.parametrize("case", [(64, 6, 2, 48, (S - 8, 0, 2 * S + 1), "mid", None, None),
                                  (128, 8, 1, 48, (S, S - 40, 2 * S + 1), "block", S + 2, 5.0)])
def test_bits_do_not_depend_on_how_the_run_is_cut(case):
    hd, nh, nkv, L, pos, *_ = case
    base = State(*case)

    def run(cuts, b=None):
        st = State.__new__(State)
        st.__dict__.update(base.__dict__)
        sl = slice(None) if b is None else slice(b, b + 1)
        st.k, st.v, st.pos_t = base.k.clone(), base.v.clone(), base.pos_t.clone()
        rows = base.qkv.view(len(pos), L, -1)[sl]
        out, t0 = [], 0
        for n in cuts:
            out.append(st.launch(rows[:, t0:t0 + n].reshape(rows.shape[0] * n, -1).clone(), n, sl).view(-1, n, nh * hd))
            st.pos_t += n
            t0 += n
        return torch.cat(out, 1), st.k[sl], st.v[sl]

    whole = run([L])
    for other in (run([16, 32]), run([1] * L)):
        assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(whole, other))
    alone = run([L], b=1)
    assert all(torch.equal(x[1:2].view(torch.int16), y.view(torch.int16)) for x, y in zip(whole, alone))


def test_agrees_with_the_training_attention():
    hd, nh, nkv, T = 64, 6, 2, 128
    st = State(hd, nh, nkv, T, (0, 0, 0))
    ref, twin = (torch.cat([oracle(st.rot[b * T:(b + 1) * T], st.k[b], st.v[b], 0, 0, T, nh, nkv, hd, None, None, t)
                            for b in range(3)]) for t in (False, True))
    train = ops.attention(st.qkv.clone(), st.cos, st.sin, 3, T, nh, nkv, hd)
    rows = st.qkv.view(3, T, -1)
    a = st.launch(rows[:, :50].reshape(150, -1).clone(), 50).view(3, 50, -1)
    st.pos_t += 50
    b = st.launch(rows[:, 50:].reshape(234, -1).clone(), 78).view(3, 78, -1)
    for name, o in (("extend.vs_train.extend", torch.cat([a, b], 1).reshape(3 * T, -1)), ("extend.vs_train.train", train)):
        o64.check(o, ref, twin, name=name)


def test_refusals_before_any_launch():
    st = State(64, 4, 4, 5, (0, 1, 2))
    args = dict(qkv=st.qkv, cos=st.cos, sin=st.sin, pos=st.pos_t, kstart=None, kcache=st.k, vcache=st.v,
                part_o=st.part_o, part_ml=st.part_ml, L=5, nh=4, nkv=4, hd=64)
    bad = [dict(qkv=st.qkv.float()), dict(qkv=st.qkv[:, ::2]), dict(qkv=st.qkv[:14]), dict(pos=st.pos_t.long()),
           dict(cos=st.cos.double()), dict(kcache=st.k.transpose(1, 2)), dict(part_o=st.part_o[:8]), dict(L=SM + 1),
           dict(nh=36, nkv=4, kcache=st.k[:, :4]), dict(hd=48), dict(window=0), dict(softcap=-1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            decode.attn_extend_launch(**{**args, **kw})
    cache = ops.KVCache(type("C", (), dict(num_attention_heads=4, num_key_value_heads=4, head_dim=64, num_hidden_layers=1,
                                           max_position_embeddings=SM)), 3, SM, DEV, BF16)
    cache.set_positions([0, 1, SM - 4])
    with pytest.raises(ValueError, match="full"):
        ops.attention_extend(st.qkv, cache, 0, st.cos, st.sin, 5)
