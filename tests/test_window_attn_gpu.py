"""Sliding-window attention (``nd_attn_fwd_win`` / ``nd_attn_bwd_fused_win``, ``ops.attention(window=)``) per element
against the float64 oracle, by the rule and with the inputs of ``test_attention_edges_gpu.py``.

The window reaches the oracle as a per-query lower bound (``_window_oracle.window_doc_start``): query q sees keys
max(kstart[b], q - W + 1) <= k <= q.  Rule (``_oracle64.check``): bf16 outputs within 2^-8 |ref64| + margin *
max|twin - ref64|, fp32 outputs within the slack alone, margin ``_oracle64.MARGIN`` (8); the slack unit is the twin's
distance from the oracle, never the kernel's.  Inputs are already-rotated bf16 rows with the spiked dO and the x20 late
key of that file's ``Case``.

W is drawn from {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, T - 1}: 1 = self only (every non-diagonal tile
skipped); W < 32 = rows with no key in a tile their wave processes; 33 = a wave's windows span two 32-key sub-tiles;
63 / 64 / 65 straddle a key tile; 127 / 128 / 129 straddle a query / key block and the dK/dV walk's end; 191 = an odd
tile count from an odd first tile.
"""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import _ext
from nanodiloco_amd.ops.attention import rope_cache, set_attn_fused_stats

from . import _oracle64 as o64
from ._frames import assert_frame_intact, framed, framed_flat
from ._window_oracle import window_doc_start
from .test_attention_edges_gpu import HDS, HEADS, bits_zero, case, ks_tensor, kstart_pairs, single_key_residue

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
TAG = "attn.win"
# per-output margins other than 8 (twice the measured ratio, rounded up to a power of two); docs/PARITY.md (sliding
# window table) has every measured ratio
MARGINS = {
    # measured 8.31 (0.31 once the oracle is fed the O the kernel stored; T = 128, W = 64, hd 32, the x20 key): the
    # cause of "attn.dq" in test_attention_edges_gpu.py,
    # unchanged by the window -- delta = rowsum(dO * O) reads O as the forward STORED it; where the kernel's O and the
    # oracle's fall on different sides of a bf16 rounding boundary, delta moves by 2^-8 |o_d| |dO_d|, 8 times more in
    # a spiked dO column, and dS = P (dP - delta) carries that to every key of the row, the x20 key included
    "attn.win.dq": 32.0,
}
REPORT = {}


def chk(out, ref64, twin, name, note=""):
    o64.check(out, ref64, twin, margin=MARGINS.get(name, o64.MARGIN), name=name, report=REPORT, note=note)


def judge(c, r, tw, o, lse, dqkv, tag, note="", rope_out=True):
    """``test_attention_edges_gpu.judge`` with this file's margins: the rule on every element of o, lse, dq, dk, dv;
    exact zeros / -inf on the fully masked rows (the set comes from the mask); all finite."""
    B, T, nh, nkv, hd = c.dims()
    nq, nk = nh * hd, nkv * hd
    seen = r["seen"]
    rows_seen = seen.reshape(-1)
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(dqkv.float()).all()), (tag, note)
    chk(o, r["o"], tw["o"], tag + ".o", note)
    seen_h = seen[:, None, :].expand(B, nh, T)
    chk(lse[seen_h], r["lse2"][seen_h], tw["lse2"][seen_h], tag + ".lse", note)
    assert bool((lse[~seen_h] == float("-inf")).all()), (tag, note, "stored LSE of a fully masked row")
    if int(r["mask"].sum(-1).max()) <= 1:  # W = 1: dS = dP - delta is exactly 0, see single_key_residue
        single_key_residue(c, r, dqkv, tag, note, rope_out, c.qkv)
    else:
        chk(dqkv[:, :nq], r["dq"], tw["dq"], tag + ".dq", note)
        chk(dqkv[:, nq:nq + nk], r["dk"], tw["dk"], tag + ".dk", note)
    chk(dqkv[:, nq + nk:], r["dv"], tw["dv"], tag + ".dv", note)
    if not bool(rows_seen.all()):
        assert bits_zero(o[~rows_seen]), (tag, note, "o of fully masked rows")
        assert bits_zero(dqkv[~rows_seen][:, nq + nk:]), (tag, note, "dv of fully masked rows")
        assert bits_zero(dqkv[~rows_seen][:, :nq + nk], any_sign=rope_out), (tag, note, "dq | dk of fully masked rows")


def judge_stats(c, r, o, ws, ds, tag, note):
    """The fused backward's workspace: -lse / c (c = scale log2 e; +inf on fully masked rows) and -delta, delta taken
    from dO and the o the forward saved (the oracle is given that o)."""
    B, T, nh, nkv, hd = c.dims()
    kw = dict(doc_start=ds, dO=c.dO, o_saved=o)
    d64 = o64.attention(c.qkv, *c.dims(), c.scale, **kw)["delta"]
    tw = o64.attention_twin(c.qkv, *c.dims(), c.scale, **kw)
    seen_h = r["seen"][:, None, :].expand(B, nh, T)
    cc = o64.f32_scalar(c.scale) * o64.LOG2E
    chk(ws[0][seen_h], -r["lse2"][seen_h] / cc, -tw["lse2"][seen_h] / torch.tensor(cc, device=DEV).float(),
        tag + ".ws_nl", note)
    assert bool((ws[0][~seen_h] == float("inf")).all()), (tag, note)
    chk(ws[1], -d64, -tw["delta"], tag + ".ws_nd", note)

WINDOWS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191]
DMA_T = [64, 128, 192, 320, 384]
REG_T = [1, 33, 65, 130, 200]


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    set_attn_fused_stats(True)
    yield
    ops.set_backend("auto")


@pytest.fixture(scope="module", autouse=True)
def _slack_report():
    yield
    for k in sorted(REPORT):
        if k.startswith(TAG):
            print(f"\n[slack] {k}: needs margin {REPORT[k]:.3g} (allowed {MARGINS.get(k, o64.MARGIN)})", end="")
    print()


def S():
    return _ext.stream_ptr(torch.device(DEV))


def dma_cases():
    """(T, W, hd, nh, nkv, spike): every T with every W < T of the list and T - 1; the head dimension, the GQA ratio
    and the late large key rotate across the pairs (not crossed)."""
    out, i = [], 0
    for T in DMA_T:
        for W in sorted({w for w in WINDOWS + [T - 1] if w < T}):
            out.append((T, W, HDS[i % 3], *HEADS[(i // 3 + i) % 3], i % 2 == 0))
            i += 1
    return out


def win_refs(c, W, ks=None, rope_out=True):
    ds = window_doc_start(c.B, c.T, W, DEV, ks)
    key = ("win", W, None if ks is None else tuple(ks.tolist()), rope_out)
    return c.refs(doc=(ds, None), rope_out=rope_out, key=key), ds


def run_ops(c, W, ks=None, rotated=True, qkv=None, dO=None):
    x = (c.qkv if qkv is None else qkv).clone().requires_grad_(True)
    o = ops.attention(x, c.cos, c.sin, *c.dims(), kstart=ks, rotated=rotated, window=W)
    lse = o.grad_fn.saved_tensors[2].clone()
    o.backward(c.dO if dO is None else dO)
    return o.detach(), lse, x.grad


def lse_bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------ LDS-DMA kernels
@pytest.mark.parametrize("T,W,hd,nh,nkv,spike", dma_cases())
def test_window_dma(T, W, hd, nh, nkv, spike):
    """Forward + fused backward at T % 64 == 0: o, lse, dq, dk, dv by the rule; a second run bitwise the first."""
    c = case(T, hd, nh, nkv, spike)
    (r, tw), _ = win_refs(c, W)
    assert bool(r["seen"].all())  # every query sees itself
    assert int(r["mask"].sum(-1).max()) == min(W, T)
    o, lse, g = run_ops(c, W)
    judge(c, r, tw, o, lse, g, TAG, f"W={W}")
    o2, lse2, g2 = run_ops(c, W)
    assert torch.equal(o, o2) and torch.equal(g, g2) and torch.equal(lse_bits(lse), lse_bits(lse2))


@pytest.mark.parametrize("T,W,hd,nh,nkv", [(192, 65, 64, 4, 2), (128, 32, 32, 4, 1), (192, 65, 128, 2, 2)])
def test_window_left_padding(T, W, hd, nh, nkv):
    """The window composed with a key start on both sides of a key tile, the last real token only, all pad: pad rows
    are bitwise +0 in o and dv, exact zeros in dq / dk, LSE -inf (``judge`` asserts them from the mask)."""
    c = case(T, hd, nh, nkv, True)
    for pair in kstart_pairs(T):
        ks = ks_tensor(pair)
        (r, tw), _ = win_refs(c, W, ks)
        o, lse, g = run_ops(c, W, ks)
        judge(c, r, tw, o, lse, g, TAG, f"W={W} kstart={pair}")
        if T in pair:  # an all-pad sequence: all zeros
            b = pair.index(T)
            assert bits_zero(o.view(2, T, -1)[b]) and bits_zero(g.view(2, T, -1)[b], any_sign=True)
            assert bool((lse[b] == float("-inf")).all())
        assert torch.equal(g, run_ops(c, W, ks)[2])


# ------------------------------------------------------------------------------------------ register-staged forward
def reg_cases():
    out, i = [], 0
    for T in REG_T:
        for W in (1, 32, 64, 65):
            if W < T:
                out.append((T, W, HDS[i % 3], *HEADS[(i // 3 + i) % 3], i % 2 == 0))
                i += 1
    return out


@pytest.mark.parametrize("T,W,hd,nh,nkv,spike", reg_cases())
def test_window_register_forward(T, W, hd, nh, nkv, spike):
    """T % 64 != 0: the register-staged forward with the per-score window term, under no_grad (prefill, evaluation);
    without and with a key start.  With a gradient required the call is refused and nothing is written."""
    c = case(T, hd, nh, nkv, spike)
    for pair in (None, (min(3, T - 1), 0)):
        ks = ks_tensor(pair)
        (r, tw), _ = win_refs(c, W, ks)
        with torch.no_grad():
            o = ops.attention(c.qkv.clone(), c.cos, c.sin, *c.dims(), kstart=ks, rotated=True, window=W)
        o64.check(o, r["o"], tw["o"], margin=o64.MARGIN, name=TAG + ".reg.o", report=REPORT, note=f"T={T} W={W} {pair}")
        if pair is not None:
            assert bits_zero(o[~r["seen"].reshape(-1)])
    x = c.qkv.clone().requires_grad_(True)
    before = x.detach().clone()
    with pytest.raises(ValueError):
        ops.attention(x, c.cos, c.sin, *c.dims(), rotated=True, window=W, inplace=True)
    assert torch.equal(x.detach(), before)


# ------------------------------------------------------------------------------------------ exact locality
def test_window_locality_exact():
    """T 256, W 64: a key / value row reaches exactly the 64 queries whose window holds it, a query's dO exactly the 64
    keys of its window -- bit for bit elsewhere (finite values only: a masked key's V row still meets an exact 0 in
    the MFMA)."""
    B, T, W, nh, nkv, hd = 2, 256, 64, 2, 1, 64
    c = case(T, hd, nh, nkv, False)
    nq, nk = nh * hd, nkv * hd
    o0, _, g0 = run_ops(c, W)
    x1 = c.qkv.clone()
    gen = torch.Generator(device=DEV).manual_seed(7)
    x1.view(B, T, -1)[:, 70, nq:] = torch.randn(B, 2 * nk, device=DEV, generator=gen).bfloat16()
    o1, _, _ = run_ops(c, W, qkv=x1)
    changed = (o0 != o1).view(B, T, -1).any(-1)
    inside = torch.zeros(T, dtype=torch.bool, device=DEV)
    inside[70:70 + W] = True
    assert not bool(changed[:, ~inside].any()), "a query outside 70..133 saw token 70"
    assert bool(changed[:, inside].all()), "a query of 70..133 did not see token 70"
    dO1 = c.dO.clone()
    dO1.view(B, T, -1)[:, 200] = torch.randn(B, nq, device=DEV, generator=gen).bfloat16()
    _, _, g1 = run_ops(c, W, dO=dO1)
    diff = (g0 != g1).view(B, T, -1)
    dq_rows, dk_rows, dv_rows = diff[..., :nq].any(-1), diff[..., nq:nq + nk].any(-1), diff[..., nq + nk:].any(-1)
    only200 = torch.zeros(T, dtype=torch.bool, device=DEV)
    only200[200] = True
    win200 = torch.zeros(T, dtype=torch.bool, device=DEV)
    win200[200 - W + 1:201] = True
    assert not bool(dq_rows[:, ~only200].any()) and bool(dq_rows[:, 200].all())
    for rows in (dk_rows, dv_rows):
        assert not bool(rows[:, ~win200].any()), "a key outside 137..200 got gradient from query 200"
        assert bool(rows[:, win200].all())


# ------------------------------------------------------------------------------------------ other checks
@pytest.mark.parametrize("T,hd,nh,nkv", [(128, 64, 4, 2), (192, 32, 2, 2), (65, 128, 4, 1), (1, 64, 2, 2)])
def test_window_not_below_T_is_no_window(T, hd, nh, nkv):
    """window >= T is not a window: today's un-windowed path, o and dqkv bit for bit (with a key start too)."""
    c = case(T, hd, nh, nkv, True)
    for ks in (None, ks_tensor((min(5, T), 0))):
        o0, lse0, g0 = run_ops(c, None, ks)
        for W in (T, T + 1, 4096):
            o, lse, g = run_ops(c, W, ks)
            assert torch.equal(o, o0) and torch.equal(g, g0) and torch.equal(lse_bits(lse), lse_bits(lse0)), W
    o, _, g = run_ops(c, 0)  # 0 = off
    assert torch.equal(o, run_ops(c, None)[0])


@pytest.mark.parametrize("hd", HDS)
def test_window_rotation_inside_equals_rotated_input(hd):
    from nanodiloco_amd.ops.attention import _rope
    B, T, nh, nkv, W = 2, 192, 4, 2, 65
    torch.manual_seed(hd)
    raw = torch.randn(B * T, (nh + 2 * nkv) * hd, device=DEV).bfloat16()
    dO = torch.randn(B * T, nh * hd, device=DEV).bfloat16()
    cos, sin = rope_cache(T, hd, 10000.0, None, DEV)
    x1 = raw.clone().requires_grad_(True)
    o1 = ops.attention(x1, cos, sin, B, T, nh, nkv, hd, window=W)
    o1.backward(dO)
    rot = raw.clone()
    _rope(rot, cos, sin, B, T, nh, nkv, hd, inverse=False)
    x2 = rot.clone().requires_grad_(True)
    o2 = ops.attention(x2, cos, sin, B, T, nh, nkv, hd, rotated=True, window=W)
    o2.backward(dO)
    assert torch.equal(o1, o2) and torch.equal(x1.grad, x2.grad)
    assert torch.equal(x1.detach(), raw)
    x3 = raw.clone().requires_grad_(True)
    assert not torch.equal(ops.attention(x3, cos, sin, B, T, nh, nkv, hd).detach(), o1.detach())  # the window bites


def raw_buffers(c, pad=16):
    B, T, nh, nkv, hd = c.dims()
    nq, n = nh * hd, B * nh * T
    bufs = {}
    bufs["x"] = framed(B * T, c.W, BF16, pad_c=pad)
    bufs["dO"] = framed(B * T, nq, BF16, pad_c=pad)
    bufs["o"] = framed(B * T, nq, BF16, pad_c=pad)
    bufs["g"] = framed(B * T, c.W, BF16, pad_c=pad)
    bufs["lse"] = framed_flat(n, F32)
    bufs["ws"] = framed_flat(2 * n, F32)
    bufs["x"][1].copy_(c.qkv)
    bufs["dO"][1].copy_(c.dO)
    return bufs


def raw_win(c, W, ks, rope_mode, bufs, fwd=True, bwd=True, fwd_tables=False, T_arg=None):
    """The raw launchers on the framed buffers; returns the two return codes (None: not called)."""
    B, T, nh, nkv, hd = c.dims()
    T = T if T_arg is None else T_arg
    L = _ext.lib()
    nq, nk = nh * hd, nkv * hd
    x, dO, o, g, lse, ws = (bufs[k][1] for k in ("x", "dO", "o", "g", "lse", "ws"))
    ld, ldo = x.stride(0), o.stride(0)
    k, v, gk, gv = x[:, nq:], x[:, nq + nk:], g[:, nq:], g[:, nq + nk:]
    cs = (c.cos.data_ptr(), c.sin.data_ptr())
    ksp = ks.data_ptr() if ks is not None else 0
    rf = rb = None
    if fwd:
        rf = L.nd_attn_fwd_win(x.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, nh, nkv, T, hd,
                               ld, ldo, *(cs if fwd_tables else (0, 0)), c.scale, ksp, W, S())
    if bwd:
        rb = L.nd_attn_bwd_fused_win(x.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dO.data_ptr(),
                                     lse.data_ptr(), g.data_ptr(), gk.data_ptr(), gv.data_ptr(), ws.data_ptr(), B, nh,
                                     nkv, T, hd, ld, ldo, *cs, c.scale, rope_mode, ksp, W, S())
    torch.cuda.synchronize()
    return rf, rb


@pytest.mark.parametrize("shape,W,pair,rope_mode", [((192, 64, 4, 2, True), 65, None, 2), ((320, 128, 4, 1, False), 129, (65, 0), 2),
                                                    ((128, 32, 2, 2, True), 31, (1, 0), 0), ((384, 64, 4, 1, True), 128, None, 0)])
def test_window_raw_strided_framed(shape, W, pair, rope_mode):
    """The raw entry points with ld / ldo wider than the rows: sentinel frames around o, lse, dqkv and ws survive; the
    rule on every output, the workspace statistics (-lse / c, -delta) included; the packed path gives the same bits."""
    c = case(*shape)
    B, T, nh, nkv, hd = c.dims()
    ks = ks_tensor(pair)
    rope_out = rope_mode == 2
    (r, tw), ds = win_refs(c, W, ks, rope_out=rope_out)
    bufs = raw_buffers(c)
    assert raw_win(c, W, ks, rope_mode, bufs) == (0, 0)
    for name in ("x", "dO", "o", "g", "lse", "ws"):
        assert_frame_intact(*bufs[name])
    assert torch.equal(bufs["x"][1], c.qkv)
    o, g = bufs["o"][1].contiguous(), bufs["g"][1].contiguous()
    lse, ws = bufs["lse"][1].view(B, nh, T), bufs["ws"][1].view(2, B, nh, T)
    judge(c, r, tw, o, lse, g, TAG, f"raw W={W} kstart={pair}", rope_out=rope_out)
    judge_stats(c, r, o, ws, ds, TAG, f"raw W={W} kstart={pair}")
    o1, lse1, g1 = run_ops(c, W, ks)
    assert torch.equal(o, o1) and torch.equal(lse_bits(lse), lse_bits(lse1))
    assert not rope_out or torch.equal(g, g1)


def test_window_refusals():
    """Every refusal comes before any launch: the buffers keep their bits."""
    c = case(128, 64, 4, 2, True)
    B, T, nh, nkv, hd = c.dims()
    t = torch.arange(T, device=DEV, dtype=torch.int32).expand(B, T).contiguous()
    x = c.qkv.clone().requires_grad_(True)
    with pytest.raises(ValueError):
        ops.attention(x, c.cos, c.sin, *c.dims(), rotated=True, inplace=True, window=32,
                      doc_bounds=(torch.zeros_like(t), torch.full_like(t, T)))
    with pytest.raises(ValueError):
        ops.attention(x, c.cos, c.sin, *c.dims(), rotated=True, inplace=True, window=-1)
    assert torch.equal(x.detach(), c.qkv)
    hd48 = 48
    y = torch.randn(B * T, (nh + 2 * nkv) * hd48, device=DEV).bfloat16()
    y0 = y.clone()
    cos48, sin48 = rope_cache(T, hd48, 10000.0, None, DEV)
    with pytest.raises(ValueError):
        ops.attention(y, cos48, sin48, B, T, nh, nkv, hd48, inplace=True, window=32)
    assert torch.equal(y, y0)
    # direct launcher calls
    bufs = raw_buffers(c)

    def untouched():
        for name in ("o", "g", "lse", "ws"):
            assert_frame_intact(bufs[name][0], None)

    assert raw_win(c, 0, None, 2, bufs)[0] != 0 and raw_win(c, 0, None, 2, bufs)[1] != 0  # window < 1
    assert raw_win(c, -3, None, 2, bufs, bwd=False)[0] != 0
    assert raw_win(c, 32, None, 2, bufs, bwd=False, fwd_tables=True)[0] != 0  # the forward takes rotated q|k only
    assert raw_win(c, 32, None, 1, bufs, fwd=False)[1] != 0                   # no rotation on load in the backward
    assert raw_win(c, 32, None, 2, bufs, fwd=False, T_arg=T - 1)[1] != 0     # no windowed backward at T % 64 != 0
    untouched()
    L = _ext.lib()
    o, lse, xx = bufs["o"][1], bufs["lse"][1], bufs["x"][1]
    assert L.nd_attn_fwd_win(xx.data_ptr(), xx.data_ptr(), xx.data_ptr(), o.data_ptr(), lse.data_ptr(), B, nh, nkv, T, 48,
                             xx.stride(0), o.stride(0), 0, 0, c.scale, 0, 32, S()) != 0  # head dim
    assert L.nd_attn_fwd_win(xx.data_ptr(), xx.data_ptr(), xx.data_ptr(), o.data_ptr(), lse.data_ptr(), B, 3, 2, T, hd,
                             xx.stride(0), o.stride(0), 0, 0, c.scale, 0, 32, S()) != 0  # nh % nkv
    assert L.nd_attn_fwd_win(xx.data_ptr(), xx.data_ptr(), xx.data_ptr(), o.data_ptr(), lse.data_ptr(), B, nh, nkv, T, hd,
                             xx.stride(0) + 4, o.stride(0), 0, 0, c.scale, 0, 32, S()) != 0  # misaligned ld
    torch.cuda.synchronize()
    untouched()
