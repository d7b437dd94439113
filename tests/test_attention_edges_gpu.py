"""The flash-attention kernels of ``csrc/attention.hip`` per element against a float64 oracle (T3).

Every forward and backward kernel -- LDS-DMA and register-staged, 128- and 256-row blocks, the three masking modes
(none, left padding ``kstart``, packed documents ``doc_bounds``), the fused and the unfused backward, rotation on
load (rope_mode 1) -- at the smallest shapes at which its launcher changes path.  References are
``_oracle64.attention`` (plain float64 from the math in the kernel header) and ``_oracle64.attention_twin`` (the same
math with the kernels' documented bf16 operand roundings); the rule is ``_oracle64.check``, unchanged:
  bf16 outputs (o, dq, dk, dv):  |out - ref64| <= 2^-8 |ref64| + margin * max|twin - ref64|, twin = the bf16-operand twin
  fp32 outputs (lse, delta, the fused path's workspace -lse/c and -delta):  slack only, twin = fp32 torch
with margin 8 except where ``MARGINS`` and docs/PARITY.md (T3, attention table) say why.  The unit of the slack is
the twin's distance from the oracle, never the kernel's.  Beside the rule: fully masked query rows give bitwise
+0 in o and dv, exact zeros in dq and dk (of either sign after the store epilogue's inverse rotation, +0 without it)
and a stored log-sum-exp of -inf (the epilogue's ``m + log2f(0)`` with ``m = -inf``), an all-pad sequence is all zeros,
rows that have a single key everywhere (T = 1) hold dq and dk to the fp32 cancellation residue (``single_key_residue``), a second backward is bitwise the first, the buffers' neighbours in memory survive (sentinel frames,
strides wider than the rows), and ``ops.attention`` with its own rotation equals the rotated-input path bitwise, so
every other case feeds already rotated bf16 values: the oracle's inputs are exactly the kernel's.

The A/B variants (register-staged forward, 8-wave blocks, plain softmax variant, deferred-max threshold 0, the
dK/dV prefetch depths, register-staged and 64-query dK/dV, the block orders) run under ``_switches.switches`` with
the same rule and margins.
"""
import functools

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import _ext
from nanodiloco_amd.ops.attention import rope_cache, set_attn_fused_stats

from . import _oracle64 as o64
from ._frames import assert_frame_intact, framed, framed_flat
from ._switches import switches
from .test_docmask_gpu import SETS, bounds, rows_for

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32

# per-output margins other than 8 (twice the measured ratio, rounded up to a power of two); docs/PARITY.md (T3,
# attention table) has every measured ratio
MARGINS = {
    # measured 9.32 (fused and unfused alike; T = 192, hd 32, the x20 key, kstart (64, 0)): delta = rowsum(dO * O) reads
    # O as the forward STORED it (attn_bwd_pre_kernel; the PRE branch of attn_bwd_dq_kernel).  Where the kernel's O and
    # the oracle's fall on different sides of a bf16 rounding boundary, delta moves by 2^-8 |o_d| |dO_d| -- 8 times
    # more in a spiked dO column -- and dS = P (dP - delta) carries that to every key of the row, the x20 key included.
    # The twin takes the same path, but its own flipped elements are few and in this draw none meets a dO spike.
    "attn.dq": 32.0,
    "attn.unfused.dq": 32.0,
    # measured 10.3 (T = 192, hd 32, kstart (1, 191)): the register-staged kernels rotate q and k on load (rope8) with
    # the expression of rope.hip, compiled separately with contraction allowed; a product fused into an fma on one side
    # only moves a rotated element across a bf16 rounding boundary in a few places per tensor, 2^-8 |q_d k_d| in one
    # score, against an fp32 twin that differs from the oracle by rounding of the sum alone
    "attn.rope1.lse": 32.0,
}
REPORT = {}


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    set_attn_fused_stats(True)
    yield
    set_attn_fused_stats(True)
    ops.set_backend("auto")


@pytest.fixture(scope="module", autouse=True)
def _slack_report():
    yield
    for k in sorted(REPORT):
        print(f"\n[slack] {k}: needs margin {REPORT[k]:.3g} (allowed {MARGINS.get(k, o64.MARGIN)})", end="")
    print()


def chk(out, ref64, twin, name, note=""):
    o64.check(out, ref64, twin, margin=MARGINS.get(name, o64.MARGIN), name=name, report=REPORT, note=note)


def S():
    return _ext.stream_ptr(torch.device(DEV))


# ------------------------------------------------------------------------------------------ cases
DMA_T = [64, 128, 192, 320, 384]  # LDS-DMA kernels: one key tile, a full block, odd tile counts 3 and 5, three blocks
REG_T = [1, 33, 65, 130, 200]     # register-staged kernels: one query, a tile's tail, a second tile's first row
HDS = [32, 64, 128]
HEADS = [(2, 2), (4, 2), (4, 1)]


def paired(ts):
    """(T, hd, nh, nkv, spike): every T with every head dimension, the GQA ratio and the late large key walking."""
    return [(T, hd, *HEADS[(i + j) % 3], (i + j) % 2 == 0) for i, T in enumerate(ts) for j, hd in enumerate(HDS)]


def kstart_pairs(T):
    """Both sides of a key tile, the last real token only, all pad: [B = 2] key starts, every value once."""
    vals = [(0, T), (1, T - 1), (63, 65), (64, 0)]
    return sorted({(max(0, min(a, T)), max(0, min(b, T))) for a, b in vals})


class Case:
    """Inputs (left unchanged) of one shape: rotated bf16 q|k|v, spiked dO, the tables."""

    def __init__(self, T, hd, nh, nkv, spike, B=2):
        self.B, self.T, self.hd, self.nh, self.nkv = B, T, hd, nh, nkv
        self.W = (nh + 2 * nkv) * hd
        self.scale = hd ** -0.5
        g = torch.Generator(device=DEV).manual_seed(1000 * T + hd + nh)
        x = torch.randn(B * T, self.W, device=DEV, generator=g)
        if spike:  # one late key row with large scores: the deferred-max rescale path
            x.view(B, T, self.W)[:, (3 * T) // 4, nh * hd:(nh + 1) * hd] *= 20
        self.qkv = x.bfloat16()
        torch.manual_seed(T + hd)
        self.dO = o64.spiked(B * T, nh * hd, DEV).bfloat16()
        self.cos, self.sin = rope_cache(T, hd, 10000.0, None, DEV)
        self._refs = {}

    def dims(self):
        return self.B, self.T, self.nh, self.nkv, self.hd

    def refs(self, ks=None, doc=None, rope_out=True, key=None):
        """(oracle, twin) of this case under a mask, computed once."""
        key = key if key is not None else (None if ks is None else tuple(ks.tolist()), rope_out)
        if key not in self._refs:
            kw = dict(kstart=ks, doc_start=doc[0] if doc is not None else None, dO=self.dO, rope_out=rope_out,
                      cos=self.cos, sin=self.sin)
            self._refs[key] = (o64.attention(self.qkv, *self.dims(), self.scale, **kw),
                               o64.attention_twin(self.qkv, *self.dims(), self.scale, **kw))
        return self._refs[key]


@functools.lru_cache(maxsize=None)
def case(T, hd, nh, nkv, spike):
    return Case(T, hd, nh, nkv, spike)


def ks_tensor(pair):
    return None if pair is None else torch.tensor(pair, dtype=torch.int32, device=DEV)


def run_ops(c, ks=None, doc=None):
    """ops.attention on the rotated rows: (o, lse as saved for the backward, dqkv)."""
    x = c.qkv.clone().requires_grad_(True)
    o = ops.attention(x, c.cos, c.sin, *c.dims(), kstart=ks, rotated=True, doc_bounds=doc)
    lse = o.grad_fn.saved_tensors[2].clone()
    o.backward(c.dO)
    return o.detach(), lse, x.grad


def bits_zero(t, any_sign=False):
    """Every element is +0 bit for bit (``any_sign``: +0 or -0)."""
    i = t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
    return not bool((i & 0x7FFF).any() if any_sign else i.any())


def judge(c, r, tw, o, lse, dqkv, tag, note="", rope_out=True, rows=None):
    """The rule on every element of o, lse, dq, dk, dv; exact zeros / -inf on the fully masked rows (the set comes
    from the mask); all finite."""
    B, T, nh, nkv, hd = c.dims()
    nq, nk = nh * hd, nkv * hd
    seen = r["seen"]                      # [B, T]
    rows_seen = seen.reshape(-1)
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(dqkv.float()).all()), (tag, note)
    chk(o, r["o"], tw["o"], tag + ".o", note)
    seen_h = seen[:, None, :].expand(B, nh, T)
    chk(lse[seen_h], r["lse2"][seen_h], tw["lse2"][seen_h], tag + ".lse", note)
    assert bool((lse[~seen_h] == float("-inf")).all()), (tag, note, "stored LSE of a fully masked row")
    if int(r["mask"].sum(-1).max()) <= 1:
        single_key_residue(c, r, dqkv, tag, note, rope_out, c.qkv if rows is None else rows)
    else:
        chk(dqkv[:, :nq], r["dq"], tw["dq"], tag + ".dq", note)
        chk(dqkv[:, nq:nq + nk], r["dk"], tw["dk"], tag + ".dk", note)
    chk(dqkv[:, nq + nk:], r["dv"], tw["dv"], tag + ".dv", note)
    if not bool(rows_seen.all()):  # left padding: pad queries see nothing, pad keys are seen by nothing
        assert bits_zero(o[~rows_seen]), (tag, note, "o of fully masked rows")
        assert bits_zero(dqkv[~rows_seen][:, nq + nk:]), (tag, note, "dv of fully masked rows")
        # dq and dk leave through the inverse rotation of the store epilogue (rope_mode 1 / 2), y2 c - y1 s on exact
        # zeros: an exact zero of either sign (+0 only without the rotation, rope_mode 0)
        assert bits_zero(dqkv[~rows_seen][:, :nq + nk], any_sign=rope_out), (tag, note, "dq | dk of fully masked rows")


def single_key_residue(c, r, dqkv, tag, note, rope_out, rows):
    """No query has more than one key (T = 1; one real token beside an all-pad sequence): P = 1 and
    dS = dP - delta = dO . v - dO . o with o = v, exactly 0.  The oracle and the twin are 0 to float64 rounding, so the
    twin's distance is no unit; what the kernels leave is the cancellation residue of two fp32 dot products of length
    hd summed in different orders, |dP - delta| <= 2 hd 2^-24 sum_d |dO_d v_d| (the standard bound gamma_hd of each),
    times P (1 to a few fp32 ulps), rounded to bf16 and multiplied by scale k (dq) or scale q, summed over the group
    (dk); 2^-6 covers the two bf16 roundings and P.  The inverse rotation mixes an element with its partner at
    i +- hd/2 with |cos|, |sin| <= 1: the bound of both."""
    B, T, nh, nkv, hd = c.dims()
    rep = nh // nkv
    x = rows.double().view(B, T, c.W)
    q = x[..., :nh * hd].view(B, T, nh, hd)
    k = x[..., nh * hd:(nh + nkv) * hd].view(B, T, nkv, hd).repeat_interleave(rep, 2)
    v = x[..., (nh + nkv) * hd:].view(B, T, nkv, hd).repeat_interleave(rep, 2)
    d = c.dO.double().view(B, T, nh, hd)
    res = 2 * hd * 2.0 ** -24 * (d * v).abs().sum(-1, keepdim=True) * r["seen"].double().view(B, T, 1, 1)
    lim_q = (1 + 2.0 ** -6) * c.scale * k.abs() * res
    lim_k = (1 + 2.0 ** -6) * c.scale * (q.abs() * res).view(B, T, nkv, rep, hd).sum(3)
    if rope_out:
        lim_q, lim_k = lim_q + lim_q.roll(hd // 2, -1), lim_k + lim_k.roll(hd // 2, -1)
    g = dqkv.double().view(B, T, c.W)
    for name, out, lim in (("dq", g[..., :nh * hd].view(B, T, nh, hd), lim_q),
                           ("dk", g[..., nh * hd:(nh + nkv) * hd].view(B, T, nkv, hd), lim_k)):
        worst = (out.abs() - lim).max().item()
        assert worst <= 0.0, (tag, note, name, "fp32 cancellation residue above its bound by", worst)


def masks_of(c, with_none=True):
    return ([None] if with_none else []) + kstart_pairs(c.T)


# ------------------------------------------------------------------------------------------ default path
@pytest.mark.parametrize("T,hd,nh,nkv,spike", paired(DMA_T + REG_T))
def test_default_path_kstart(T, hd, nh, nkv, spike):
    """ops.attention as the model calls it (rotated rows, rope_mode 2): the LDS-DMA forward and the fused backward at
    T % 64 == 0, the register-staged forward and the unfused register backward elsewhere; no mask and every key
    start; the backward twice, bitwise."""
    c = case(T, hd, nh, nkv, spike)
    for pair in masks_of(c):
        ks = ks_tensor(pair)
        r, tw = c.refs(ks)
        o, lse, g = run_ops(c, ks)
        judge(c, r, tw, o, lse, g, "attn", f"kstart={pair}")
        o2, lse2, g2 = run_ops(c, ks)
        assert torch.equal(o, o2) and torch.equal(g, g2) and torch.equal(lse.view(torch.int32), lse2.view(torch.int32))
        if pair is not None and T in pair:  # an all-pad sequence: all zeros; the other row was judged above
            b = pair.index(T)
            assert bits_zero(o.view(2, T, -1)[b]) and bits_zero(g.view(2, T, -1)[b], any_sign=True)
            assert bool((lse[b] == float("-inf")).all())


DOC_T = [64, 128, 192, 320]


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("T,hd,nh,nkv,spike", [p for p in paired(DOC_T) if (DOC_T.index(p[0]) + HDS.index(p[1])) % 3 != 2]
                         + [(320, 64, 4, 2, True)])
def test_default_path_documents(T, hd, nh, nkv, spike, name):
    """Packed documents (nd_attn_fwd_doc / nd_attn_bwd_fused_doc) under the boundary sets of test_docmask_gpu.py."""
    c = case(T, hd, nh, nkv, spike)
    doc = bounds(T, rows_for(T, 2, name))
    r, tw = c.refs(doc=doc, key=("doc", name))
    assert bool(r["seen"].all())  # every token sees itself
    o, lse, g = run_ops(c, doc=doc)
    judge(c, r, tw, o, lse, g, "attn.doc", name)
    o2, _, g2 = run_ops(c, doc=doc)
    assert torch.equal(o, o2) and torch.equal(g, g2)


@pytest.mark.parametrize("T,hd,nh,nkv,spike", paired(DMA_T))
def test_unfused_backward_dma(T, hd, nh, nkv, spike):
    """set_attn_fused_stats(False) at T % 64 == 0: nd_attn_bwd_pre, attn_neg_stats and the LDS-DMA dK/dV and dQ
    kernels (the register kernels at T % 64 != 0 are the default path there: test_default_path_kstart)."""
    c = case(T, hd, nh, nkv, spike)
    set_attn_fused_stats(False)
    for pair in masks_of(c):
        ks = ks_tensor(pair)
        r, tw = c.refs(ks)
        o, lse, g = run_ops(c, ks)
        judge(c, r, tw, o, lse, g, "attn.unfused", f"kstart={pair}")
        assert torch.equal(g, run_ops(c, ks)[2])


@pytest.mark.parametrize("hd", HDS)
def test_rotation_inside_equals_rotated_input(hd):
    """ops.attention(x) (which rotates) == ops.attention(nd_rope_inplace(x), rotated=True), output and gradient,
    bitwise: the rotation kernel has its own per-element test, everything here feeds rotated rows."""
    from nanodiloco_amd.ops.attention import _rope
    B, T, nh, nkv = 2, 192, 4, 2
    torch.manual_seed(hd)
    raw = torch.randn(B * T, (nh + 2 * nkv) * hd, device=DEV).bfloat16()
    dO = torch.randn(B * T, nh * hd, device=DEV).bfloat16()
    cos, sin = rope_cache(T, hd, 10000.0, None, DEV)
    x1 = raw.clone().requires_grad_(True)
    o1 = ops.attention(x1, cos, sin, B, T, nh, nkv, hd)
    o1.backward(dO)
    rot = raw.clone()
    _rope(rot, cos, sin, B, T, nh, nkv, hd, inverse=False)
    assert not torch.equal(rot, raw)
    x2 = rot.clone().requires_grad_(True)
    o2 = ops.attention(x2, cos, sin, B, T, nh, nkv, hd, rotated=True)
    o2.backward(dO)
    assert torch.equal(o1, o2) and torch.equal(x1.grad, x2.grad)
    assert torch.equal(x1.detach(), raw)  # the caller's tensor was not rotated


# ------------------------------------------------------------------------------------------ raw entry points
def raw_run(c, mode, ks=None, doc=None, qkv=None, pad=16):
    """The raw launchers on framed buffers with row strides wider than the rows (ld = W + 2 pad, ldo = nh hd + 2 pad,
    multiples of 8): forward, then the backward of ``mode`` -- "fused" (nd_attn_bwd_fused_ks / _doc, rope_mode 2),
    "fused0" (the same with rope_mode 0: no rotation of dq / dk), "unfused" (nd_attn_bwd_pre + nd_attn_bwd_ks,
    rope_mode 2), "rope1" (tables to the forward, rope_mode 1).
    Every frame must survive bit for bit.  Returns o, lse, dqkv, delta (unfused / rope1), ws [2, B, nh, T]."""
    B, T, nh, nkv, hd = c.dims()
    L = _ext.lib()
    nq, nk, n = nh * hd, nkv * hd, B * nh * T
    xbig, x = framed(B * T, c.W, BF16, pad_c=pad)
    x.copy_(c.qkv if qkv is None else qkv)
    dbig, dO = framed(B * T, nq, BF16, pad_c=pad)
    dO.copy_(c.dO)
    obig, o = framed(B * T, nq, BF16, pad_c=pad)
    gbig, g = framed(B * T, c.W, BF16, pad_c=pad)
    lbig, lse = framed_flat(n, F32)
    wbig, ws = framed_flat(2 * n, F32)
    ebig, delta = framed_flat(n, F32)
    ld, ldo = x.stride(0), o.stride(0)
    assert ld == c.W + 2 * pad and ldo == nq + 2 * pad and ld % 8 == 0 and ldo % 8 == 0
    k, v, gk, gv = x[:, nq:], x[:, nq + nk:], g[:, nq:], g[:, nq + nk:]
    rope1 = mode == "rope1"
    cs = (c.cos.data_ptr(), c.sin.data_ptr())
    ksp = ks.data_ptr() if ks is not None else 0
    if doc is not None:
        _ext.check(L.nd_attn_fwd_doc(x.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, nh, nkv,
                                     T, hd, ld, ldo, 0, 0, c.scale, doc[0].data_ptr(), doc[1].data_ptr(), S()), "fwd_doc")
    else:
        _ext.check(L.nd_attn_fwd_ks(x.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, nh, nkv,
                                    T, hd, ld, ldo, *(cs if rope1 else (0, 0)), c.scale, ksp, S()), "fwd_ks")
    if mode in ("fused", "fused0"):
        rm = 2 if mode == "fused" else 0
        if doc is not None:
            _ext.check(L.nd_attn_bwd_fused_doc(x.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dO.data_ptr(),
                                               lse.data_ptr(), g.data_ptr(), gk.data_ptr(), gv.data_ptr(), ws.data_ptr(),
                                               B, nh, nkv, T, hd, ld, ldo, *cs, c.scale, rm, doc[0].data_ptr(),
                                               doc[1].data_ptr(), S()), "bwd_fused_doc")
        else:
            _ext.check(L.nd_attn_bwd_fused_ks(x.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dO.data_ptr(),
                                              lse.data_ptr(), g.data_ptr(), gk.data_ptr(), gv.data_ptr(), ws.data_ptr(),
                                              B, nh, nkv, T, hd, ld, ldo, *cs, c.scale, rm, ksp, S()), "bwd_fused_ks")
    else:
        _ext.check(L.nd_attn_bwd_pre(o.data_ptr(), dO.data_ptr(), delta.data_ptr(), B, nh, T, hd, ldo, S()), "bwd_pre")
        _ext.check(L.nd_attn_bwd_ks(x.data_ptr(), k.data_ptr(), v.data_ptr(), dO.data_ptr(), lse.data_ptr(),
                                    delta.data_ptr(), g.data_ptr(), gk.data_ptr(), gv.data_ptr(), ws.data_ptr(), B, nh,
                                    nkv, T, hd, ld, ldo, *cs, c.scale, 1 if rope1 else 2, ksp, S()), "bwd_ks")
    torch.cuda.synchronize()
    assert_frame_intact(xbig, x)
    assert torch.equal(x, c.qkv if qkv is None else qkv)  # the inputs themselves are read only
    assert_frame_intact(dbig, dO)
    assert_frame_intact(obig, o)
    assert_frame_intact(gbig, g)
    assert_frame_intact(lbig, lse)
    uses_ws = mode in ("fused", "fused0") or (mode == "unfused" and T % 64 == 0)
    assert_frame_intact(wbig, ws if uses_ws else None)  # the register kernels take no workspace
    assert_frame_intact(ebig, delta if mode in ("unfused", "rope1") else None)
    return o.contiguous(), lse.view(B, nh, T), g.contiguous(), delta.view(B, nh, T), ws.view(2, B, nh, T)


def judge_stats(c, r, o, delta, ws, ks, doc, tag, note):
    """delta (its kernel's inputs are dO and the o the forward saved: the oracle takes that o) and the fused path's
    workspace, -lse / c (c = scale log2 e; +inf on fully masked rows) and -delta."""
    B, T, nh, nkv, hd = c.dims()
    kw = dict(kstart=ks, doc_start=doc[0] if doc is not None else None, dO=c.dO, o_saved=o)
    d64 = o64.attention(c.qkv, *c.dims(), c.scale, **kw)["delta"]
    tw = o64.attention_twin(c.qkv, *c.dims(), c.scale, **kw)
    if delta is not None:
        chk(delta, d64, tw["delta"], tag + ".delta", note)
    if ws is not None:
        seen_h = r["seen"][:, None, :].expand(B, nh, T)
        cc = o64.f32_scalar(c.scale) * o64.LOG2E
        chk(ws[0][seen_h], -r["lse2"][seen_h] / cc, -tw["lse2"][seen_h] / torch.tensor(cc, device=DEV).float(),
            tag + ".ws_nl", note)
        assert bool((ws[0][~seen_h] == float("inf")).all()), (tag, note)
        chk(ws[1], -d64, -tw["delta"], tag + ".ws_nd", note)


RAW = [  # mode, mask, (T, hd, nh, nkv, spike)
    ("fused", "none", (192, 64, 4, 2, True)), ("fused", "kstart", (320, 128, 4, 1, False)),
    ("fused", "kstart", (128, 32, 2, 2, True)), ("fused0", "kstart", (192, 64, 2, 2, False)),
    ("fused0", "doc", (64, 32, 2, 2, True)), ("fused", "doc", (192, 64, 4, 2, True)),
    ("fused", "doc", (128, 128, 2, 2, False)), ("unfused", "none", (128, 64, 4, 1, False)),
    ("unfused", "kstart", (192, 32, 4, 2, True)), ("unfused", "kstart", (130, 64, 4, 2, True)),
    ("unfused", "none", (65, 128, 2, 2, False)), ("unfused", "kstart", (33, 32, 4, 1, True)),
]


@pytest.mark.parametrize("mode,mask,shape", RAW)
def test_raw_strided_framed(mode, mask, shape):
    """Each mode through the raw entry points with ld and ldo wider than the rows: o, lse, dqkv, delta and the
    workspace framed; the same rule on every output, delta and the workspace included."""
    c = case(*shape)
    T = c.T
    ks = ks_tensor((65 if T > 65 else 1, 0)) if mask == "kstart" else None
    doc = bounds(T, rows_for(T, 2, "off_by_one")) if mask == "doc" else None
    fused, rope_out = mode != "unfused", mode != "fused0"
    r, tw = c.refs(ks, doc=doc, rope_out=rope_out, key=("doc", "off_by_one", rope_out) if doc is not None else None)
    o, lse, g, delta, ws = raw_run(c, mode, ks, doc)
    tag = "attn.unfused" if not fused else "attn.doc" if doc is not None else "attn"
    judge(c, r, tw, o, lse, g, tag, f"raw {mode} {mask}", rope_out=rope_out)
    judge_stats(c, r, o, None if fused else delta, ws if fused or T % 64 == 0 else None, ks, doc, tag, f"raw {mask}")
    # the packed path computes the same bits (strides do not change the arithmetic)
    set_attn_fused_stats(fused)
    o1, lse1, g1 = run_ops(c, ks, doc)
    assert torch.equal(o, o1) and torch.equal(lse.view(torch.int32), lse1.view(torch.int32))
    assert not rope_out or torch.equal(g, g1)


@pytest.mark.parametrize("T,hd,nh,nkv,spike", [p for i, p in enumerate(paired(DMA_T[:3] + REG_T)) if i % 3 == i // 3 % 3]
                         + [(200, 64, 4, 2, True)])
def test_rope_mode1_raw(T, hd, nh, nkv, spike):
    """Rotation on load (tables given to the forward, rope_mode 1 backward; always the register-staged kernels): the
    oracle's input is nd_rope_inplace of the same raw rows -- the kernels rotate with the same fp32 arithmetic and
    one rounding."""
    from nanodiloco_amd.ops.attention import _rope
    c = case(T, hd, nh, nkv, spike)
    raw = c.qkv  # the case's rows taken as the RAW projection here
    rot = raw.clone()
    _rope(rot, c.cos, c.sin, *c.dims(), inverse=False)
    for pair in [None, kstart_pairs(T)[1]]:
        ks = ks_tensor(pair)
        kw = dict(kstart=ks, dO=c.dO, rope_out=True, cos=c.cos, sin=c.sin)
        r = o64.attention(rot, *c.dims(), c.scale, **kw)
        tw = o64.attention_twin(rot, *c.dims(), c.scale, **kw)
        o, lse, g, delta, _ = raw_run(c, "rope1", ks, qkv=raw)
        judge(c, r, tw, o, lse, g, "attn.rope1", f"kstart={pair}", rows=rot)
        d64 = o64.attention(rot, *c.dims(), c.scale, kstart=ks, dO=c.dO, o_saved=o)["delta"]
        d32 = o64.attention_twin(rot, *c.dims(), c.scale, kstart=ks, dO=c.dO, o_saved=o)["delta"]
        chk(delta, d64, d32, "attn.rope1.delta", f"kstart={pair}")


# ------------------------------------------------------------------------------------------ A/B variants
VAR = [(128, 64, 4, 2, True), (192, 64, 2, 2, False), (320, 64, 4, 1, True), (128, 128, 2, 2, False)]


def variant_run(c, env, tag, fused=True, bitwise_default=False):
    """The full forward + backward of a case under ``switches(**env)``, without a mask and with left padding, by the
    same rule and margins as the default kernels."""
    for pair in (None, (63, 0)):
        ks = ks_tensor(pair)
        r, tw = c.refs(ks)
        set_attn_fused_stats(fused)
        if bitwise_default:
            o0, lse0, g0 = run_ops(c, ks)
        with switches(**env) as state:
            for k, v in env.items():
                assert state[k] == str(v), (k, v, state[k])
            o, lse, g = run_ops(c, ks)
            g2 = run_ops(c, ks)[2]
        judge(c, r, tw, o, lse, g, tag, f"{env} kstart={pair}")
        assert torch.equal(g, g2)
        if bitwise_default:
            assert torch.equal(o, o0) and torch.equal(g, g0) and torch.equal(lse, lse0), (env, pair)


@pytest.mark.parametrize("T,hd,nh,nkv,spike", VAR)
@pytest.mark.parametrize("env", [{"ND_ATTN_FWD": "r"}, {"ND_ATTN_FWD_W": "8"}, {"ND_ATTN_ABL": "0"}, {"ND_ATTN_ABL": "32"},
                                 {"ND_ATTN_THR": "0"}, {"ND_ATTN_FWD_W": "8", "ND_ATTN_ABL": "0"}],
                         ids=lambda e: "-".join(f"{k[8:]}{v}" for k, v in e.items()))
def test_variants_forward(T, hd, nh, nkv, spike, env):
    variant_run(case(T, hd, nh, nkv, spike), env, "attn.var_fwd")


@pytest.mark.parametrize("T,hd,nh,nkv,spike", VAR)
def test_variants_dq_w8(T, hd, nh, nkv, spike):
    variant_run(case(T, hd, nh, nkv, spike), {"ND_ATTN_DQ_W": "8"}, "attn.var_dq")


@pytest.mark.parametrize("T,hd,nh,nkv,spike", VAR)
@pytest.mark.parametrize("nb", ["2", "3", "4"])
def test_variants_dkdv_prefetch_depth(T, hd, nh, nkv, spike, nb):
    """64-query dK/dV tiles with NB LDS buffers: the same 32-query steps in the same order as the default kernel, so
    bitwise the default's gradients."""
    variant_run(case(T, hd, nh, nkv, spike), {"ND_ATTN_DKDV_NB": nb}, "attn.var_dkdv", bitwise_default=True)


@pytest.mark.parametrize("T,hd,nh,nkv,spike", VAR)
def test_variants_dkdv_w8(T, hd, nh, nkv, spike):
    variant_run(case(T, hd, nh, nkv, spike), {"ND_ATTN_DKDV_W": "8"}, "attn.var_dkdv")


@pytest.mark.parametrize("T,hd,nh,nkv,spike", VAR)
@pytest.mark.parametrize("env", [{"ND_ATTN_DKDV": "r"}, {"ND_DKDV_BQ": "64"}], ids=["DKDVr", "BQ64"])
def test_variants_dkdv_unfused(T, hd, nh, nkv, spike, env):
    """The register-staged dK/dV kernel and the 64-query LDS-DMA tiles: switches of the unfused backward."""
    variant_run(case(T, hd, nh, nkv, spike), env, "attn.var_dkdv", fused=False)


@pytest.mark.parametrize("T,hd,nh,nkv,spike", VAR)
@pytest.mark.parametrize("env", [{"ND_ATTN_ORDER": "0"}, {"ND_ATTN_ORDER": "1"}] +
                         [{"ND_ATTN_DKDV_ORDER": str(i)} for i in range(4)],
                         ids=lambda e: "-".join(f"{k[8:]}{v}" for k, v in e.items()))
def test_variants_block_order(T, hd, nh, nkv, spike, env):
    """The block-index maps of the three kernels (DKDV_ORDER bit 0 applies to MHA only, bit 1 walks the query tiles
    downwards: another fp32 accumulation order of dK / dV, the same rule)."""
    variant_run(case(T, hd, nh, nkv, spike), env, "attn.var_order")
