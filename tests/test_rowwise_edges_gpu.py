"""Edge shapes of the row-wise and streaming HIP kernels against float64 oracles, per element (T3).

``csrc/norm.hip``, ``rope.hip``, ``swiglu.hip``, ``cross_entropy.hip``, ``embedding.hip``, ``optim.hip`` and
``transpose.hip`` at the shapes where their launchers change path: every chunk count of the RMSNorm dispatch,
column counts that are no multiple of a chunk, one to a few rows, every grid cap wrapped once, the scalar tails of
the optimizer streams, the dispatch borders of the cross-entropy kernels, fp32 paths, out-of-range ids, partial
transpose tiles.  References are ``tests/_oracle64.py``; the error rule is ``_oracle64.check`` (bf16 outputs: half
an ulp relative plus slack, fp32 outputs: slack, slack = margin x the error of the fp32 PyTorch twin computed
here on the same inputs; margin 8 except where ``MARGINS`` and the table in docs/PARITY.md say why).  Kernels that
write in place or into views also run on an operand framed by a sentinel bit pattern that must survive.

RMSNorm dtype combinations (x/h, a, y; the backward's dy has y's dtype, its branch gradient a's):
  no residual add: fp32 -> bf16, fp32 -> fp32, bf16 -> bf16 (``rmsnorm`` and, with dres, ``rmsnorm_res``);
  with the add:    fp32 + bf16 -> bf16, fp32 + fp32 -> fp32, fp32 + fp32 -> bf16, bf16 + bf16 -> bf16.
Unreachable through ``ops``: the backward's fp32 dy with a bf16 branch gradient (it needs the forward
fp32 + bf16 -> fp32, which ``nd_rmsnorm_fwd`` refuses), and the bf16-residual backward with a branch gradient that
is not dx itself.
"""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import _ext
from nanodiloco_amd.ops import reference as ref

from . import _oracle64 as o64
from ._switches import switches
from ._frames import _PATTERN, _ints, assert_frame_intact, framed, framed_flat  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16

# per-output margins other than 8 (twice the measured ratio, rounded up to a power of two); docs/PARITY.md (T3, slack
# table) has every measured ratio
MARGINS = {
    # measured 70.3: v_fma_f32 x * log2(e) - lse2 feeds v_exp_f32 with lse2 carrying the rounding of m * log2(e)
    # (half an ulp of 86.6 at |x| = 60: p off by 2.6e-6 relative), which shows where softmax - 1 cancels to 0
    "ce_bf16.dlogits": 256.0,
    # measured 8.95 / 8.63: __expf = v_mul_f32 by log2(e) + v_exp_f32; the product's rounding scales with |x - lse|
    "ce_reg4.dlogits": 32.0,
    "ce_reg16.dlogits": 32.0,
}
REPORT = {}


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    torch.manual_seed(0)
    yield
    ops.set_backend("auto")


@pytest.fixture(scope="module", autouse=True)
def _slack_report():
    yield
    for k in sorted(REPORT):
        print(f"\n[slack] {k}: needs margin {REPORT[k]:.3g} (allowed {MARGINS.get(k, o64.MARGIN)})", end="")
    print()


def chk(out, ref64, twin32, name, note=""):
    o64.check(out, ref64, twin32, margin=MARGINS.get(name, o64.MARGIN), name=name, report=REPORT, note=note)


class torch_twin:
    """``with torch_twin():`` the same ``ops.*`` call takes its PyTorch path on the GPU tensors."""

    def __enter__(self):
        ops.set_backend("torch")

    def __exit__(self, *exc):
        ops.set_backend("hip")
        return False


def S():
    return _ext.stream_ptr(torch.device(DEV))


# ------------------------------------------------------------------------------------------ RMSNorm
NORM_COLS = [8, 72, 512, 520, 1032, 1536, 2056, 4096]
NORM_ROWS = [1, 3, 67, 257]
NORM_COMBOS = [  # mode, residual dtype, branch dtype, y dtype
    ("plain", F32, None, BF16), ("plain", F32, None, F32), ("plain", BF16, None, BF16),
    ("res", F32, None, BF16), ("res", BF16, None, BF16),
    ("add", F32, BF16, BF16), ("add", F32, F32, F32), ("add", F32, F32, BF16), ("add", BF16, BF16, BF16),
]


def _norm_case(mode, hdt, adt, ydt, rows, cols, eps=1e-5):
    h = o64.spiked(rows, cols, DEV).to(hdt)
    a = o64.spiked(rows, cols, DEV, 0.5, start=3).to(adt) if mode == "add" else None
    w = 1 + 0.1 * torch.randn(cols, device=DEV)
    dy = o64.spiked(rows, cols, DEV, 1.0, start=5).to(ydt)
    dres = torch.randn(rows, cols, device=DEV).to(hdt) if mode != "plain" else None
    gw0 = torch.randn(cols, device=DEV)
    gw = gw0.clone()
    hx = h.clone().requires_grad_(True)
    ax = hn = None
    if mode == "plain":
        y = ops.rmsnorm(hx, w, gw, eps, ydt)
        y.backward(dy)
    elif mode == "res":
        y, hn = ops.rmsnorm_res(hx, w, gw, eps, ydt)
        torch.autograd.backward((y, hn), (dy, dres))
    else:
        ax = a.clone().requires_grad_(True)
        y, hn = ops.add_rmsnorm(hx, ax, w, gw, eps, ydt)
        torch.autograd.backward((y, hn), (dy, dres))
    rounded = mode == "add" and hdt == BF16
    r = o64.rmsnorm(h, w, eps, a=a, round_hnew=rounded, dy=dy, dres=dres)
    # the fp32 twin on the same inputs
    hn32 = h.float() + a.float() if a is not None else h.float()
    if rounded:
        hn32 = hn32.bfloat16().float()
    y32 = ref.rmsnorm(hn32, w, eps)
    dx32, dw32 = ref.rmsnorm_backward(dy.float(), hn32, w, eps)
    if dres is not None:
        dx32 = dx32 + dres.float()
    rstd32 = torch.rsqrt(hn32.pow(2).mean(-1) + eps)

    assert y.dtype == ydt and hx.grad.dtype == hdt
    chk(y.detach(), r["y"], y32, "rmsnorm.y")
    if mode == "add":
        assert hn.dtype == hdt and torch.equal(hn.detach(), hn32.to(hdt))  # one correctly rounded add (+ RNE to bf16)
        assert ax.grad.dtype == adt
        chk(ax.grad, r["da"], dx32, "rmsnorm.da")
    chk(hx.grad, r["dx"], dx32, "rmsnorm.dx")
    chk(gw, gw0.double() + r["dw"], gw0 + dw32, "rmsnorm.dw")  # accumulated into gw, not overwritten
    from nanodiloco_amd.ops.norm import _hip_fwd
    y2, _, rstd = _hip_fwd(h, a, w, eps, ydt)
    assert torch.equal(y2, y.detach())
    chk(rstd, r["rstd"], rstd32, "rmsnorm.rstd")


@pytest.mark.parametrize("cols", NORM_COLS)
def test_rmsnorm_every_chunk_count_and_dtype(cols):
    """Every NCH of the dispatch (1, 2, 4 through nch = 3, 8 at both ends), the first lane of a new chunk, 1 / 3 /
    67 / 257 rows (67: a second backward block with three rows); dtype combinations paired across shapes."""
    i = NORM_COLS.index(cols)
    for j, (mode, hdt, adt, ydt) in enumerate(NORM_COMBOS):
        _norm_case(mode, hdt, adt, ydt, NORM_ROWS[(i + j) % 4], cols)
        _norm_case(mode, hdt, adt, ydt, NORM_ROWS[(i + j + 2) % 4], cols)


@pytest.mark.parametrize("rows,combo", [(32768 + 5, 8), (32768 + 5, 0), (65536 + 67, 5), (65536 + 67, 4)])
def test_rmsnorm_grid_wrap(rows, combo):
    """More rows than the capped grids visit in one trip: 8192 forward blocks x 4 waves, 1024 backward blocks x 64."""
    _norm_case(*NORM_COMBOS[combo], rows, 8)


@pytest.mark.parametrize("cols", [12, 4104])
def test_rmsnorm_refuses_bad_columns_and_writes_nothing(cols):
    rows = 3
    x = torch.randn(rows, cols, device=DEV)
    w = torch.ones(cols, device=DEV)
    with pytest.raises(RuntimeError):
        ops.rmsnorm(x, w, None, 1e-5, BF16)
    L = _ext.lib()
    ybig, y = framed_flat(rows * cols, BF16)
    rbig, rstd = framed_flat(rows, F32)
    snap = (_ints(ybig).clone(), _ints(rbig).clone())
    assert L.nd_rmsnorm_fwd(x.data_ptr(), 0, 0, 0, w.data_ptr(), y.data_ptr(), 1, 0, rstd.data_ptr(), rows, cols, 1e-5,
                            S()) != 0
    dxbig, dx = framed_flat(rows * cols, F32)
    pbig, part = framed_flat(cols, F32)
    snap2 = (_ints(dxbig).clone(), _ints(pbig).clone())
    dy = torch.randn(rows, cols, device=DEV)
    rs = torch.ones(rows, device=DEV)
    assert L.nd_rmsnorm_bwd(dy.data_ptr(), 0, x.data_ptr(), 0, w.data_ptr(), rs.data_ptr(), 0, dx.data_ptr(), 0, 0, rows,
                            cols, part.data_ptr(), S()) != 0
    torch.cuda.synchronize()
    assert torch.equal(_ints(ybig), snap[0]) and torch.equal(_ints(rbig), snap[1])
    assert torch.equal(_ints(dxbig), snap2[0]) and torch.equal(_ints(pbig), snap2[1])


def test_colsum_add_row_groups_and_column_edges():
    """nd_colsum_add at 1 / 15 / 16 / 17 / 127 / 128 / 129 partial rows (the 16 row groups and the 8-deep unroll)
    and 4 / 60 / 64 / 68 / 4096 columns (one quad, a partial and a second workgroup); += into a framed output."""
    L = _ext.lib()
    for rows in (1, 15, 16, 17, 127, 128, 129):
        for cols in (4, 60, 64, 68, 4096):
            part = o64.spiked(rows, cols, DEV)
            big, out = framed_flat(cols, F32)
            out.copy_(torch.randn(cols, device=DEV))
            out0 = out.clone()
            _ext.check(L.nd_colsum_add(part.data_ptr(), out.data_ptr(), rows, cols, S()), "colsum")
            chk(out, o64.colsum_add(part, out0), out0 + part.sum(0), "colsum_add")
            assert_frame_intact(big, out)


# ------------------------------------------------------------------------------------------ RoPE
def _rope_twin(x32, cos, sin, B, T, nh, nkv, hd, inverse=False):
    q, k, v = ref.split_qkv(x32, B, T, nh, nkv, hd)
    s = -sin if inverse else sin
    return torch.cat([ref.apply_rope(q, cos, s).transpose(1, 2).reshape(B * T, -1),
                      ref.apply_rope(k, cos, s).transpose(1, 2).reshape(B * T, -1),
                      v.transpose(1, 2).reshape(B * T, -1)], dim=1)


def _assert_rope_roundtrip(x, r, back, hd, nrot):
    """inverse(forward(x)) == x within two roundings: u * (|y1| + |y2|) from the stored forward pair, u * |x| from the
    store of the result (u: half an ulp of the dtype; 1 + 2u: the second rounding acts on the perturbed value), and
    the fp32 tables' cos^2 + sin^2 = 1 +- 2^-23 with the fp32 arithmetic of both passes: 2^-21 of the pair's norm."""
    rows = x.shape[0]
    u = 2.0 ** -8 if x.dtype == BF16 else 2.0 ** -24
    half = hd // 2
    y = r[:, :nrot].reshape(rows, -1, hd).abs()
    ysum = (y[..., :half] + y[..., half:]).repeat(1, 1, 2).reshape(rows, nrot)
    xx = x.double()[:, :nrot].reshape(rows, -1, hd)
    norm = (xx[..., :half] ** 2 + xx[..., half:] ** 2).sqrt().repeat(1, 1, 2).reshape(rows, nrot)
    bound = u * (1 + 2 * u) * (ysum + x.double()[:, :nrot].abs()) + 2.0 ** -21 * norm
    err = (back.double()[:, :nrot] - x.double()[:, :nrot]).abs()
    assert bool((err <= bound).all()), (err - bound).max().item()


def _rope_case(dt, hd, B, T, nh, nkv):
    from nanodiloco_amd.ops.attention import rope_cache
    rows, ld = B * T, (nh + 2 * nkv) * hd
    nrot = (nh + nkv) * hd
    cos, sin = rope_cache(T, hd, 10000.0, None, DEV)
    x = o64.spiked(rows, ld, DEV).to(dt)
    big, qkv = framed(rows, ld, dt)
    qkv.copy_(x)
    L = _ext.lib()

    def run(inverse):
        _ext.check(L.nd_rope_inplace(qkv.data_ptr(), _ext.dtcode(qkv), cos.data_ptr(), sin.data_ptr(), rows, T, nh, nkv,
                                     hd, qkv.stride(0), inverse, S()), "nd_rope_inplace")

    run(0)
    fwd = qkv.clone()
    r = o64.rope(x, cos, sin, B, T, nh, nkv, hd)
    chk(fwd, r, _rope_twin(x.float(), cos, sin, B, T, nh, nkv, hd), "rope.fwd")
    assert torch.equal(fwd[:, nrot:], x[:, nrot:])  # v untouched
    assert_frame_intact(big, qkv)
    run(1)
    back = qkv.clone()
    chk(back, o64.rope(fwd, cos, sin, B, T, nh, nkv, hd, inverse=True),
        _rope_twin(fwd.float(), cos, sin, B, T, nh, nkv, hd, inverse=True), "rope.inv")
    assert torch.equal(back[:, nrot:], x[:, nrot:])
    assert_frame_intact(big, qkv)
    _assert_rope_roundtrip(x, r, back, hd, nrot)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("hd", [8, 32, 64, 128])
def test_rope_head_dims_positions_and_gqa(hd, dt):
    """One 4-pair group per head (hd 8) up to 16; (B, T) where ``row % T`` wraps; GQA 4/4, 4/2, 4/1; in place on a
    strided view whose frame must survive; v bitwise untouched; forward and inverse per element."""
    for (B, T), (nh, nkv) in zip([(1, 1), (3, 5), (2, 96)], [(4, 4), (4, 2), (4, 1)]):
        _rope_case(dt, hd, B, T, nh, nkv)
    _rope_case(dt, hd, 3, 5, 4, 4)


def test_rope_grid_wrap():
    """7300 rows x 36 rotated heads x 16 groups: just over the 16384 x 256 work items of the capped grid."""
    assert 7300 * 36 * 16 > 16384 * 256
    _rope_case(BF16, 128, 4, 1825, 32, 4)


# ------------------------------------------------------------------------------------------ SwiGLU
def _swiglu_case(dt, n, F):
    gu = o64.spiked(n, 2 * F, DEV)
    gu[0, :5] = torch.tensor([100.0, -100.0, 20.0, -20.0, 0.0], device=DEV)
    gu[n - 1, F - 5:F] = torch.tensor([0.0, -20.0, 20.0, -100.0, 100.0], device=DEV)
    gu = gu.to(dt)
    dy = o64.spiked(n, F, DEV, 1.0, start=2).to(dt)
    x = gu.clone().requires_grad_(True)
    y = ops.swiglu(x)
    y.backward(dy)
    assert y.dtype == dt and x.grad.dtype == dt
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(x.grad).all())
    chk(y.detach(), o64.swiglu_fwd(gu), ref.swiglu(gu.float()), "swiglu.fwd")
    chk(x.grad, o64.swiglu_bwd(dy, gu), ref.swiglu_backward(dy.float(), gu.float()), "swiglu.bwd")


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("F", [8, 72, 2688])
def test_swiglu_small_shapes_and_saturated_gates(F, dt):
    """One 8-column item per row up to 336, 1 / 3 / 777 rows, gates at +-100, +-20 and 0 beside random ones."""
    for n in (1, 3, 777):
        _swiglu_case(dt, n, F)


def test_swiglu_grid_wrap():
    """4 194 304 + 5 one-item rows: five items past the 16384 x 256 of the capped grid."""
    _swiglu_case(BF16, 4 * 1024 * 1024 + 5, 8)


def test_swiglu_refuses_f12():
    gu = torch.randn(3, 24, device=DEV).bfloat16()
    with pytest.raises(RuntimeError):
        ops.swiglu(gu)


# ------------------------------------------------------------------------------------------ embedding
def _embedding_case(odt, n, d, V=300):
    W = torch.randn(V, d, device=DEV)
    base = torch.randn(V, d, device=DEV)
    ids = torch.randint(0, V, (n,), device=DEV)
    if n >= 5:
        ids[1], ids[2], ids[n - 1] = -1, V, V + 5
        ids[3] = ids[0]
    safe, ok = o64._masked_ids(ids, V)
    gW = base.clone()
    out = ops.embedding(ids, W, gW, out_dtype=odt)
    assert out.dtype == odt and torch.equal(out.detach(), o64.embedding_fwd(ids, W).float().to(odt))
    assert not bool(out.detach()[~ok].any())  # out-of-range ids: zero rows
    dy = o64.spiked(n, d, DEV).to(odt)
    out.backward(dy)
    r = o64.embedding_bwd(ids, dy, V, base)
    twin = base.clone().index_add_(0, safe, dy.float() * ok[:, None])
    chk(gW, r, twin, "embedding.bwd_atomic")
    _embedding_sorted(ids, dy, V, base, r, twin)


def _embedding_sorted(ids, dy, V, base, r, twin):
    from nanodiloco_amd.ops.embedding import sorted_bwd_workspace
    n, d = dy.shape
    gW = base.clone()
    perm = torch.argsort(ids, stable=True)
    sid = ids.index_select(0, perm).contiguous()
    ws = sorted_bwd_workspace(n, d, DEV).fill_(float("nan"))
    _ext.check(_ext.lib().nd_embedding_bwd_sorted(sid.data_ptr(), perm.data_ptr(), dy.data_ptr(), _ext.dtcode(dy),
                                                  gW.data_ptr(), ws.data_ptr(), n, d, V, S()), "sorted")
    chk(gW, r, twin, "embedding.bwd_sorted")


@pytest.mark.parametrize("odt", [F32, BF16])
@pytest.mark.parametrize("d", [4, 100, 256, 260, 1024])
def test_embedding_row_widths_and_bad_ids(d, odt):
    """One lane's float4 (d 4) to four column trips (1024), widths that end inside a trip (100, 260); ids -1, V and
    V + 5 give zero rows forward and nothing backward, atomic and sorted."""
    for n in (1, 5, 4099):
        _embedding_case(odt, n, d)


@pytest.mark.parametrize("odt", [F32, BF16])
def test_embedding_grid_wrap(odt):
    _embedding_case(odt, 32768 + 7, 4)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_embedding_sorted_long_runs_and_chunk_borders(dt):
    """Sorted backward: a run over more than three 64-row chunks (head / tail join), a run ending exactly on a chunk
    border, out-of-range ids at both ends of the sorted order."""
    V, d = 50, 100
    counts = [(-1, 3), (2, 61), (5, 64 * 3 + 40), (6, 24), (7, 64), (9, 1), (11, 63), (V, 2), (V + 5, 7)]
    ids = torch.cat([torch.full((c,), i, device=DEV, dtype=torch.long) for i, c in counts])
    assert (3 + 61 + 64 * 3 + 40 + 24) % 64 == 0 and (3 + 61) % 64 == 0
    ids = ids[torch.randperm(ids.numel(), device=DEV)]
    safe, ok = o64._masked_ids(ids, V)
    dy = o64.spiked(ids.numel(), d, DEV).to(dt)
    base = torch.randn(V, d, device=DEV)
    _embedding_sorted(ids, dy, V, base, o64.embedding_bwd(ids, dy, V, base),
                      base.clone().index_add_(0, safe, dy.float() * ok[:, None]))


def test_embedding_sorted_chunk_wrap():
    """More 64-row chunks than the capped grid's 32768 waves, d = 4."""
    V, d, n = 1000, 4, 64 * 32768 + 64 * 5 + 3
    ids = torch.randint(0, V, (n,), device=DEV)
    ids[:300] = 17
    dy = torch.randn(n, d, device=DEV)
    base = torch.randn(V, d, device=DEV)
    _embedding_sorted(ids, dy, V, base, o64.embedding_bwd(ids, dy, V, base), base.clone().index_add_(0, ids, dy))


# ------------------------------------------------------------------------------------------ cross-entropy alone
CE_V = [8, 100, 1000, 1001, 8192, 8200, 32000, 32768, 32776, 50257]
IGN = -100


def _ce_kernel_name(V, dt):
    if V % 8 or V > 32768:
        return "ce_generic"
    if V <= 8192:
        return "ce_reg4"
    return "ce_bf16" if dt == BF16 else "ce_reg16"


def _ce_inputs(V, dt):
    """18 rows: three logit patterns (4 randn; one +60 among -60; constant) x six targets (0, V - 1, a column of
    the last partial chunk, a middle column, ignore_index, the row's arg-max)."""
    n = 18
    x = 4 * torch.randn(n, V, device=DEV)
    peak = [V - 1, 0, max(0, V - 3), V // 2, V // 3, (V - 1) // 8 * 8]
    for k, r in enumerate(range(1, n, 3)):
        x[r] = -60.0
        x[r, peak[k]] = 60.0
    x[2::3] = 1.5
    x = x.to(dt)
    tgt = torch.empty(n, dtype=torch.long, device=DEV)
    kinds = [0, V - 1, max(0, V - 3), V // 2, IGN, None]
    for r in range(n):
        k = kinds[(r // 3 + r % 3) % 6]  # every pattern meets every kind of target
        tgt[r] = int(x[r].float().argmax()) if k is None else k
    return x, tgt


def _ce_twin(x32, tgt, scale):
    lse = torch.logsumexp(x32, dim=-1)
    ok = tgt != IGN
    safe = torch.where(ok, tgt, torch.zeros_like(tgt))
    loss = torch.where(ok, lse - x32.gather(1, safe[:, None])[:, 0], torch.zeros_like(lse))
    p = torch.softmax(x32, dim=-1)
    p.scatter_add_(1, safe[:, None], -torch.ones_like(p[:, :1]))
    return lse, loss, p * (ok[:, None].to(p.dtype) * scale)


def _ce_run(x, tgt, scale, with_rows, loss0=3.0):
    n, V = x.shape
    big, flat = framed_flat(n * V, x.dtype, pad=64)
    logits = flat.view(n, V)
    logits.copy_(x)
    lbig, lse = framed_flat(n, F32)
    rbig, rows = framed_flat(n, F32)
    loss_sum = torch.full((1,), loss0, device=DEV)
    _ext.check(_ext.lib().nd_ce_fwd_bwd(logits.data_ptr(), _ext.dtcode(x), tgt.data_ptr(), loss_sum.data_ptr(),
                                        scale.data_ptr(), n, V, IGN, lse.data_ptr(), rows.data_ptr() if with_rows else 0,
                                        0.0, S()), "nd_ce_fwd_bwd")
    assert_frame_intact(big, flat)
    assert_frame_intact(lbig, lse)
    assert_frame_intact(rbig, rows if with_rows else None)
    return logits, lse, rows, loss_sum


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("V", CE_V)
def test_ce_kernel_alone(V, dt):
    """nd_ce_fwd_bwd on given logits, both sides of the dispatch borders at 8192 and 32768 and V % 8 != 0: every
    dlogits element, lse_out, row_loss (ignored rows exactly 0) and the atomic loss_sum against float64; bf16 rows
    that take the packed kernel run once more under ND_CE=r, under the name ce_reg16."""
    k = _ce_kernel_name(V, dt)
    _ce_alone(V, dt, k)
    if k == "ce_bf16":  # ND_CE=r: bf16 rows of 8192 < V <= 32768 take the register kernel instead of the packed one
        with switches(ND_CE="r") as state:
            assert state["ND_CE"] == "r"
            _ce_alone(V, dt, "ce_reg16")


def _ce_alone(V, dt, k):
    x, tgt = _ce_inputs(V, dt)
    scale = torch.tensor([0.25 / 15], device=DEV)
    lse64, loss64, dl64 = o64.ce_rows(x, tgt, scale.item())
    lse32, loss32, dl32 = _ce_twin(x.float(), tgt, scale)
    dl, lse, rows, loss_sum = _ce_run(x, tgt, scale, True)
    chk(dl, dl64, dl32, k + ".dlogits")
    chk(lse, lse64, lse32, k + ".lse")
    chk(rows, loss64, loss32, k + ".row_loss")
    assert not bool(rows[tgt == IGN].any()) and not bool(dl[tgt == IGN].any())
    assert loss_sum.item() == 3.0  # row_loss given: the atomic sum is not touched
    dl2, lse2, _, _ = _ce_run(x, tgt, scale, False)
    assert torch.equal(dl2, dl) and torch.equal(lse2, lse)
    # the atomic sum, one launch per group of three rows: a six-element tensor for the rule
    sums = torch.cat([_ce_run(x[g:g + 3], tgt[g:g + 3], scale, False, 0.0)[3] for g in range(0, 18, 3)])
    chk(sums, loss64.reshape(6, 3).sum(1), loss32.reshape(6, 3).sum(1), k + ".loss_sum")
    # an all-ignored batch: zero loss, all-zero dlogits
    none = torch.full_like(tgt, IGN)
    dl, _, rows, _ = _ce_run(x, none, scale, True)
    assert not bool(dl.any()) and not bool(rows.any())
    dl, _, _, loss_sum = _ce_run(x, none, scale, False)
    assert not bool(dl.any()) and loss_sum.item() == 3.0


def test_lm_head_ce_all_targets_ignored():
    n, d, V = 64, 256, 1000
    y0 = (0.5 * torch.randn(n, d, device=DEV)).bfloat16()
    W = (0.05 * torch.randn(V, d, device=DEV)).bfloat16()
    tgt = torch.full((n,), IGN, device=DEV, dtype=torch.long)
    res = []
    for twin in (False, True):
        ops.set_backend("torch" if twin else "hip")
        y = y0.clone().requires_grad_(True)
        gW = torch.zeros(V, d, device=DEV)
        loss = ops.lm_head_ce(y, W, gW, tgt, loss_scale=0.25, chunk_rows=256)
        loss.backward()
        res.append((loss.detach(), y.grad, gW))
    ops.set_backend("hip")
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a.float(), b.float()) and not bool(a.any())


# ------------------------------------------------------------------------------------------ optimizer kernels
OPT_N = [1, 3, 4, 5, 1027, 2 * 1024 * 1024 + 4099 + 3]


def _grad(n, scale=3.0):
    """randn * scale with 8 * scale spikes at both ends and on either side of the last float4 boundary."""
    g = scale * torch.randn(n, device=DEV) + 1.0
    for k, i in enumerate((0, n - 1, (n // 4) * 4 - 1, min(n - 1, (n // 4) * 4))):
        if n >= 8:
            g[i] = 8.0 * scale * (1 - 2 * (k % 2))
    return g


REPLICAS = 32  # independent launches of a tiny size, judged as one tensor: the rule's slack is a maximum over the
#                compared tensor, and on a handful of elements the twin's error is whatever one draw gives (even 0)


def _replicas(n):
    return REPLICAS if n < 64 else 1


def _chk_steps(runs, names):
    """runs: per replica, per step, {name: (out, ref64, twin32)}; each step's replicas are compared as one tensor."""
    for step in range(len(runs[0])):
        for name in names:
            out, r64, t32 = (torch.cat([run[step][name][k].reshape(-1) for run in runs]) for k in range(3))
            chk(out, r64, t32, name, f"step {step + 1}")


def _adamw_steps(n, shadow, max_norm, wd):
    bufs = [framed_flat(n, F32) for _ in range(3)]
    (pb, p), (mb, m), (vb, v) = bufs
    p.copy_(torch.randn(n, device=DEV))
    m.zero_()
    v.zero_()
    sb, sh = framed_flat(n, BF16)
    sh.zero_()
    p32, m32, v32 = p.clone(), m.clone(), v.clone()
    p64, m64, v64 = p.double(), m.double(), v.double()
    norm, norm32 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    steps = []
    for step in (1, 2, 3):
        g = _grad(n)
        ops.adamw_step(p, g.clone(), m, v, sh if shadow else None, step, 1e-3, (0.9, 0.999), 1e-8, wd, max_norm,
                       norm_out=norm)
        with torch_twin():
            ops.adamw_step(p32, g.clone(), m32, v32, None, step, 1e-3, (0.9, 0.999), 1e-8, wd, max_norm, norm_out=norm32)
        p64, m64, v64, n64 = o64.adamw(p64, g, m64, v64, step, 1e-3, (0.9, 0.999), 1e-8, wd, max_norm)
        if max_norm == 0.5 and n >= 1027:
            assert n64.item() > 0.5  # the clip binds
        steps.append({"adamw.master": (p.clone(), p64, p32.clone()), "adamw.m": (m.clone(), m64, m32.clone()),
                      "adamw.v": (v.clone(), v64, v32.clone()), "adamw.norm_out": (norm.clone(), n64, norm32.clone()),
                      "global_grad_norm": (ops.global_grad_norm(g), n64, norm32.clone())})
        if shadow:
            assert torch.equal(sh, p.bfloat16())
    for big, view in bufs + [(sb, sh)]:
        assert_frame_intact(big, view)
    if not shadow:
        assert not bool(sh.any())
    return steps


@pytest.mark.parametrize("shadow,max_norm,wd", [(True, None, 0.0), (False, 0.5, 0.01), (True, 1e9, 0.01)])
@pytest.mark.parametrize("n", OPT_N)
def test_adamw_tails_wrap_and_clip(n, shadow, max_norm, wd):
    """n % 4 tails of the sum-of-squares and AdamW streams, one element, a wrap of the 2048-block grid; no clip, a
    clip that binds, one that does not; three steps, master / m / v per element, norm_out, the bf16 shadow."""
    runs = [_adamw_steps(n, shadow, max_norm, wd) for _ in range(_replicas(n))]
    _chk_steps(runs, ["adamw.master", "adamw.m", "adamw.v"])
    # the norms of all steps and replicas as one tensor
    for name in ("adamw.norm_out", "global_grad_norm"):
        out, r64, t32 = (torch.cat([st[name][k].reshape(-1) for run in runs for st in run]) for k in range(3))
        chk(out, r64, t32, name)


@pytest.mark.parametrize("comm", [F32, BF16])
@pytest.mark.parametrize("n", OPT_N)
def test_pseudograd_bitwise(n, comm):
    sync = torch.randn(n, device=DEV)
    local = sync - 0.01 * _grad(n)
    big, delta = framed_flat(n, comm)
    ops.pseudograd(sync, local, delta)
    assert torch.equal(delta, (sync - local).to(comm))  # one correctly rounded subtraction (+ RNE to bf16)
    assert torch.equal(delta, o64.pseudograd(sync, local).float().to(comm))
    assert_frame_intact(big, delta)


def _outer_steps(n, comm, shadow, drift):
    sync0 = torch.randn(n, device=DEV)
    bufs = [framed_flat(n, F32) for _ in range(3)]
    (pb, p), (sb_, sync), (mb, mom) = bufs
    p.copy_(sync0 - 0.01 * torch.randn(n, device=DEV))
    sync.copy_(sync0)
    mom.fill_(7.0)  # a first step must not read it
    shb, sh = framed_flat(n, BF16)
    sh.zero_()
    p32, s32, m32 = p.clone(), sync.clone(), mom.clone()
    p64, s64, m64 = p.double(), sync.double(), mom.double()
    steps = []
    for first in (True, False):
        dsum = (4 * (s32 - p32) + 0.003 * torch.randn(n, device=DEV)).to(comm)
        base = 0.01 * torch.randn(n, device=DEV) if drift else None
        ops.outer_nesterov(p, sync, dsum, mom, sh if shadow else None, 0.25, 0.7, 0.9, first, drift_base=base)
        with torch_twin():
            ops.outer_nesterov(p32, s32, dsum, m32, None, 0.25, 0.7, 0.9, first, drift_base=base)
        p64, s64, m64 = o64.outer_nesterov(p64, s64, dsum, m64, 0.25, 0.7, 0.9, first, base)
        steps.append({"outer.master": (p.clone(), p64, p32.clone()), "outer.sync": (sync.clone(), s64, s32.clone()),
                      "outer.mom": (mom.clone(), m64, m32.clone())})
        if first:  # mom = delta_sum / 4: exact
            assert torch.equal(mom, dsum.float() * 0.25) and torch.equal(mom.double(), m64)
        if shadow:
            assert torch.equal(sh, p.bfloat16())
        if not drift:
            assert torch.equal(sync, p)
    for big, view in bufs + [(shb, sh)]:
        assert_frame_intact(big, view)
    if not shadow:
        assert not bool(sh.any())
    return steps


@pytest.mark.parametrize("comm,shadow,drift", [(F32, True, False), (BF16, False, True), (F32, False, True),
                                               (BF16, True, False)])
@pytest.mark.parametrize("n", [1, 5, 4099, 1024 * 1024 + 259])
def test_outer_nesterov_two_steps(n, comm, shadow, drift):
    """First step, then a non-first one on the same state; inv_world 1/4; fp32 / bf16 delta_sum; shadow or none;
    drift_base or none; a wrap of the 4096-block grid.  master, sync, mom per element; the shadow bitwise."""
    runs = [_outer_steps(n, comm, shadow, drift) for _ in range(_replicas(n))]
    _chk_steps(runs, ["outer.master", "outer.sync", "outer.mom"])


# ------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 64), (65, 63), (1000, 264)])
def test_transpose_small_and_partial_tiles(rows, cols):
    """One element, one row, edge tiles on the scalar kernel (odd strides), partial tiles on the vector kernel."""
    w = torch.randn(rows, cols, device=DEV).bfloat16()
    out = torch.empty(cols, rows, device=DEV, dtype=BF16)
    ops.transpose_into(out, w)
    assert torch.equal(out, w.t())
    assert torch.equal(out.double(), o64.transpose(w))


@pytest.mark.parametrize("rows,cols,pad", [(1000, 264, 16), (65, 63, 5), (1, 64, 8)])
def test_transpose_strided_views_keep_their_padding(rows, cols, pad):
    """Source and destination are column slices of wider tensors (lds > cols, ldd > rows): 1000 x 264 with pad 16 keeps
    the vector kernel (16-B aligned bases, strides % 8 == 0), the others take the scalar one; the destination's
    padding columns survive."""
    wide = torch.randn(rows, cols + 2 * pad, device=DEV).bfloat16()
    src = wide[:, pad:pad + cols]
    big, dst = framed(cols, rows, BF16, pad_r=1, pad_c=pad)
    assert src.stride(0) > cols and dst.stride(0) > rows
    ops.transpose_into(dst, src)
    assert torch.equal(dst, src.t())
    assert_frame_intact(big, dst)
