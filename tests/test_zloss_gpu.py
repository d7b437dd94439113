"""z-loss on the HIP path: the Z instantiations of ``csrc/cross_entropy.hip`` (``nd_ce_z_fwd_bwd``,
``nd_ce_z_fwd_bwd_q8``) per element against the float64 oracle of ``tests/_zloss.py`` (checked on the CPU by
``tests/test_zloss_cpu.py``), ``ops.lm_head_ce(..., z_loss=)``, the model with ``z_loss`` set -- eager, captured and
with the fp8 lm head.

Error rule: ``_oracle64.check`` (bf16 outputs: half an ulp relative plus slack; fp32 outputs: slack; slack = margin
x the error of the fp32 PyTorch twin of the same formulae on the same inputs), margin 8 except ``MARGINS``.  Every
case prints the margin it needed; docs/PARITY.md ("z-loss") has the table.

``MARGINS``: the packed bf16 kernel keeps its logsumexp in the log2 domain, ``lse2 = m * log2(e) + log2(s)`` and
``lse = lse2 * ln 2``: half an ulp of 86.6 (3.8e-6, times ln 2) from the first product and half an ulp of 60
(1.9e-6) from the second at the saturated rows, m = 60, where the twin's lse is exactly 60 -- the effect
docs/PARITY.md (T3) derives for ``ce_bf16.lse``.  In ``lse^2`` it is multiplied by 2 lse = 120: up to 5.4e-4, plus
half an ulp of 3600 (1.2e-4), against a twin error of 3.4e-5 over the tensor (a ratio of 20; first measured 14.3).
Margin 32 for the packed kernel's ``row_z`` and the sums of it.  Every other output keeps the margin of 8 -- the
dlogits too, whose z-free siblings need 32 and 256: on the target column of a saturated row, where the kernels'
exp error shows, ``p g - 1`` no longer cancels to 0 and the twin's own rounding is of the same size.
"""
import os

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import _ext
from nanodiloco_amd.ops import fp8

from . import _oracle64 as o64
from . import _zloss as zl
from ._frames import assert_frame_intact, framed_flat
from ._switches import switches

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
IGN = zl.IGN
INVALID = 1  # hipErrorInvalidValue
ZC = o64.f32_scalar(1e-2)  # the C float the kernels receive
CE_V = [8, 100, 1001, 8192, 8200, 32768, 32776]
N_ROWS = 24

MARGINS = {"z.ce_bf16.row_z": 32.0, "z.ce_bf16.z_sum": 32.0}
REPORT = {}


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    torch.manual_seed(0)
    yield
    ops.set_backend("auto")
    ops.set_deterministic(False)


@pytest.fixture(scope="module", autouse=True)
def _slack_report():
    yield
    for k in sorted(REPORT):
        print(f"\n[slack] {k}: needs margin {REPORT[k]:.3g} (allowed {MARGINS.get(k, o64.MARGIN)})", end="")
    print()


def chk(out, ref64, twin32, name, rel=None, note=""):
    ratio = o64.excess_ratio(out, ref64, twin32, rel)
    print(f"[z-loss] {name}{' ' + note if note else ''}: needs margin {ratio:.3g}")
    o64.check(out, ref64, twin32, margin=MARGINS.get(name, o64.MARGIN), name=name, rel=rel, report=REPORT, note=note)


def S():
    return _ext.stream_ptr(torch.device(DEV))


def sc(v):
    return torch.tensor([v], dtype=F32, device=DEV)


def _bits(t):
    return t.detach().contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


# ------------------------------------------------------------------------------------------ the kernels alone
def _kernel_name(V, dt):
    if V % 8 or V > 32768:
        return "ce_generic"
    if V <= 8192:
        return "ce_reg4"
    return "ce_bf16" if dt == BF16 else "ce_reg16"


def _inputs(V, dt):
    """24 rows: four logit patterns (4 randn; one +60 among -60; constant 1.5; -20 + randn, whose lse is negative:
    g < 1) x six targets (0, V - 1, a column of the last partial 8-chunk, a middle column, ignore_index, the row's
    arg-max); every pattern meets every kind of target."""
    n = N_ROWS
    x = 4 * torch.randn(n, V, device=DEV)
    peak = [V - 1, 0, max(0, V - 3), V // 2, V // 3, (V - 1) // 8 * 8]
    for k, r in enumerate(range(1, n, 4)):
        x[r] = -60.0
        x[r, peak[k]] = 60.0
    x[2::4] = 1.5
    x[3::4] = -20.0 + torch.randn(n // 4, V, device=DEV)
    x = x.to(dt)
    tgt = torch.empty(n, dtype=torch.long, device=DEV)
    kinds = [0, V - 1, max(0, V - 3), V // 2, IGN, None]
    for r in range(n):
        k = kinds[(r // 4 + r % 4) % 6]
        tgt[r] = int(x[r].float().argmax()) if k is None else k
    return x, tgt


def _run(x, tgt, scale, with_rows, ce0=3.0, z0=5.0):
    """nd_ce_z_fwd_bwd on framed buffers: (dlogits, lse, row CE, row lse^2, CE sum, lse^2 sum)."""
    n, V = x.shape
    big, flat = framed_flat(n * V, x.dtype, pad=64)
    logits = flat.view(n, V)
    logits.copy_(x)
    lbig, lse = framed_flat(n, F32)
    rbig, rows = framed_flat(n, F32)
    zbig, rows_z = framed_flat(n, F32)
    ce_sum, z_sum = torch.full((1,), ce0, device=DEV), torch.full((1,), z0, device=DEV)
    _ext.check(_ext.lib().nd_ce_z_fwd_bwd(logits.data_ptr(), _ext.dtcode(x), tgt.data_ptr(), ce_sum.data_ptr(),
                                          z_sum.data_ptr(), scale.data_ptr(), n, V, IGN, lse.data_ptr(),
                                          rows.data_ptr() if with_rows else 0, rows_z.data_ptr() if with_rows else 0,
                                          ZC, S()), "nd_ce_z_fwd_bwd")
    assert_frame_intact(big, flat)
    assert_frame_intact(lbig, lse)
    assert_frame_intact(rbig, rows if with_rows else None)
    assert_frame_intact(zbig, rows_z if with_rows else None)
    return logits, lse, rows, rows_z, ce_sum, z_sum


def _plain(x, tgt, scale, with_rows, ce0=3.0):
    """The z-free entry on the same inputs: (dlogits, row CE, CE sum)."""
    d = x.clone()
    rows = torch.zeros(x.shape[0], device=DEV)
    ce_sum = torch.full((1,), ce0, device=DEV)
    _ext.check(_ext.lib().nd_ce_fwd_bwd(d.data_ptr(), _ext.dtcode(d), tgt.data_ptr(), ce_sum.data_ptr(),
                                        scale.data_ptr(), x.shape[0], x.shape[1], IGN, 0,
                                        rows.data_ptr() if with_rows else 0, 0.0, S()), "nd_ce_fwd_bwd")
    return d, rows, ce_sum


def _alone(V, dt, k):
    x, tgt = _inputs(V, dt)
    n_valid = int((tgt != IGN).sum())
    scale = sc(0.25 / n_valid)
    lse64, ce64, z64, dl64 = zl.ce_z_rows(x, tgt, scale.item(), ZC)
    lse32, ce32, z32, dl32 = zl.ce_z_rows_twin(x.float(), tgt, scale, ZC)
    g = 1.0 + 2.0 * ZC * lse64
    assert float(g.min()) < 0.9 and float(g.max()) > 2.0  # a missing or misplaced factor is far outside the rule
    dl, lse, rows, rows_z, ce_sum, z_sum = _run(x, tgt, scale, True)
    chk(dl, dl64, dl32, f"z.{k}.dlogits", note=f"V={V}")
    chk(lse, lse64, lse32, f"z.{k}.lse")
    chk(rows, ce64, ce32, f"z.{k}.row_ce")
    chk(rows_z, z64, z32, f"z.{k}.row_z")
    ign = tgt == IGN
    assert not bool(dl[ign].any()) and not bool(rows[ign].any()) and not bool(rows_z[ign].any())
    assert ce_sum.item() == 3.0 and z_sum.item() == 5.0  # per-row outputs given: no atomic, the sums are not touched
    dl2, lse2, _, _, _, _ = _run(x, tgt, scale, False)
    assert torch.equal(dl2, dl) and torch.equal(lse2, lse)
    # the atomic sums, one launch per group of four rows: six-element tensors for the rule
    sums = [_run(x[a:a + 4], tgt[a:a + 4], scale, False, 0.0, 0.0)[4:] for a in range(0, N_ROWS, 4)]
    chk(torch.cat([s[0] for s in sums]), ce64.reshape(6, 4).sum(1), ce32.reshape(6, 4).sum(1), f"z.{k}.ce_sum")
    chk(torch.cat([s[1] for s in sums]), z64.reshape(6, 4).sum(1), z32.reshape(6, 4).sum(1), f"z.{k}.z_sum")
    # CE is untouched by z: per row, and the atomic sum (two rows per launch from 0: a + b is the same either way)
    pd, prow, _ = _plain(x, tgt, scale, True)
    assert torch.equal(_bits(prow), _bits(rows)), "per-row CE differs from nd_ce_fwd_bwd's"
    assert not torch.equal(pd, dl)
    for a in range(0, N_ROWS, 2):
        zce = _run(x[a:a + 2], tgt[a:a + 2], scale, False, 0.0, 0.0)[4]
        assert torch.equal(_bits(zce), _bits(_plain(x[a:a + 2], tgt[a:a + 2], scale, False, 0.0)[2])), a
    # an all-ignored batch: all-zero outputs, accumulators untouched
    none = torch.full_like(tgt, IGN)
    dl, _, rows, rows_z, _, _ = _run(x, none, scale, True)
    assert not bool(dl.any()) and not bool(rows.any()) and not bool(rows_z.any())
    dl, _, _, _, ce_sum, z_sum = _run(x, none, scale, False)
    assert not bool(dl.any()) and ce_sum.item() == 3.0 and z_sum.item() == 5.0


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", CE_V)
def test_ce_z_kernel_alone(V, dt):
    """nd_ce_z_fwd_bwd on given logits, both sides of the dispatch borders at 8192 and 32768 and V % 8 != 0: every
    dlogits element, lse, the per-row CE and lse^2 and both atomic sums against float64; the CE outputs bitwise those
    of nd_ce_fwd_bwd; bf16 rows that take the packed kernel run once more under ND_CE=r."""
    k = _kernel_name(V, dt)
    _alone(V, dt, k)
    if k == "ce_bf16":
        with switches(ND_CE="r") as state:
            assert state["ND_CE"] == "r"
            _alone(V, dt, "ce_reg16")


def test_ce_z_refuses_bad_arguments():
    x, tgt = _inputs(100, F32)
    d = x.clone()
    ce, z = sc(3.0), sc(5.0)
    L = _ext.lib()
    for coef, zp in ((-1.0, z.data_ptr()), (float("nan"), z.data_ptr()), (float("inf"), z.data_ptr()), (ZC, 0)):
        rc = L.nd_ce_z_fwd_bwd(d.data_ptr(), _ext.dtcode(d), tgt.data_ptr(), ce.data_ptr(), zp, sc(1.0).data_ptr(),
                               N_ROWS, 100, IGN, 0, 0, 0, coef, S())
        assert rc == INVALID
    torch.cuda.synchronize()
    assert torch.equal(d, x) and ce.item() == 3.0 and z.item() == 5.0


# ------------------------------------------------------------------------------------------ fp8 dlogits
PRIOR = 2.0 ** -24


def _target(fmt, scale):
    r = fp8.Fp8Recipe(DEV, capacity=4)
    k = r.new_slot(fmt)
    r.scale[k] = scale
    r.ready[k] = True
    r.amax.fill_(PRIOR)
    return r, k, r.target(k, fmt)


def _q8(x, tgt, scale, fmt, qscale=2000.0):
    """nd_ce_z_fwd_bwd_q8 on framed logits and a framed fp8 output: (q, its frame, recipe, slot, CE sum, z sum, rc)."""
    n, V = x.shape
    lbig, lflat = framed_flat(n * V, x.dtype, pad=64)
    logits = lflat.view(n, V)
    logits.copy_(x)
    r, k, t = _target(fmt, qscale)
    big, qflat = framed_flat(n * V, fp8.TORCH_DT[fmt], pad=64)
    ce, z = sc(3.0), sc(5.0)
    rc = _ext.lib().nd_ce_z_fwd_bwd_q8(logits.data_ptr(), _ext.dtcode(logits), tgt.data_ptr(), ce.data_ptr(),
                                       z.data_ptr(), scale.data_ptr(), n, V, IGN, 0, 0, 0, ZC, *t.args(qflat), S())
    torch.cuda.synchronize()
    assert_frame_intact(lbig, lflat)
    assert torch.equal(_bits(logits), _bits(x)), "the logits were modified"
    assert_frame_intact(big, qflat if rc == 0 else None)
    return qflat.view(n, V), r, k, ce, z, rc


@pytest.mark.parametrize("V", [8200, 32768])
@pytest.mark.parametrize("fmt", [fp8.E4M3, fp8.E5M2], ids=["e4m3", "e5m2"])
def test_ce_z_q8_is_the_cast_of_the_bf16_dlogits(fmt, V):
    """V at the two ends of what the q8 entry accepts: its bytes and amax are bitwise nd_fp8_cast over the bf16
    dlogits of nd_ce_z_fwd_bwd (the invariant of the z-free pair), partial slot by partial slot (row b -> b % parts);
    the logits buffer is left as given; the sums are those of the bf16 entry."""
    x, tgt = _inputs(V, BF16)
    scale = sc(1.0 / 16)
    d, _, _, _, ce_ref, z_ref = _run(x, tgt, scale, False)
    q, r, k, ce, z, rc = _q8(x, tgt, scale, fmt)
    assert rc == 0
    ref_amax = torch.full((fp8.AMAX_PARTS,), PRIOR, device=DEV)
    ref8 = fp8.cast(d, r.scale[k:k + 1], fmt, ref_amax)
    assert torch.equal(q.view(torch.uint8), ref8.view(torch.uint8))
    assert r.amax[k].max().item() == ref_amax.max().item() == max(PRIOR, d.float().abs().max().item())
    row_max = d.float().abs().amax(dim=1)
    want = torch.full((fp8.AMAX_PARTS,), PRIOR, device=DEV)
    for b in range(N_ROWS):
        want[b % fp8.AMAX_PARTS] = torch.maximum(want[b % fp8.AMAX_PARTS], row_max[b])
    assert torch.equal(_bits(r.amax[k]), _bits(want))
    assert bool((r.amax[k + 1:] == PRIOR).all())
    assert bool((q.view(torch.uint8)[tgt == IGN] == 0).all())
    for got, ref in ((ce, ce_ref), (z, z_ref)):  # float atomics over 20 rows: equal up to their order
        assert abs(got.item() - ref.item()) <= 1e-5 * abs(ref.item())


@pytest.mark.parametrize("case", ["V=8192", "V=32776", "fp32", "ND_CE=r"])
def test_ce_z_q8_refuses_outside_its_range(case):
    V = {"V=8192": 8192, "V=32776": 32776}.get(case, 8200)
    x, tgt = _inputs(V, F32 if case == "fp32" else BF16)
    if case == "ND_CE=r":
        with switches(ND_CE="r"):
            q, r, k, ce, z, rc = _q8(x, tgt, sc(1.0 / 16), fp8.E5M2)
    else:
        q, r, k, ce, z, rc = _q8(x, tgt, sc(1.0 / 16), fp8.E5M2)
    assert rc == INVALID  # _q8 has checked that neither the logits nor any byte of the output frame changed
    assert ce.item() == 3.0 and z.item() == 5.0 and bool((r.amax == PRIOR).all())


# ------------------------------------------------------------------------------------------ lm_head_ce
def _lm_head(y0, W, tgt, backend, **kw):
    ops.set_backend(backend)
    try:
        y = y0.clone().requires_grad_(True)
        gW = torch.zeros(W.shape[0], W.shape[1], device=DEV)
        parts = ops.lm_head_ce_parts(y, W, gW, tgt, loss_scale=0.25, chunk_rows=256, **kw)
        parts.loss.backward()
        torch.cuda.synchronize()
        return parts, y.grad, gW
    finally:
        ops.set_backend("hip")


@pytest.mark.parametrize("V", [1000, 8200])
def test_lm_head_ce_z(V):
    """The whole op, two chunks (one ragged), bf16: loss parts, y.grad and gW against the float64 oracle of the op on
    the stored operands; the twin is the same op under set_backend("torch").

    The loss parts carry one more term than the rule's slack: the HIP path stores the logits in bf16 (the compute
    dtype) where the twin keeps them in fp32, so each logit is off by up to 2^-9 |x|, lse and x_t by up to
    2^-9 max|x| each (CE row: 2^-8 max|x|) and lse^2 by 2 |lse| 2^-9 max|x|.  That worst case, relative to the
    oracle's value, is the ``rel`` of the two checks."""
    n, d = 320, 256
    y0 = (0.5 * torch.randn(n, d, device=DEV)).bfloat16()
    W = (0.05 * torch.randn(V, d, device=DEV)).bfloat16()
    tgt = torch.randint(0, V, (n,), device=DEV)
    tgt[::10] = IGN
    ce64, z64, dy64, gw64 = zl.lm_head_ce_z(y0, W, tgt, 0.25, ZC)
    x64 = y0.double() @ W.double().t()
    xmax, lsemax = float(x64.abs().max()), float(torch.logsumexp(x64, dim=-1).abs().max())
    twin, dy32, gw32 = _lm_head(y0, W, tgt, "torch", z_loss=ZC)
    got, dy, gw = _lm_head(y0, W, tgt, "hip", z_loss=ZC)
    chk(got.ce_loss.reshape(1), ce64.reshape(1), twin.ce_loss.reshape(1), "z.lm_head.ce",
        rel=2.0 ** -8 * xmax / float(ce64))
    chk(got.z_loss.reshape(1), z64.reshape(1), twin.z_loss.reshape(1), "z.lm_head.z",
        rel=ZC * 2.0 * lsemax * 2.0 ** -9 * xmax / float(z64))
    assert float(z64) > 0.05 * float(ce64) > 0  # the z term is no rounding matter at these sizes
    assert torch.equal(got.loss.detach(), got.ce_loss + got.z_loss)
    chk(dy, dy64, dy32, "z.lm_head.dy", note=f"V={V}")
    chk(gw, gw64, gw32, "z.lm_head.gW", note=f"V={V}")
    # z_loss = 0.0 is the call that omits the argument, bit for bit; deterministic mode so that the loss is too
    ops.set_deterministic(True)
    a, dya, gwa = _lm_head(y0, W, tgt, "hip")
    b, dyb, gwb = _lm_head(y0, W, tgt, "hip", z_loss=0.0)
    assert torch.equal(a.loss, b.loss) and torch.equal(dya, dyb) and torch.equal(gwa, gwb) and b.z_loss is None
    # and the deterministic z path (per-row outputs, no float atomic) repeats bitwise and agrees with the atomic one
    c1, dyc1, gwc1 = _lm_head(y0, W, tgt, "hip", z_loss=ZC)
    c2, dyc2, gwc2 = _lm_head(y0, W, tgt, "hip", z_loss=ZC)
    assert torch.equal(c1.ce_loss, c2.ce_loss) and torch.equal(c1.z_loss, c2.z_loss) and torch.equal(c1.loss, c2.loss)
    assert torch.equal(dyc1, dy) and torch.equal(gwc1, gw) and torch.equal(dyc2, dy)
    assert torch.equal(c1.ce_loss, a.ce_loss)  # the same per-row CE, summed in the same order
    assert abs(float(c1.z_loss) - float(got.z_loss)) <= 1e-5 * float(got.z_loss)


# ------------------------------------------------------------------------------------------ model and graph
def _tiny():
    return LlamaConfig.from_json(os.path.join(ROOT, "configs", "llama_tiny.json"))


def _ids(seed, vocab):
    return torch.randint(0, vocab, (4, 64), device=DEV, generator=torch.Generator(DEV).manual_seed(seed))


def _eager(m, ids):
    m.store.zero_grad()
    out = m(ids, labels=ids, loss_scale=0.5)
    out.loss.backward()
    torch.cuda.synchronize()
    return (out.loss.detach().clone(), out.ce_loss.clone(), None if out.z_loss is None else out.z_loss.clone(),
            m.store.grad.clone())


def test_model_z_loss_eager_and_graph_bitwise():
    """The tiny model, 4 x 64 tokens, deterministic mode, z_loss = 1e-2: two eager passes agree bitwise in loss,
    ce_loss, z_loss and the flat grad buffer; GraphedMicroStep (two warm-ups, capture, two replays) returns the same
    bits through its static buffers; against z_loss = 0 the gradient differs and ce_loss does not."""
    from nanodiloco_amd.utils.graphs import GraphedMicroStep
    ops.set_deterministic(True)
    cfg = _tiny()
    ids = _ids(1, cfg.vocab_size)
    m = LlamaForCausalLM(cfg, DEV, BF16).init_weights(3)
    l0, ce0, z0, g0 = _eager(m, ids)
    assert z0 is None and torch.equal(l0, ce0)
    m.z_loss = 1e-2
    l1, ce1, z1, g1 = _eager(m, ids)
    l2, ce2, z2, g2 = _eager(m, ids)
    assert torch.equal(l1, l2) and torch.equal(ce1, ce2) and torch.equal(z1, z2) and torch.equal(g1, g2)
    assert torch.equal(ce1, ce0) and not torch.equal(g1, g0)
    assert torch.equal(l1, ce1 + z1) and 0.5 < float(z1) < 2.0  # 1e-2 * (ln 32000)^2 = 1.08 at initialisation
    assert bool(torch.isfinite(g1).all())
    g = GraphedMicroStep(m)
    for call in range(5):  # 2 eager warm-ups, capture + replay, 2 more replays
        m.store.zero_grad()
        loss = g(ids, ids, 0.5)
        torch.cuda.synchronize()
        assert torch.equal(loss, l1) and torch.equal(g.ce_loss, ce1) and torch.equal(g.z_loss, z1), call
        assert torch.equal(m.store.grad, g1), call
    assert g.graph is not None
    # another batch through the same graph: the static buffers follow
    ids2 = _ids(2, cfg.vocab_size)
    m.store.zero_grad()
    loss = g(ids2, ids2, 0.5).clone()
    ce_g, z_g, grad_g = g.ce_loss.clone(), g.z_loss.clone(), m.store.grad.clone()
    l3, ce3, z3, g3 = _eager(m, ids2)
    assert torch.equal(loss, l3) and torch.equal(ce_g, ce3) and torch.equal(z_g, z3) and torch.equal(grad_g, g3)
    assert not torch.equal(ce3, ce1)
    m.z_loss = 0.0
    with pytest.raises(ValueError, match="z_loss changed"):
        g(ids, ids, 0.5)


def test_fp8_model_z_loss_runs_the_q8_entry():
    """The tiny model with the fp8 projections and z_loss = 1e-2: the first step (no scale yet) takes the bf16 z
    entry plus the cast, later steps the z q8 entry; the z-free entries never run; every gradient is finite."""
    from ._model_oracle import spying
    cfg = _tiny()
    ids = _ids(1, cfg.vocab_size)
    m = LlamaForCausalLM(cfg, DEV, BF16, fp8=True, fp8_wgrad=True).init_weights(3)
    m.z_loss = 1e-2
    ran = []
    with spying() as spy:
        for step in range(3):
            before = (spy.ran("nd_ce_z_fwd_bwd"), spy.ran("nd_ce_z_fwd_bwd_q8"))
            m.store.zero_grad()
            out = m(ids, labels=ids)
            out.loss.backward()
            torch.cuda.synchronize()
            m.fp8.recipe.update()
            ran.append((spy.ran("nd_ce_z_fwd_bwd") - before[0], spy.ran("nd_ce_z_fwd_bwd_q8") - before[1]))
            assert bool(torch.isfinite(m.store.grad).all()) and bool(m.store.grad.any()), step
            assert bool(torch.isfinite(out.loss)) and 0.5 < float(out.z_loss) < 2.0
            assert torch.equal(out.loss.detach(), out.ce_loss + out.z_loss)
    print(f"[z-loss] fp8 model: launchers {dict(sorted(spy.calls.items()))} refused {dict(spy.refused)}")
    assert ran == [(1, 0), (0, 1), (0, 1)], ran
    assert spy.calls["nd_ce_fwd_bwd"] == 0 and spy.calls["nd_ce_fwd_bwd_q8"] == 0
