"""Logit soft-capping on the HIP path: the CAP instantiations of ``csrc/cross_entropy.hip`` (``nd_ce_cap_fwd_bwd``,
``nd_ce_cap_fwd_bwd_q8``), the capped loss-only kernel and ``nd_logit_softcap`` (``csrc/ce_loss.hip``) per element
against the float64 oracle of ``tests/_softcap.py`` (checked on the CPU by ``tests/test_softcap_cpu.py``),
``ops.lm_head_ce(..., softcap=)``, and the model with ``final_logit_softcapping`` set -- eager, captured, with the fp8
lm head, and decoding.

Error rule: ``_oracle64.check`` (bf16 outputs: half an ulp relative plus slack; fp32 outputs: slack; slack = margin
x the error of the fp32 PyTorch twin of the same formulae -- ``torch.tanh`` and ``1 - t * t`` -- on the same inputs),
margin 8 except ``MARGINS``.  Every case prints the margin it needed; docs/PARITY.md ("Logit soft-capping") has the
table.

``MARGINS`` is empty: on the MI355X no output needed more than 3.34 (``capz.ce_bf16.z_sum``; the dlogits 2.99 at
most).  The packed kernel's log2-domain ``lse``, which needs 3.87 and 14.3 in its uncapped z-loss siblings, needs 1
here: its first product is C log2(e) t <= 11.5 instead of 60 log2(e).  Should an output ever need more than 8: read its
"needs margin" line, derive where the error comes from as tests/test_zloss_gpu.py does, allow the next power of two at
or above twice the measured need, and record both in docs/PARITY.md.

``nd_logit_softcap`` has a rule of its own, relative per element (``REL``): the value is u = x * (1/C) (two roundings,
2 x 2^-24), then below |u| = 1/4 an odd series (three fused steps, 1.5 x 2^-24; truncation < 2^-26) and above it
(1 - e) / (1 + e) with e = exp(-2|u|) from v_exp_f32 (1 ulp = 2^-23 of e <= 0.61, over 1 - e >= 0.39: 3.1 x 2^-24 at
the border and falling), 1 + e and v_rcp_f32 (0.5 + 2) and the product (0.5), and the product with C (0.5): under
10 x 2^-24 in all, and REL = 2^-20 = 16 x 2^-24.  bf16 results add the half ulp of their one rounding, 2^-8.
"""
import dataclasses
import os

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.config import LlamaConfig
from nanodiloco_amd.models import LlamaForCausalLM
from nanodiloco_amd.ops import _ext
from nanodiloco_amd.ops import fp8

from . import _oracle64 as o64
from . import _softcap as sc
from ._frames import assert_frame_intact, framed_flat
from ._switches import switches

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
IGN = sc.IGN
INVALID = 1  # hipErrorInvalidValue
CAP = 8.0  # exact as a C float
ZC = o64.f32_scalar(1e-2)
CE_V = [8, 100, 1001, 8192, 8200, 32768, 32776]
N_PAT, N_ROWS = 5, 30
REL = 2.0 ** -20

MARGINS = {}
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
    print(f"[softcap] {name}{' ' + note if note else ''}: needs margin {ratio:.3g}")
    o64.check(out, ref64, twin32, margin=MARGINS.get(name, o64.MARGIN), name=name, rel=rel, report=REPORT, note=note)


def S():
    return _ext.stream_ptr(torch.device(DEV))


def scalar(v):
    return torch.tensor([v], dtype=F32, device=DEV)


def _bits(t):
    return t.detach().contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ------------------------------------------------------------------------------------------ the kernels alone
def _kernel_name(V, dt):
    if V % 8 or V > 32768:
        return "ce_generic"
    if V <= 8192:
        return "ce_reg4"
    return "ce_bf16" if dt == BF16 else "ce_reg16"


def _inputs(V, dt):
    """30 rows: five logit patterns (4 randn; one +60 among -60; constant 1.5; -20 + randn; 4 randn with every third
    column at +300 and the next at -300, which saturates the cap: a naive (e - 1) / (e + 1) gives NaN there) x six
    targets (0, V - 1, a column of the last partial 8-chunk, a middle column, ignore_index, the row's arg-max); every
    pattern meets every kind of target."""
    n = N_ROWS
    x = 4 * torch.randn(n, V, device=DEV)
    peak = [V - 1, 0, max(0, V - 3), V // 2, V // 3, (V - 1) // 8 * 8]
    for k, r in enumerate(range(1, n, N_PAT)):
        x[r] = -60.0
        x[r, peak[k]] = 60.0
    x[2::N_PAT] = 1.5
    x[3::N_PAT] = -20.0 + torch.randn(n // N_PAT, V, device=DEV)
    x[4::N_PAT, 0::3] = 300.0
    x[4::N_PAT, 1::3] = -300.0
    x = x.to(dt)
    tgt = torch.empty(n, dtype=torch.long, device=DEV)
    kinds = [0, V - 1, max(0, V - 3), V // 2, IGN, None]
    for r in range(n):
        k = kinds[(r // N_PAT + r % N_PAT) % 6]
        tgt[r] = int(x[r].float().argmax()) if k is None else k
    return x, tgt


def _run(x, tgt, scale, with_rows, z, ce0=3.0, z0=5.0, cap=CAP):
    """nd_ce_cap_fwd_bwd on framed buffers: (dlogits, lse, row CE, row lse^2, CE sum, lse^2 sum); ``z``: the z
    coefficient, 0.0 = the entry without z-loss (no z_sum, no row_z)."""
    n, V = x.shape
    big, flat = framed_flat(n * V, x.dtype, pad=64)
    logits = flat.view(n, V)
    logits.copy_(x)
    lbig, lse = framed_flat(n, F32)
    rbig, rows = framed_flat(n, F32)
    zbig, rows_z = framed_flat(n, F32)
    ce_sum, z_sum = torch.full((1,), ce0, device=DEV), torch.full((1,), z0, device=DEV)
    _ext.check(_ext.lib().nd_ce_cap_fwd_bwd(logits.data_ptr(), _ext.dtcode(x), tgt.data_ptr(), ce_sum.data_ptr(),
                                            z_sum.data_ptr() if z else 0, scale.data_ptr(), n, V, IGN, lse.data_ptr(),
                                            rows.data_ptr() if with_rows else 0,
                                            rows_z.data_ptr() if with_rows and z else 0, z, cap, S()),
               "nd_ce_cap_fwd_bwd")
    assert_frame_intact(big, flat)
    assert_frame_intact(lbig, lse)
    assert_frame_intact(rbig, rows if with_rows else None)
    assert_frame_intact(zbig, rows_z if with_rows and z else None)
    return logits, lse, rows, rows_z, ce_sum, z_sum


def _alone(V, dt, k, z):
    x, tgt = _inputs(V, dt)
    n_valid = int((tgt != IGN).sum())
    scale = scalar(0.25 / n_valid)
    lse64, ce64, z64, dl64 = sc.ce_cap_rows(x, tgt, scale.item(), z, CAP)
    lse32, ce32, z32, dl32 = sc.ce_cap_rows_twin(x.float(), tgt, scale, z, CAP)
    d = 1.0 - torch.tanh(x.double() / CAP) ** 2
    assert float(d.min()) < 0.1 and float(d.max()) > 0.95  # a missing or misplaced factor is far outside the rule
    assert bool((x.float().abs() == 300.0).any())
    p = ("capz." if z else "cap.") + k
    dl, lse, rows, rows_z, ce_sum, z_sum = _run(x, tgt, scale, True, z)
    chk(dl, dl64, dl32, f"{p}.dlogits", note=f"V={V}")
    chk(lse, lse64, lse32, f"{p}.lse")
    chk(rows, ce64, ce32, f"{p}.row_ce")
    if z:
        chk(rows_z, z64, z32, f"{p}.row_z")
    ign = tgt == IGN
    assert not bool(dl[ign].any()) and not bool(rows[ign].any()) and (not z or not bool(rows_z[ign].any()))
    assert ce_sum.item() == 3.0 and z_sum.item() == 5.0  # per-row outputs given: no atomic, the sums are not touched
    dl2, lse2, _, _, _, _ = _run(x, tgt, scale, False, z)
    assert torch.equal(dl2, dl) and torch.equal(lse2, lse)
    # the atomic sums, one launch per group of five rows: six-element tensors for the rule
    sums = [_run(x[a:a + N_PAT], tgt[a:a + N_PAT], scale, False, z, 0.0, 0.0)[4:] for a in range(0, N_ROWS, N_PAT)]
    chk(torch.cat([s[0] for s in sums]), ce64.reshape(6, N_PAT).sum(1), ce32.reshape(6, N_PAT).sum(1), f"{p}.ce_sum")
    if z:
        chk(torch.cat([s[1] for s in sums]), z64.reshape(6, N_PAT).sum(1), z32.reshape(6, N_PAT).sum(1), f"{p}.z_sum")
    else:
        assert all(s[1].item() == 0.0 for s in sums)
    # an all-ignored batch: all-zero outputs, accumulators untouched
    none = torch.full_like(tgt, IGN)
    dl, _, rows, rows_z, _, _ = _run(x, none, scale, True, z)
    assert not bool(dl.any()) and not bool(rows.any()) and (not z or not bool(rows_z.any()))
    dl, _, _, _, ce_sum, z_sum = _run(x, none, scale, False, z)
    assert not bool(dl.any()) and ce_sum.item() == 3.0 and z_sum.item() == 5.0


@pytest.mark.parametrize("z", [0.0, ZC], ids=["ce", "ce+z"])
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", CE_V)
def test_ce_cap_kernel_alone(V, dt, z):
    """nd_ce_cap_fwd_bwd on given logits, C = 8, both sides of the dispatch borders at 8192 and 32768 and V % 8 != 0,
    with and without z-loss, with and without per-row outputs: every dlogits element, lse, the per-row CE and lse^2
    and the atomic sums against float64; bf16 rows that take the packed kernel run once more under ND_CE=r."""
    k = _kernel_name(V, dt)
    _alone(V, dt, k, z)
    if k == "ce_bf16":
        with switches(ND_CE="r") as state:
            assert state["ND_CE"] == "r"
            _alone(V, dt, "ce_reg16", z)


def test_cap_entries_refuse_bad_arguments():
    """A cap that is <= 0, NaN or infinite (and a z coefficient without its accumulator, or a bad one with it) gives
    hipErrorInvalidValue from every capped launcher, and nothing is written."""
    x, tgt = _inputs(100, F32)
    d = x.clone()
    ce, z = scalar(3.0), scalar(5.0)
    rows, hit = torch.full((N_ROWS,), 7.0, device=DEV), torch.full((N_ROWS,), 9, dtype=torch.uint8, device=DEV)
    L = _ext.lib()
    one = scalar(1.0)
    bad_caps = (0.0, -1.0, float("nan"), float("inf"), -float("inf"))
    for cap in bad_caps:
        assert L.nd_ce_cap_fwd_bwd(d.data_ptr(), _ext.dtcode(d), tgt.data_ptr(), ce.data_ptr(), 0, one.data_ptr(),
                                   N_ROWS, 100, IGN, 0, 0, 0, 0.0, cap, S()) == INVALID
        assert L.nd_ce_cap_fwd_bwd(d.data_ptr(), _ext.dtcode(d), tgt.data_ptr(), ce.data_ptr(), z.data_ptr(),
                                   one.data_ptr(), N_ROWS, 100, IGN, 0, 0, 0, ZC, cap, S()) == INVALID
        assert L.nd_ce_loss_cap(d.data_ptr(), _ext.dtcode(d), tgt.data_ptr(), N_ROWS, 100, IGN, rows.data_ptr(), 0,
                                hit.data_ptr(), cap, S()) == INVALID
        assert L.nd_logit_softcap(d.data_ptr(), _ext.dtcode(d), d.numel(), cap, S()) == INVALID
    for coef, zp in ((-1.0, z.data_ptr()), (float("nan"), z.data_ptr()), (float("inf"), z.data_ptr()), (ZC, 0)):
        assert L.nd_ce_cap_fwd_bwd(d.data_ptr(), _ext.dtcode(d), tgt.data_ptr(), ce.data_ptr(), zp, one.data_ptr(),
                                   N_ROWS, 100, IGN, 0, 0, 0, coef, CAP, S()) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(d, x) and ce.item() == 3.0 and z.item() == 5.0
    assert bool((rows == 7.0).all()) and bool((hit == 9).all())


# ------------------------------------------------------------------------------------------ fp8 dlogits
PRIOR = 2.0 ** -24


def _target(fmt, scale):
    r = fp8.Fp8Recipe(DEV, capacity=4)
    k = r.new_slot(fmt)
    r.scale[k] = scale
    r.ready[k] = True
    r.amax.fill_(PRIOR)
    return r, k, r.target(k, fmt)


def _q8(x, tgt, scale, fmt, z, cap=CAP, qscale=2000.0):
    """nd_ce_cap_fwd_bwd_q8 on framed logits and a framed fp8 output: (q, recipe, slot, CE sum, z sum, rc)."""
    n, V = x.shape
    lbig, lflat = framed_flat(n * V, x.dtype, pad=64)
    logits = lflat.view(n, V)
    logits.copy_(x)
    r, k, t = _target(fmt, qscale)
    big, qflat = framed_flat(n * V, fp8.TORCH_DT[fmt], pad=64)
    ce, zs = scalar(3.0), scalar(5.0)
    rc = _ext.lib().nd_ce_cap_fwd_bwd_q8(logits.data_ptr(), _ext.dtcode(logits), tgt.data_ptr(), ce.data_ptr(),
                                         zs.data_ptr() if z else 0, scale.data_ptr(), n, V, IGN, 0, 0, 0, z, cap,
                                         *t.args(qflat), S())
    torch.cuda.synchronize()
    assert_frame_intact(lbig, lflat)
    assert torch.equal(_bits(logits), _bits(x)), "the logits were modified"
    assert_frame_intact(big, qflat if rc == 0 else None)
    return qflat.view(n, V), r, k, ce, zs, rc


@pytest.mark.parametrize("z", [0.0, ZC], ids=["ce", "ce+z"])
@pytest.mark.parametrize("V", [8200, 32768])
@pytest.mark.parametrize("fmt", [fp8.E4M3, fp8.E5M2], ids=["e4m3", "e5m2"])
def test_ce_cap_q8_is_the_cast_of_the_bf16_dlogits(fmt, V, z):
    """V at the two ends of what the q8 entry accepts: its bytes and amax are bitwise nd_fp8_cast over the bf16
    dlogits of nd_ce_cap_fwd_bwd, partial slot by partial slot (row b -> b % parts); the logits buffer is left as
    given; the sums are those of the bf16 entry."""
    x, tgt = _inputs(V, BF16)
    scale = scalar(1.0 / 16)
    d, _, _, _, ce_ref, z_ref = _run(x, tgt, scale, False, z)
    q, r, k, ce, zs, rc = _q8(x, tgt, scale, fmt, z)
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
    for got, ref in ((ce, ce_ref), (zs, z_ref)):  # float atomics over 25 rows: equal up to their order
        assert abs(got.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert _q8(x, tgt, scale, fmt, z, cap=float("nan"))[5] == INVALID  # a bad cap: refused, nothing written


@pytest.mark.parametrize("case", ["V=8192", "V=32776", "fp32", "ND_CE=r"])
def test_ce_cap_q8_refuses_outside_its_range(case):
    V = {"V=8192": 8192, "V=32776": 32776}.get(case, 8200)
    x, tgt = _inputs(V, F32 if case == "fp32" else BF16)
    if case == "ND_CE=r":
        with switches(ND_CE="r"):
            q, r, k, ce, z, rc = _q8(x, tgt, scalar(1.0 / 16), fp8.E5M2, ZC)
    else:
        q, r, k, ce, z, rc = _q8(x, tgt, scalar(1.0 / 16), fp8.E5M2, ZC)
    assert rc == INVALID  # _q8 has checked that neither the logits nor any byte of the output frame changed
    assert ce.item() == 3.0 and z.item() == 5.0 and bool((r.amax == PRIOR).all())


# ------------------------------------------------------------------------------------------ loss only
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [100, 1001, 8200])
def test_ce_loss_cap(V, dt):
    """nd_ce_loss_cap (the vector kernel at V % 8 == 0, else the scalar one): per-row loss and lse against float64,
    row_hit bitwise the uncapped call's (the top-1 of the stored logits: in the saturated pattern +300 and the randn
    maximum cap to different values only in the stored domain)."""
    x, tgt = _inputs(V, dt)
    lse64, ce64, _, _ = sc.ce_cap_rows(x, tgt, 1.0, 0.0, CAP)
    lse32, ce32, _, _ = sc.ce_cap_rows_twin(x.float(), tgt, 1.0, 0.0, CAP)
    L = _ext.lib()
    out = {}
    for cap in (0.0, CAP):
        rbig, rows = framed_flat(N_ROWS, F32)
        lbig, lse = framed_flat(N_ROWS, F32)
        hbig, hit = framed_flat(N_ROWS, torch.uint8)
        xin = x.clone()
        if cap:
            _ext.check(L.nd_ce_loss_cap(xin.data_ptr(), _ext.dtcode(x), tgt.data_ptr(), N_ROWS, V, IGN, rows.data_ptr(),
                                        lse.data_ptr(), hit.data_ptr(), cap, S()), "nd_ce_loss_cap")
        else:
            _ext.check(L.nd_ce_loss(xin.data_ptr(), _ext.dtcode(x), tgt.data_ptr(), N_ROWS, V, IGN, rows.data_ptr(),
                                    lse.data_ptr(), hit.data_ptr(), S()), "nd_ce_loss")
        torch.cuda.synchronize()
        for big, view in ((rbig, rows), (lbig, lse), (hbig, hit)):
            assert_frame_intact(big, view)
        assert torch.equal(_bits(xin), _bits(x))
        out[cap] = (rows.clone(), lse.clone(), hit.clone())
    rows, lse, hit = out[CAP]
    k = "ce_loss_vec" if V % 8 == 0 else "ce_loss_scalar"
    chk(rows, ce64, ce32, f"cap.{k}.row_loss", note=f"V={V}")
    chk(lse, lse64, lse32, f"cap.{k}.lse")
    assert torch.equal(hit, out[0.0][2]) and bool(hit.any()) and not bool(hit.all())
    assert not torch.equal(rows, out[0.0][0]) and not bool(rows[tgt == IGN].any())


# ------------------------------------------------------------------------------------------ nd_logit_softcap
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [1, 7, 4099])
def test_logit_softcap_kernel(n, dt):
    """In place over [n] at a base that is not 16-byte aligned (head, 16-byte body and tail all occur at 4099): every
    element inside REL of the float64 value of the stored input; 0 stays 0, +-300 gives exactly +-C, NaN stays NaN,
    +-1e-4 keeps its value (no cancellation); the frame around the buffer is intact."""
    special = torch.tensor([1e-4, -1e-4, 0.0, CAP, -CAP, 300.0, -300.0, float("nan"), 1.99, -2.01, 0.3],
                           dtype=F32, device=DEV)  # 1.99 and -2.01: either side of the series' border, |x / C| = 1/4
    v = CAP * torch.randn(n, device=DEV)
    k = min(n, special.numel())
    v[torch.linspace(0, n - 1, k, device=DEV).long()] = special[:k]  # spread over head, body and tail
    v = v.to(dt)
    big, x = framed_flat(n, dt, pad=17)
    assert x.data_ptr() % 16 != 0
    x.copy_(v)
    _ext.check(_ext.lib().nd_logit_softcap(x.data_ptr(), _ext.dtcode(x), n, CAP, S()), "nd_logit_softcap")
    torch.cuda.synchronize()
    assert_frame_intact(big, x)
    ref = sc.softcap64(v, CAP)
    nan = torch.isnan(v)
    assert bool(torch.isnan(x[nan]).all()) and not bool(torch.isnan(x[~nan]).any())
    rel = REL + (o64.BF16_HALF_ULP if dt == BF16 else 0.0)
    err = (x.double() - ref).abs()[~nan]
    worst = float((err / ref.abs()[~nan].clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"[softcap] nd_logit_softcap n={n} {dt}: worst relative error {worst:.3g} (allowed {rel:.3g})")
    assert bool((err <= rel * ref.abs()[~nan]).all()), worst
    big_in = v.float().abs() == 300.0
    assert torch.equal(x[big_in].float(), CAP * torch.sign(v[big_in].float()))
    assert bool((x[v.float() == 0.0] == 0.0).all())
    # the op: the same bits, in place, on the tensor it was given
    y = v.clone()
    assert ops.logit_softcap(y, CAP) is y and torch.equal(_bits(y[~nan]), _bits(x[~nan]))


# ------------------------------------------------------------------------------------------ lm_head_ce
OP_CAP = 0.5  # logits of std 0.4: the cap acts on every row


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


@pytest.mark.parametrize("z", [0.0, ZC], ids=["ce", "ce+z"])
@pytest.mark.parametrize("V", [1000, 8200])
def test_lm_head_ce_cap(V, z):
    """The whole op, two chunks (one ragged), bf16: loss parts, y.grad and gW against the float64 oracle of the op on
    the stored operands; the twin is the same op under set_backend("torch").

    The loss carries one more term than the rule's slack: the HIP path stores the logits in bf16 where the twin keeps
    them in fp32, so each logit is off by up to 2^-9 |x| before the cap, whose slope is at most 1: lse and y_t by up
    to 2^-9 max|x| each, the CE row by 2^-8 max|x|.  That worst case, relative to the oracle's value, is ``rel``."""
    from ._model_oracle import spying
    n, d = 320, 256
    y0 = (0.5 * torch.randn(n, d, device=DEV)).bfloat16()
    W = (0.05 * torch.randn(V, d, device=DEV)).bfloat16()
    tgt = torch.randint(0, V, (n,), device=DEV)
    tgt[::10] = IGN
    ce64, z64, dy64, gw64 = sc.lm_head_ce_cap(y0, W, tgt, 0.25, z, OP_CAP)
    x64 = y0.double() @ W.double().t()
    dd = 1 - torch.tanh(x64 / OP_CAP) ** 2
    assert float(dd.min()) < 0.1 and float(dd.max()) > 0.95
    xmax = float(x64.abs().max())
    twin, dy32, gw32 = _lm_head(y0, W, tgt, "torch", z_loss=z, softcap=OP_CAP)
    with spying() as spy:
        got, dy, gw = _lm_head(y0, W, tgt, "hip", z_loss=z, softcap=OP_CAP)
    assert spy.ran("nd_ce_cap_fwd_bwd") == 2 and not spy.ran("nd_ce_fwd_bwd") and not spy.ran("nd_ce_z_fwd_bwd")
    p = "capz" if z else "cap"
    chk(got.ce_loss.reshape(1), ce64.reshape(1), twin.ce_loss.reshape(1), f"{p}.lm_head.ce",
        rel=2.0 ** -8 * xmax / float(ce64))
    if z:
        lsemax = OP_CAP + float(torch.log(torch.tensor(float(V))))
        chk(got.z_loss.reshape(1), z64.reshape(1), twin.z_loss.reshape(1), f"{p}.lm_head.z",
            rel=ZC * 2.0 * lsemax * 2.0 ** -9 * xmax / float(z64))
        assert torch.equal(got.loss.detach(), got.ce_loss + got.z_loss)
    else:
        assert got.z_loss is None and torch.equal(got.loss.detach(), got.ce_loss)
    chk(dy, dy64, dy32, f"{p}.lm_head.dy", note=f"V={V}")
    chk(gw, gw64, gw32, f"{p}.lm_head.gW", note=f"V={V}")
    # softcap = 0.0 is the call that omits the argument: the same launches, bit for bit (deterministic mode so that
    # the loss is too)
    ops.set_deterministic(True)
    kw = dict(z_loss=z) if z else {}
    with spying() as spy_a:
        a, dya, gwa = _lm_head(y0, W, tgt, "hip", **kw)
    with spying() as spy_b:
        b, dyb, gwb = _lm_head(y0, W, tgt, "hip", softcap=0.0, **kw)
    assert dict(spy_a.calls) == dict(spy_b.calls) and not spy_b.calls["nd_ce_cap_fwd_bwd"]
    assert torch.equal(a.loss, b.loss) and torch.equal(dya, dyb) and torch.equal(gwa, gwb)
    # the deterministic capped path (per-row outputs, no float atomic) repeats bitwise and agrees with the atomic one
    c1, dyc1, gwc1 = _lm_head(y0, W, tgt, "hip", z_loss=z, softcap=OP_CAP)
    c2, dyc2, gwc2 = _lm_head(y0, W, tgt, "hip", z_loss=z, softcap=OP_CAP)
    assert torch.equal(c1.loss, c2.loss) and torch.equal(c1.ce_loss, c2.ce_loss)
    assert torch.equal(dyc1, dy) and torch.equal(gwc1, gw) and torch.equal(dyc2, dy)
    assert abs(float(c1.ce_loss) - float(got.ce_loss)) <= 1e-5 * float(got.ce_loss)
    assert not torch.equal(dya, dy)
    # the loss-only op on the same operands: the capped entry, the rows of the deterministic path's sum
    with spying() as spy:
        row_loss, row_hit = ops.lm_head_loss(y0, W, tgt, chunk_rows=256, softcap=OP_CAP)
        loss0, hit0 = ops.lm_head_loss(y0, W, tgt, chunk_rows=256)
    assert spy.ran("nd_ce_loss_cap") == 2 and spy.ran("nd_ce_loss") == 2
    assert torch.equal(row_hit, hit0) and not torch.equal(row_loss, loss0)
    n_valid = int((tgt != IGN).sum())
    assert abs(float(row_loss.sum()) / n_valid - float(c1.ce_loss)) <= 1e-4 * float(c1.ce_loss)


# ------------------------------------------------------------------------------------------ model and graph
MODEL_CAP = 0.0625  # the tiny model's initial logits are of this size: the cap bends every one of them


def _tiny(cap=None):
    cfg = LlamaConfig.from_json(os.path.join(ROOT, "configs", "llama_tiny.json"))
    return dataclasses.replace(cfg, final_logit_softcapping=cap) if cap else cfg


def _ids(seed, vocab):
    return torch.randint(0, vocab, (4, 64), device=DEV, generator=torch.Generator(DEV).manual_seed(seed))


def _eager(m, ids):
    m.store.zero_grad()
    out = m(ids, labels=ids, loss_scale=0.5)
    out.loss.backward()
    torch.cuda.synchronize()
    return (out.loss.detach().clone(), out.ce_loss.clone(), None if out.z_loss is None else out.z_loss.clone(),
            m.store.grad.clone())


@pytest.mark.parametrize("z", [0.0, 1e-2], ids=["ce", "ce+z"])
def test_model_cap_eager_and_graph_bitwise(z):
    """The tiny model with final_logit_softcapping, 4 x 64 tokens, deterministic mode: two eager passes agree bitwise
    in loss, its parts and the flat grad buffer; GraphedMicroStep (two warm-ups, capture, two replays) returns the
    same bits; against the cap-free model (same weights) loss and gradient differ; a cap changed after capture is
    refused."""
    from nanodiloco_amd.utils.graphs import GraphedMicroStep
    ops.set_deterministic(True)
    ids = _ids(1, _tiny().vocab_size)
    m0 = LlamaForCausalLM(_tiny(), DEV, BF16).init_weights(3)
    m0.z_loss = z
    l0, ce0, _, g0 = _eager(m0, ids)
    m = LlamaForCausalLM(_tiny(MODEL_CAP), DEV, BF16).init_weights(3)
    m.z_loss = z
    assert m.softcap == MODEL_CAP
    l1, ce1, z1, g1 = _eager(m, ids)
    l2, ce2, z2, g2 = _eager(m, ids)
    assert torch.equal(l1, l2) and torch.equal(ce1, ce2) and torch.equal(g1, g2) and (z1 is None) == (not z)
    assert not torch.equal(ce1, ce0) and not torch.equal(g1, g0) and bool(torch.isfinite(g1).all()) and bool(g1.any())
    g = GraphedMicroStep(m)
    for call in range(5):  # 2 eager warm-ups, capture + replay, 2 more replays
        m.store.zero_grad()
        loss = g(ids, ids, 0.5)
        torch.cuda.synchronize()
        assert torch.equal(loss, l1) and torch.equal(g.ce_loss, ce1), call
        assert torch.equal(m.store.grad, g1), call
    assert g.graph is not None
    ids2 = _ids(2, m.config.vocab_size)
    m.store.zero_grad()
    loss = g(ids2, ids2, 0.5).clone()
    grad_g = m.store.grad.clone()
    l3, _, _, g3 = _eager(m, ids2)
    assert torch.equal(loss, l3) and torch.equal(grad_g, g3) and not torch.equal(l3, l1)
    m.softcap = 2 * MODEL_CAP
    with pytest.raises(ValueError, match="softcap changed"):
        g(ids, ids, 0.5)


def test_fp8_model_cap_runs_the_q8_entry():
    """The tiny model with the fp8 projections and the cap: the first step (no scale yet) takes the bf16 capped entry
    plus the cast, later steps the capped q8 entry; the cap-free entries never run; every gradient is finite."""
    from ._model_oracle import spying
    cfg = _tiny(MODEL_CAP)
    ids = _ids(1, cfg.vocab_size)
    m = LlamaForCausalLM(cfg, DEV, BF16, fp8=True, fp8_wgrad=True).init_weights(3)
    ran = []
    with spying() as spy:
        for step in range(3):
            before = (spy.ran("nd_ce_cap_fwd_bwd"), spy.ran("nd_ce_cap_fwd_bwd_q8"))
            m.store.zero_grad()
            out = m(ids, labels=ids)
            out.loss.backward()
            torch.cuda.synchronize()
            m.fp8.recipe.update()
            ran.append((spy.ran("nd_ce_cap_fwd_bwd") - before[0], spy.ran("nd_ce_cap_fwd_bwd_q8") - before[1]))
            assert bool(torch.isfinite(m.store.grad).all()) and bool(m.store.grad.any()), step
            assert bool(torch.isfinite(out.loss)) and out.z_loss is None
    print(f"[softcap] fp8 model: launchers {dict(sorted(spy.calls.items()))} refused {dict(spy.refused)}")
    assert ran == [(1, 0), (0, 1), (0, 1)], ran
    for name in ("nd_ce_fwd_bwd", "nd_ce_fwd_bwd_q8", "nd_ce_z_fwd_bwd", "nd_ce_z_fwd_bwd_q8"):
        assert spy.calls[name] == 0, name


def test_model_logits_are_capped():
    """forward().logits, prefill and decode_step of the capped model against the float64 cap of the cap-free model's
    logits (the same weights, the same kernels up to the lm head), inside REL per element; loss_stats runs the capped
    loss-only entry; generation with a captured decode step gives the eager tokens."""
    from ._model_oracle import spying
    m0 = LlamaForCausalLM(_tiny(), DEV, BF16).init_weights(3)
    m1 = LlamaForCausalLM(_tiny(MODEL_CAP), DEV, BF16).init_weights(3)
    ids = _ids(1, m0.config.vocab_size)[:2, :32].contiguous()

    def same(got, raw):
        ref = sc.softcap64(raw, MODEL_CAP)
        assert float(raw.abs().max()) > MODEL_CAP and float(got.abs().max()) <= MODEL_CAP
        assert bool(((got.double() - ref).abs() <= REL * ref.abs()).all())

    with spying() as spy:
        same(m1(ids).logits, m0(ids).logits)
        c0, c1 = m0.new_cache(2, 40), m1.new_cache(2, 40)
        p0, p1 = m0.prefill(ids, None, c0), m1.prefill(ids, None, c1)
        same(p1, p0)
        tok = p0.argmax(-1)
        same(m1.decode_step(tok, c1), m0.decode_step(tok, c0))
        assert spy.ran("nd_logit_softcap") == 3
        s1, s0 = m1.loss_stats(ids, ids), m0.loss_stats(ids, ids)
        assert spy.ran("nd_ce_loss_cap") >= 1
    assert torch.equal(s1[1:], s0[1:]) and float(s1[0]) != float(s0[0])
    a = m1.generate(ids, max_new_tokens=6, hip_graph=True)
    b = m1.generate(ids, max_new_tokens=6, hip_graph=False)
    assert torch.equal(a, b)
