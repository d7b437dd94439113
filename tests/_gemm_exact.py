"""Inputs for which the MFMA GEMMs' fp32 accumulator is EXACT, the exact products, a bitwise comparison that
localises a failure, and float64 oracles (with fp32 twins) of the fused epilogues of ``csrc/gemm_pp.hip``.

Plain PyTorch; nothing here calls the code under test.  ``tests/test_gemm_exact_cpu.py`` checks these helpers on
the CPU, ``tests/test_gemm_exact_gpu.py`` uses them against the HIP kernels.

The exactness argument: operands are small integers (|a| <= amax, |b| <= bmax), exactly representable in bf16,
e4m3 and e5m2.  Every product is an integer and every partial sum of any subset of the K products, plus an
integer-valued initial value |c| <= cmax, has magnitude <= K * amax * bmax + cmax (``exact_bound``).  Below 2^24
every such integer is an fp32 number, so the fp32 accumulator is exact in any summation order, with any split-K
and any tile walk: fp32 outputs must equal the integer product bit for bit, bf16 outputs its one rounding.

The epilogue-isolating inputs (``iso_operands``): x in {-1, 0, 1}, w in {-1, 0, 1} / 16, K <= 256.  The product is
a multiple of 1/16 of magnitude <= K / 16 <= 16, i.e. n / 16 with |n| <= 256: 9 significant bits at most (256 itself
is a power of two), exactly representable in bf16.  The bf16 rounding between the accumulator and the epilogue
(``rbf(acc)`` in ``pp_epilogue``, the stored ``gu`` of form 0) is then the identity and the oracle knows the
epilogue's input exactly, whatever the saved form or the operand type.
"""
import torch

from . import _oracle64 as O

E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
EXACT_LIMIT = 2 ** 24


# ------------------------------------------------------------------------------------------ inputs
def int_operand(rows, cols, lo, hi, dtype, seed, device="cpu"):
    """Integer-valued [rows, cols] tensor, uniform in [lo, hi], as bf16 / e4m3 / e5m2 (drawn on the CPU from
    ``seed``: the same values wherever they are used)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(lo, hi + 1, (rows, cols), generator=g).float()
    out = x.to(dtype)
    assert torch.equal(out.float(), x), "not representable"
    return out.to(device)


def exact_bound(K, amax, bmax, cmax=0):
    """The largest magnitude any partial sum of a K-term product of |a| <= amax, |b| <= bmax on top of an
    initial |c| <= cmax can take."""
    return K * amax * bmax + cmax


def iso_operands(M, N, K, seed, device="cpu", f8=False, adt=E4):
    """The epilogue-isolating pair.  bf16: (x [M, K] in {-1, 0, 1}, w [N, K] in {-1, 0, 1} / 16).  fp8: the same
    values as (x8 = 2 x, sa = 1/2, w8 = 16 w, sb = 1/16): x8 in ``adt``, w8 e4m3, power-of-two scales, so the
    dequantised product is the same multiple of 1/16.  Returns (x, w, sa, sb); sa = sb = None for bf16."""
    assert K <= 256
    x = int_operand(M, K, -1, 1, torch.bfloat16, seed, device)
    w = int_operand(N, K, -1, 1, torch.bfloat16, seed + 1, device)
    if not f8:
        return x, (w.float() / 16).bfloat16(), None, None
    sa = torch.tensor([0.5], device=device)
    sb = torch.tensor([1.0 / 16], device=device)
    return (x.float() * 2).to(adt), w.float().to(E4), sa, sb


# ------------------------------------------------------------------------------------------ exact products
def _f64(t):
    return t.float().double()  # fp8 -> fp32 is exact; fp8 has no direct widening to float64 everywhere


def exact_nt(a, b, scale=1.0):
    """float64 a[M, K] . b[N, K]^T (* scale)."""
    return (_f64(a) @ _f64(b).t()) * scale


def exact_tn(dy, x, gw0=None, scale=1.0):
    """float64 gw0[M, N] + scale * dy[K, M]^T . x[K, N]."""
    p = (_f64(dy).t() @ _f64(x)) * scale
    return p if gw0 is None else gw0.double() + p


# ------------------------------------------------------------------------------------------ bitwise comparison
def _ints(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def to_dtype(ref64, dtype):
    """``ref64`` in ``dtype`` with ONE rounding where ref64 is an fp32 number (every exact product here is)."""
    return ref64.float().to(dtype)


def _residues(idx):
    out = []
    for m in (16, 64, 128):
        r = torch.unique(idx % m)
        if r.numel() == 1:
            out.append(f"all = {int(r[0])} mod {m}")
    return ", ".join(out) if out else "no common residue mod 16 / 64 / 128"


def describe_mismatch(out, ref64, tile=256):
    """None when ``out`` equals ``ref64`` cast to its dtype bit for bit, else the failure report (text)."""
    assert out.shape == ref64.shape and out.dim() == 2, (out.shape, ref64.shape)
    exp = to_dtype(ref64, out.dtype)
    bad = _ints(out) != _ints(exp)
    if not bool(bad.any()):
        return None
    rows, cols = torch.nonzero(bad, as_tuple=True)
    r, c = int(rows[0]), int(cols[0])
    r0, r1, c0, c1 = int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())
    return (f"{int(bad.sum())} of {bad.numel()} elements differ in bits; first at ({r}, {c}): "
            f"out={out[r, c].float().item()!r} expected={exp[r, c].float().item()!r} exact={ref64[r, c].item()!r}; "
            f"bad rows {r0}..{r1}, columns {c0}..{c1} "
            f"({tile} x {tile} tiles ({r0 // tile}, {c0 // tile})..({r1 // tile}, {c1 // tile})); "
            f"rows: {_residues(rows)}; columns: {_residues(cols)}")


def expect_bits(out, ref64, name=""):
    """Assert ``out`` == ``ref64`` cast to ``out.dtype``, compared as integers."""
    msg = describe_mismatch(out, ref64)
    assert msg is None, f"{name}: {msg}"


# ------------------------------------------------------------------------------------------ epilogue oracles
# Written from the header and pp_epilogue of csrc/gemm_pp.hip.  gu = [gate | up] is the bf16-rounded projection
# (with iso_operands: the exact one); s = sigmoid(gate).
#   forward, form 0:  stores gu and act = gate * s * up
#   forward, form 1:  stores [A | B], A = up s (1 + gate (1 - s)) = d act / d gate, B = gate s = d act / d up; act
#   backward, form 0: d(gate) = d up s (1 + gate (1 - s)), d(up) = d gate s from the saved gu
#   backward, form 1: d(gate) = d A, d(up) = d B from the saved bf16 [A | B]
def rope(exact, cos, sin, T, hd, rope_cols):
    """RoPE on the first ``rope_cols`` columns of the [B T, N] product, rows are tokens t = row % T."""
    M = exact.shape[0]
    assert M % T == 0 and rope_cols % hd == 0
    return O.rope(exact, cos, sin, M // T, T, rope_cols // hd, 0, hd)


def rope_twin(exact, cos, sin, T, hd, rope_cols):
    """The fp32 twin: rotate_half form, fp32 tables."""
    x = exact.float()
    M, half = x.shape[0], hd // 2
    t = torch.arange(M, device=x.device) % T
    c = cos[t, :half].float()[:, None, :]
    s = sin[t, :half].float()[:, None, :]
    blk = x[:, :rope_cols].reshape(M, rope_cols // hd, hd)
    x1, x2 = blk[..., :half], blk[..., half:]
    rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).reshape(M, rope_cols)
    return torch.cat([rot, x[:, rope_cols:]], dim=1)


def swiglu_act(gu):
    return O.swiglu_fwd(gu)


def swiglu_act_twin(gu):
    g, u = gu.float().chunk(2, dim=-1)
    return g * torch.sigmoid(g) * u


def swiglu_coef(gu):
    """[A | B] in float64."""
    g, u = gu.double().chunk(2, dim=-1)
    s = torch.sigmoid(g)
    return torch.cat([u * s * (1.0 + g * (1.0 - s)), g * s], dim=-1)


def swiglu_coef_twin(gu):
    g, u = gu.float().chunk(2, dim=-1)
    s = torch.sigmoid(g)
    return torch.cat([u * s * (1.0 + g * (1.0 - s)), g * s], dim=-1)


def dswiglu(dact, saved, form):
    """d(gate | up) in float64 from the exact d(act) [M, F] and the bf16 saved tensor [M, 2F] actually passed in."""
    if form == 0:
        return O.swiglu_bwd(dact, saved)
    d = dact.double()
    a, b = saved.double().chunk(2, dim=-1)
    return torch.cat([d * a, d * b], dim=-1)


def dswiglu_twin(dact, saved, form):
    d = dact.float()
    a, b = saved.float().chunk(2, dim=-1)
    if form == 0:
        s = torch.sigmoid(a)
        return torch.cat([d * b * s * (1.0 + a * (1.0 - s)), d * a * s], dim=-1)
    return torch.cat([d * a, d * b], dim=-1)
