"""float64 oracles of the row-wise and streaming ops, one per-element error rule, spiked test inputs.

Every function here is plain PyTorch in float64, written from the math in the kernel headers
(``csrc/norm.hip``, ``rope.hip``, ``swiglu.hip``, ``cross_entropy.hip``, ``embedding.hip``, ``optim.hip``,
``transpose.hip``, ``attention.hip``) and ``ops/reference.py``; none of them calls the code under test.  They run on whatever
device their inputs live on; ``tests/test_oracle64_cpu.py`` checks each against the project's torch twin
on the CPU, ``tests/test_rowwise_edges_gpu.py`` and ``tests/test_attention_edges_gpu.py`` use them against the
HIP kernels.

The error rule (``check``), per element:
  output stored as bf16:  |out - ref64| <= 2^-8 * |ref64| + slack     (2^-8: half a bf16 ulp, relative)
  output stored as fp32:  |out - ref64| <= slack
  slack = margin * max|twin32 - ref64| over the same tensor, twin32 = the fp32 PyTorch twin on the same
  inputs (measured against the oracle, never against the kernel); margin 8 unless docs/PARITY.md says why not.

The fp8 quantisers (``csrc/fp8.hip``, ``cvt4`` in ``csrc/common.h``) have no error rule: ``fp8_quantise`` gives the
bytes from the 256-entry code tables (``fp8_codes``), ``fp8_probes`` the inputs at which a conversion can go wrong;
``tests/test_fp8_quant_edges_gpu.py`` compares bytes.
"""
import math

import torch

BF16_HALF_ULP = 2.0 ** -8
MARGIN = 8.0


# ------------------------------------------------------------------------------------------ error rule
def excess_ratio(out, ref64, twin32, rel=None):
    """max over elements of (|out - ref64| - rel * |ref64|) / max|twin32 - ref64|: the margin this output
    needs (<= 0: inside the bf16 rounding term alone).  inf when the twin is exact and the output is not."""
    ref64 = ref64.double()
    if rel is None:
        rel = BF16_HALF_ULP if out.dtype == torch.bfloat16 else 0.0
    err = (out.double() - ref64).abs() - rel * ref64.abs()
    unit = (twin32.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    worst = err.max().item() if ref64.numel() else 0.0
    if worst != worst:
        return float("nan")
    if worst <= 0.0:
        return 0.0
    return worst / unit if unit > 0 else float("inf")


def check(out, ref64, twin32, margin=MARGIN, name="", rel=None, report=None, note=""):
    """Assert the error rule on EVERY element of ``out``; on failure name the worst element.  ``report``
    (a dict) collects the measured margin per name (max over calls) for the table in docs/PARITY.md."""
    assert out.shape == ref64.shape == twin32.shape, (name, out.shape, ref64.shape, twin32.shape)
    ref64 = ref64.double()
    if rel is None:
        rel = BF16_HALF_ULP if out.dtype == torch.bfloat16 else 0.0
    if ref64.numel() == 0:
        return
    unit = (twin32.double() - ref64).abs().max().item()
    slack = margin * unit
    err = (out.double() - ref64).abs()
    bound = rel * ref64.abs() + slack
    over = err - bound
    ratio = excess_ratio(out, ref64, twin32, rel)
    if report is not None:
        prev = report.get(name, 0.0)
        report[name] = ratio if (ratio != ratio or ratio > prev) else prev
    bad = ~(err <= bound)  # NaN counts as bad
    if bool(bad.any()):
        flat = torch.where(bad.reshape(-1), over.reshape(-1).nan_to_num(float("inf")),
                           torch.full_like(over.reshape(-1), float("-inf"))).argmax().item()
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref64.shape)) if ref64.dim() else ()
        raise AssertionError(
            f"{name}{' [' + note + ']' if note else ''}: {int(bad.sum())} of {ref64.numel()} elements outside the "
            f"rule; worst at {idx}: "
            f"out={out.reshape(-1)[flat].item()!r} ref64={ref64.reshape(-1)[flat].item()!r} "
            f"err={err.reshape(-1)[flat].item():.3e} bound={bound.reshape(-1)[flat].item():.3e} "
            f"twin32={twin32.reshape(-1)[flat].item()!r} "
            f"(slack {slack:.3e} = {margin} x twin32 error {unit:.3e}; needs margin {ratio:.3g})")


# ------------------------------------------------------------------------------------------ inputs
def spike_columns(cols):
    """Column order of the spikes: the last 8 columns, the first column of every 512-column chunk, then every
    other position -- so even a few rows hit the places where a dropped or mis-indexed chunk shows."""
    first = list(range(max(0, cols - 8), cols)) + [c for c in range(0, cols, 512)]
    seen, order = set(), []
    for c in first + list(range(cols)):
        if c not in seen:
            seen.add(c)
            order.append(c)
    return order


def spiked(rows, cols, device, scale=1.0, start=0):
    """randn * scale with one +-8*scale spike per row at a column that walks through ``spike_columns``."""
    x = torch.randn(rows, cols, device=device) * scale
    order = torch.tensor(spike_columns(cols), device=device)
    r = torch.arange(rows, device=device)
    col = order[(r + start) % order.numel()]
    sign = 1.0 - 2.0 * ((r // 2) % 2).to(x.dtype)
    x[r, col] = 8.0 * scale * sign
    return x


# ------------------------------------------------------------------------------------------ RMSNorm
def f32_scalar(v):
    """The value a C ``float`` argument takes."""
    return float(torch.tensor(v, dtype=torch.float32))


def rmsnorm(h, w, eps, a=None, round_hnew=False, dy=None, dres=None):
    """h_new = h (+ a); rstd = 1/sqrt(mean(h_new^2) + eps); y = w * h_new * rstd.
    ``round_hnew``: h_new is rounded to bf16 (after the fp32 sum, as stored) before the statistics.
    With ``dy``: g = dy * w, dx = rstd * (g - xhat * mean(g * xhat)) + dres, da = dx, dw = sum_rows dy * xhat.
    Returns a dict of float64 tensors y, h_new, rstd and (with dy) dx, da, dw."""
    hn = h.double()
    if a is not None:
        hn = hn + a.double()
    if round_hnew:
        hn = hn.float().bfloat16().double()
    rstd = 1.0 / torch.sqrt((hn * hn).mean(-1, keepdim=True) + f32_scalar(eps))
    xhat = hn * rstd
    out = {"y": w.double() * xhat, "h_new": hn, "rstd": rstd[..., 0]}
    if dy is not None:
        d = dy.double()
        g = d * w.double()
        dx = rstd * (g - xhat * (g * xhat).mean(-1, keepdim=True))
        if dres is not None:
            dx = dx + dres.double()
        out.update(dx=dx, da=dx, dw=(d * xhat).reshape(-1, hn.shape[-1]).sum(0))
    return out


def colsum_add(part, out):
    return out.double() + part.double().sum(0)


# ------------------------------------------------------------------------------------------ RoPE
def rope(qkv, cos, sin, B, T, nh, nkv, hd, inverse=False):
    """Half-split rotation of the q and k heads of packed rows [B*T, (nh + 2 nkv) * hd]; element i pairs with
    i + hd/2; the fp32 tables [T, hd] are taken as given (first half read) and widened; v passes through."""
    x = qkv.double()
    nrot, half = nh + nkv, hd // 2
    blk = x[:, :nrot * hd].reshape(B, T, nrot, hd)
    c = cos[:T, :half].double()[None, :, None, :]
    s = sin[:T, :half].double()[None, :, None, :]
    if inverse:
        s = -s
    x1, x2 = blk[..., :half], blk[..., half:]
    rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).reshape(B * T, nrot * hd)
    return torch.cat([rot, x[:, nrot * hd:]], dim=1)


# ------------------------------------------------------------------------------------------ attention
LOG2E = 1.4426950408889634


def attention_mask(B, T, device, kstart=None, doc_start=None):
    """Boolean [B, 1, T, T], True = query row attends to key column: key <= query, and key >= kstart[b] (left
    padding) or key >= doc_start[b, query] (packed documents)."""
    t = torch.arange(T, device=device)
    ok = (t[None, :] <= t[:, None]).expand(B, T, T).clone()
    if kstart is not None:
        ok &= t.view(1, 1, T) >= kstart.to(device).long().view(B, 1, 1)
    if doc_start is not None:
        ok &= t.view(1, 1, T) >= doc_start.to(device).long().view(B, T, 1)
    return ok.unsqueeze(1)


def _attention(qkv, B, T, nh, nkv, hd, scale, kstart, doc_start, dO, rope_out, cos, sin, o_saved, rnd):
    assert kstart is None or doc_start is None
    x = qkv.double().view(B, T, (nh + 2 * nkv) * hd)
    rep = nh // nkv
    q = x[..., :nh * hd].reshape(B, T, nh, hd).transpose(1, 2)
    k = x[..., nh * hd:(nh + nkv) * hd].reshape(B, T, nkv, hd).transpose(1, 2).repeat_interleave(rep, dim=1)
    v = x[..., (nh + nkv) * hd:].reshape(B, T, nkv, hd).transpose(1, 2).repeat_interleave(rep, dim=1)
    ok = attention_mask(B, T, qkv.device, kstart, doc_start)
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~ok, float("-inf"))
    m = s.amax(-1, keepdim=True)
    seen = torch.isfinite(m)  # rows with at least one key
    p = torch.exp(s - torch.where(seen, m, torch.zeros_like(m)))  # unnormalised, masked keys exactly 0
    l = p.sum(-1, keepdim=True)
    l1 = torch.where(seen, l, torch.ones_like(l))
    o = (rnd(p) @ v) / l1  # fully masked rows: 0
    lse2 = ((m + torch.log(l)) * LOG2E)[..., 0]  # fully masked rows: -inf + log(0) = -inf

    def rows(t4):  # [B, H, T, hd] -> [B*T, H*hd]
        return t4.transpose(1, 2).reshape(B * T, -1)

    out = {"o": rows(o), "lse2": lse2, "mask": ok, "seen": seen[:, 0, :, 0].expand(B, T)}
    if dO is None:
        return out
    d = dO.double().view(B, T, nh, hd).transpose(1, 2)
    ob = (rows(o).bfloat16() if o_saved is None else o_saved).double().view(B, T, nh, hd).transpose(1, 2)
    delta = (d * ob).sum(-1)
    P = p / l1
    dv = rnd(P).transpose(-1, -2) @ d
    dS = rnd(P * (d @ v.transpose(-1, -2) - delta[..., None]))
    dq = scale * (dS @ k)
    dk = scale * (dS.transpose(-1, -2) @ q)
    dk = dk.view(B, nkv, rep, T, hd).sum(2)  # GQA: the group's query heads
    dv = dv.view(B, nkv, rep, T, hd).sum(2)
    dqkv = torch.cat([rows(dq), rows(dk), rows(dv)], dim=1)
    if rope_out:
        dqkv = rope(dqkv, cos, sin, B, T, nh, nkv, hd, inverse=True)
    out.update(delta=delta, dqkv=dqkv, dq=dqkv[:, :nh * hd], dk=dqkv[:, nh * hd:(nh + nkv) * hd],
               dv=dqkv[:, (nh + nkv) * hd:])
    return out


def attention(qkv, B, T, nh, nkv, hd, scale, kstart=None, doc_start=None, dO=None, rope_out=False, cos=None,
              sin=None, o_saved=None):
    """Causal attention on packed rows q|k|v [B*T, (nh + 2 nkv) * hd] AS THE KERNELS SEE THEM (q|k already rotated);
    query head h uses kv head h // (nh / nkv).  Query q attends to keys lo <= k <= q with lo = 0, ``kstart[b]``
    (int [B]) or ``doc_start[b, q]`` (int [B, T]).  s = scale * q k^T, P = softmax(s), o = P v; a query with no key
    gives o = 0 and lse = -inf.  Returns float64: o [B*T, nh*hd], lse2 [B, nh, T] = logsumexp(s) * log2(e) (the
    stored unit), mask [B, 1, T, T], seen [B, T] (the query has a key), and with ``dO`` [B*T, nh*hd]:
      delta [B, nh, T] = rowsum(dO * o_bf16), o_bf16 = o rounded to bf16 as the forward saves it (``o_saved``: that
      tensor given instead, for a kernel whose input it is);
      dV = P^T dO, dP = dO V^T, dS = P * (dP - delta), dQ = scale dS K, dK = scale dS^T Q, dK / dV summed over the
      query heads of a group; dq [B*T, nh*hd], dk, dv [B*T, nkv*hd] and the packed dqkv.
    ``rope_out``: dq and dk go through the inverse rotation (``cos`` / ``sin``), as the store epilogues of
    rope_mode 2 do -- the gradient with respect to the un-rotated q|k."""
    return _attention(qkv, B, T, nh, nkv, hd, scale, kstart, doc_start, dO, rope_out, cos, sin, o_saved,
                      lambda t: t)


def attention_twin(qkv, B, T, nh, nkv, hd, scale, kstart=None, doc_start=None, dO=None, rope_out=False, cos=None,
                   sin=None, o_saved=None):
    """The error level of the kernels' number formats, nothing of their tiling or deferred max: the same float64
    math with the operand roundings the kernel header documents -- P (unnormalised in the forward, its row sum l
    taken from the unrounded P) rounded to bf16 before P V and before P^T dO, dS rounded to bf16 before dS K and
    dS^T Q.  ``lse2`` and ``delta`` (fp32 outputs) are instead the plain fp32 PyTorch twin on the same inputs."""
    out = _attention(qkv, B, T, nh, nkv, hd, scale, kstart, doc_start, dO, rope_out, cos, sin, o_saved,
                     lambda t: t.bfloat16().double())
    x = qkv.float().view(B, T, (nh + 2 * nkv) * hd)
    q = x[..., :nh * hd].reshape(B, T, nh, hd).transpose(1, 2)
    k = x[..., nh * hd:(nh + nkv) * hd].reshape(B, T, nkv, hd).transpose(1, 2).repeat_interleave(nh // nkv, dim=1)
    s = (q @ k.transpose(-1, -2)) * f32_scalar(scale)
    out["lse2"] = torch.logsumexp(s.masked_fill(~out["mask"], float("-inf")), dim=-1) * f32_scalar(LOG2E)
    if dO is not None:
        ob = attention(qkv, B, T, nh, nkv, hd, scale, kstart, doc_start)["o"].bfloat16() if o_saved is None else o_saved
        out["delta"] = (dO.float() * ob.float()).view(B, T, nh, hd).sum(-1).transpose(1, 2)
    return out


# ------------------------------------------------------------------------------------------ SwiGLU
def swiglu_fwd(gu):
    g, u = gu.double().chunk(2, dim=-1)
    return g * torch.sigmoid(g) * u


def swiglu_bwd(dy, gu):
    """dg = dy * u * s * (1 + g * (1 - s)), du = dy * g * s, s = sigmoid(g); returns d(gate|up)."""
    g, u = gu.double().chunk(2, dim=-1)
    d = dy.double()
    s = torch.sigmoid(g)
    return torch.cat([d * u * s * (1.0 + g * (1.0 - s)), d * g * s], dim=-1)


# ------------------------------------------------------------------------------------------ embedding
def _masked_ids(ids, V):
    ids = ids.reshape(-1)
    ok = (ids >= 0) & (ids < V)
    return torch.where(ok, ids, torch.zeros_like(ids)), ok  # never index with a bad id


def embedding_fwd(ids, W):
    safe, ok = _masked_ids(ids, W.shape[0])
    return W.double().index_select(0, safe) * ok[:, None].double()


def embedding_bwd(ids, dy, V, base=None):
    """gW[id] += dy[row] over the in-range ids (out-of-range rows contribute nothing)."""
    safe, ok = _masked_ids(ids, V)
    d = dy.double() * ok[:, None].double()
    gw = (base.double().clone() if base is not None
          else torch.zeros(V, dy.shape[1], dtype=torch.float64, device=dy.device))
    return gw.index_add_(0, safe, d)


# ------------------------------------------------------------------------------------------ cross-entropy
def ce_rows(logits, targets, scale, ignore_index=-100):
    """Per row: lse, loss = lse - x[target], dlogits = (softmax - onehot) * scale; ignored rows give 0 loss and
    0 gradient.  Returns (lse, row_loss, dlogits) in float64."""
    x = logits.double()
    lse = torch.logsumexp(x, dim=-1)
    ok = targets != ignore_index
    safe = torch.where(ok, targets, torch.zeros_like(targets))
    picked = x.gather(1, safe[:, None])[:, 0]
    loss = torch.where(ok, lse - picked, torch.zeros_like(lse))
    p = torch.exp(x - lse[:, None])
    p.scatter_add_(1, safe[:, None], -torch.ones_like(p[:, :1]))
    return lse, loss, p * (ok[:, None].double() * float(scale))


# ------------------------------------------------------------------------------------------ optimizer
def adamw(master, grad, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=1.0):
    """Clip by global norm (coef = min(1, max_norm / (norm + 1e-6))), decoupled decay, lerp first moment,
    second moment, bias-corrected step.  Returns (master, m, v, norm), all float64, inputs untouched."""
    b1, b2 = betas
    p, g, m, v = master.double(), grad.double(), m.double(), v.double()
    norm = g.norm()
    if max_norm is not None:
        g = g * torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    p = p * (1.0 - lr * weight_decay)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    p = p - (lr / (1.0 - b1 ** step)) * (m / denom)
    return p, m, v, norm


def pseudograd(sync, local):
    return sync.double() - local.double()


def outer_nesterov(master, sync, delta_sum, mom, inv_world, lr, momentum, first, drift_base=None):
    """d = delta_sum * inv_world; mom = d (first) or momentum * mom + d; new = sync - lr * (d + momentum * mom);
    master = new, or with drift_base: new + (master - (sync - drift_base)); sync = new.
    Returns (master, sync, mom) in float64."""
    d = delta_sum.double() * inv_world
    mom = d.clone() if first else mom.double() * momentum + d
    new = sync.double() - lr * (d + momentum * mom)
    if drift_base is not None:
        master = master.double() + drift_base.double() - sync.double() + new
    else:
        master = new.clone()
    return master, new, mom


# ------------------------------------------------------------------------------------------ transpose
def transpose(x):
    return x.double().t()


# ------------------------------------------------------------------------------------------ fp8 quantisers
FP8_FMAX = {0: 448.0, 1: 57344.0}  # fmt 0: e4m3fn, 1: e5m2 (ops/fp8.py E4M3 / E5M2)
_FP8_LAYOUT = {0: (4, 3, 7), 1: (5, 2, 15)}  # exponent bits, mantissa bits, bias
_FP8_NAN_BYTE = 0x7F  # a NaN code in both formats (e4m3fn: S.1111.111; e5m2: S.11111.11)


def fp8_codes(fmt):
    """The 256 decoded values of OCP e4m3fn (fmt 0) / e5m2 (fmt 1) as float64, indexed by the byte.
    e4m3fn: no infinities, only S.1111.111 is NaN (largest finite 448); e5m2: IEEE-like, exponent 31 is inf / NaN."""
    eb, mb, bias = _FP8_LAYOUT[fmt]
    vals = []
    for byte in range(256):
        sign = -1.0 if byte & 0x80 else 1.0
        e, m = (byte >> mb) & ((1 << eb) - 1), byte & ((1 << mb) - 1)
        if fmt == 0 and e == 15 and m == 7:
            v = float("nan")
        elif fmt == 1 and e == 31:
            v = float("inf") if m == 0 else float("nan")
        elif e == 0:
            v = m * 2.0 ** (1 - bias - mb)
        else:
            v = (1.0 + m * 2.0 ** -mb) * 2.0 ** (e - bias)
        vals.append(sign * v)
    return torch.tensor(vals, dtype=torch.float64)


def _fp8_finite(fmt):
    """The finite non-negative code values in byte order (byte b decodes to element b; strictly increasing)."""
    c = fp8_codes(fmt)[:128]
    return c[torch.isfinite(c)]


def fp8_quantise(x, scale, fmt):
    """The bytes (uint8) of ``fp8(clamp(x * scale, -FMAX, FMAX))`` as csrc/fp8.hip states it: the product is ONE
    fp32 multiply of the widened input (bf16 widens exactly) by the fp32 scale -- taken here as the exact float64
    product of the two rounded once to fp32, subnormal results kept; the clamped value goes to the nearest finite
    code of its own sign, ties to the code with an even low bit, -0 to 0x80; NaN gives a NaN code (compare with
    ``fp8_is_nan``, not by byte); +-inf saturates to +-FMAX.  No float8 dtype and no kernel is involved."""
    s = float(torch.as_tensor(scale).float().reshape(-1)[0])  # the fp32 scale (a number or a one-element tensor)
    p = (x.double() * s).float().double()  # 24 x 24 significant bits: exact in float64, then one rounding
    finite = _fp8_finite(fmt).to(x.device)
    mids = (finite[:-1] + finite[1:]) / 2  # exact: a code has at most 4 significant bits
    a = p.abs().clamp(max=FP8_FMAX[fmt])  # NaN stays NaN
    nan = torch.isnan(a)
    a = torch.where(nan, torch.zeros_like(a), a)
    lo = torch.searchsorted(mids, a.reshape(-1).contiguous()).reshape(a.shape)  # number of midpoints below a
    tie = mids[lo.clamp(max=mids.numel() - 1)] == a
    code = torch.where(tie & (lo % 2 == 1), lo + 1, lo)
    code = code | (torch.signbit(p).long() << 7)
    code = torch.where(nan, torch.full_like(code, _FP8_NAN_BYTE), code)
    return code.to(torch.uint8)


def fp8_is_nan(q, fmt):
    """Which bytes of ``q`` (uint8 or a float8 tensor) decode to NaN."""
    return torch.isnan(fp8_codes(fmt).to(q.device)[q.view(torch.uint8).long()])


def fp8_same(q, ref, fmt):
    """Byte equality, with every NaN code equal to every other NaN code."""
    q, ref = q.view(torch.uint8), ref.view(torch.uint8)
    return (q == ref) | (fp8_is_nan(q, fmt) & fp8_is_nan(ref, fmt))


def _ulp_step(v, up):
    """Positive finite ``v`` (fp32 or bf16) moved one ulp of its dtype up or down."""
    it = torch.int32 if v.dtype == torch.float32 else torch.int16
    return (v.view(it) + (1 if up else -1)).view(v.dtype)


def fp8_probes(fmt, dtype):
    """The inputs at which a quantiser can round wrongly, as a 1-D CPU tensor of ``dtype`` (fp32 or bf16): every
    finite non-negative code value; every midpoint of adjacent codes (the first is half the smallest subnormal);
    each midpoint moved one ulp of ``dtype`` either way; FMAX moved up one ulp, 1e30 and inf; all of these negated;
    +-0.  Code values and midpoints have at most 5 significant bits and exponents bf16 holds: exact in both dtypes.
    NaN is kept apart (``float('nan')`` is added by the tests that want it)."""
    finite = _fp8_finite(fmt)
    mids = ((finite[:-1] + finite[1:]) / 2).to(dtype)
    assert bool((mids.double() * 2 == finite[:-1] + finite[1:]).all())
    fmax = torch.tensor([FP8_FMAX[fmt]], dtype=dtype)
    pos = torch.cat([finite.to(dtype), mids, _ulp_step(mids, False), _ulp_step(mids, True), _ulp_step(fmax, True),
                     torch.tensor([1e30, float("inf")], dtype=dtype)])
    return torch.cat([pos, -pos, torch.tensor([0.0, -0.0], dtype=dtype)])
