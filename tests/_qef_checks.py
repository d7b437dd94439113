"""Checks of the two error-feedback ops of the quantised transport (``ops.pseudograd_q_ef``, ``ops.qreduce_ef``)
against an in-test oracle, written once and run on CPU (tests/test_qef_cpu.py: the PyTorch path) and on the GPU
(tests/test_qef_gpu.py: the HIP kernels).  The oracle is ``_qoracle.quant`` plus the two residual formulas of
docs/DESIGN.md "Error feedback" in plain fp32 torch ops (every operation rounds on its own); it uses nothing from
``nanodiloco_amd.ops.qcomm``.  Buffers are guarded as in tests/_qcomm_checks.py, the residual included."""
import torch

from nanodiloco_amd import ops

from . import _qoracle as qo
from ._qcomm_checks import f32_guards_intact, guarded_bytes, guarded_f32, guards_intact, make_chunks

QB = qo.QB


# ------------------------------------------------------------------------------------------------ oracle
def oracle_stage1(sync, master, e, w, bits):
    """x = fl(fl(sync - master) + e), quantised as w chunks -> (codes [w, c], scales [w, c/256], new e [n])."""
    n = sync.numel()
    c = qo.chunk(n, w)
    x = torch.zeros(w * c)
    x[:n] = (sync - master) + e
    xb = x.view(-1, QB)
    codes, scale = qo.quant(xb, bits)
    r = xb - codes.float() * scale[:, None]
    return codes.view(w, c), scale.view(w, c // QB), r.view(-1)[:n].clone()


def oracle_stage2(codes, scales, e, bits):
    """acc = sum_r fl(code_r * scale_r) in rank order from 0.0, x = fl(acc + e) -> (codes [1, c], scales
    [1, c/256], new e [c])."""
    acc = torch.zeros(codes.shape[1])
    for r in range(codes.shape[0]):
        acc = acc + qo.dequant(codes[r], scales[r])
    xb = (acc + e).view(-1, QB)
    q, s = qo.quant(xb, bits)
    r = xb - q.float() * s[:, None]
    return q.view(1, -1), s.view(1, -1), r.view(-1)


def same_bits(a, b):
    """bitwise equality of two fp32 tensors (NaN == NaN, +0 != -0)"""
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ runners
def run_stage1(sync, master, e, w, bits, dev):
    """ops.pseudograd_q_ef on guarded buffers -> (wire bytes on the CPU, new residual on the CPU)."""
    n = sync.numel()
    c = qo.chunk(n, w)
    sf, s = guarded_f32(sync, dev)
    mf, m = guarded_f32(master, dev)
    ef, ev = guarded_f32(e, dev)
    full, out = guarded_bytes(w * qo.chunk_bytes(c, bits), dev)
    ops.pseudograd_q_ef(s, m, ev, out, w, c, bits)
    assert guards_intact(full), "pseudograd_q_ef wrote outside its wire buffer"
    assert f32_guards_intact(ef), "pseudograd_q_ef wrote a residual outside [0, n)"
    assert f32_guards_intact(sf) and f32_guards_intact(mf)
    assert same_bits(s, sync) and same_bits(m, master)
    return out.cpu().clone(), ev.cpu().clone()


def run_stateless1(sync, master, w, bits, dev):
    c = qo.chunk(sync.numel(), w)
    out = torch.zeros(w * qo.chunk_bytes(c, bits), dtype=torch.uint8, device=dev)
    ops.pseudograd_q(sync.to(dev), master.to(dev), out, w, c, bits)
    return out.cpu()


def run_stage2(inp, nw, c, bits, e, dev):
    """ops.qreduce_ef on guarded buffers -> (wire chunk on the CPU, new residual on the CPU)."""
    inp = inp.to(dev)
    before = inp.clone()
    ef, ev = guarded_f32(e, dev)
    full, out = guarded_bytes(qo.chunk_bytes(c, bits), dev)
    ops.qreduce_ef(inp, nw, c, bits, ev, out)
    assert guards_intact(full), "qreduce_ef wrote outside its output chunk"
    assert f32_guards_intact(ef), "qreduce_ef wrote a residual outside its chunk"
    assert torch.equal(inp, before)
    return out.cpu().clone(), ev.cpu().clone()


def _span(n, seed, sigma=1e-3):
    """sync, master with sync - master ~ N(0, sigma) (the difference itself is whatever fp32 makes of it)"""
    g = torch.Generator().manual_seed(seed)
    master = torch.randn(n, generator=g) * 0.05
    sync = master + torch.randn(n, generator=g) * sigma
    return sync, master


def _half_step_residual(n, bits, seed, sigma=1e-3):
    """a residual of about half a quantisation step of a block of N(0, sigma) values (amax ~ 3 sigma)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) - 0.5) * (3 * sigma / qo.qmax(bits))


def _half_step(per, n, bits):
    """|x - code * scale| <= scale / 2 up to the two roundings of x * inv (tests/_qcomm_checks.py,
    check_random_quantiser: 2^-20 holds at small sizes, the arithmetic bound at millions of elements)"""
    return per / 2 * (1 + (2.0 ** -20 if n < 100_000 else 4 * qo.qmax(bits) * 2.0 ** -23))


# ------------------------------------------------------------------------------------------------ 1. anchor
def check_zero_anchor_stage1(n, w, bits, dev):
    sync, master = _span(n, 11 * n + w + bits)
    wire, e = run_stage1(sync, master, torch.zeros(n), w, bits, dev)
    assert torch.equal(wire, run_stateless1(sync, master, w, bits, dev)), "zero residual: wire differs from pseudograd_q"
    oc, os_, oe = oracle_stage1(sync, master, torch.zeros(n), w, bits)
    assert torch.equal(wire, qo.pack(oc, os_, bits))
    assert same_bits(e, oe)
    assert bool((e != 0).any())


def check_zero_anchor_stage2(c, w, bits, dev):
    codes, scales = make_chunks(w, c, bits, False, seed=17 * w + c + bits)
    inp = qo.pack(codes, scales, bits)
    wire, e = run_stage2(inp, w, c, bits, torch.zeros(c), dev)
    ref = torch.zeros(qo.chunk_bytes(c, bits), dtype=torch.uint8, device=dev)
    ops.qreduce(inp.to(dev), w, c, bits, ref)
    assert torch.equal(wire, ref.cpu()), "zero residual: wire differs from qreduce"
    oc, os_, oe = oracle_stage2(codes, scales, torch.zeros(c), bits)
    assert torch.equal(wire, qo.pack(oc, os_, bits))
    assert same_bits(e, oe)
    assert w == 1 or bool((e != 0).any())  # one rank: requantising its own codes is exact


# ------------------------------------------------------------------------------------------------ 2. non-zero
def check_nonzero_stage1(n, w, bits, dev):
    sync, master = _span(n, 13 * n + w + bits)
    e0 = _half_step_residual(n, bits, n + 5)
    wire, e = run_stage1(sync, master, e0, w, bits, dev)
    oc, os_, oe = oracle_stage1(sync, master, e0, w, bits)
    assert torch.equal(wire, qo.pack(oc, os_, bits))
    assert same_bits(e, oe)
    # the residual mattered: without it other codes go out
    assert not torch.equal(wire, run_stateless1(sync, master, w, bits, dev))
    # and it is what was not delivered, at most half a step (the format's bound, as in check_random_quantiser)
    per = os_.view(-1).repeat_interleave(QB)[:n]
    assert bool((e.abs() <= _half_step(per, n, bits)).all())


def check_nonzero_stage2(c, w, bits, dev):
    codes, scales = make_chunks(w, c, bits, False, seed=19 * w + c + bits)
    e0 = _half_step_residual(c, bits, c + w, sigma=1e-3 * w ** 0.5)
    wire, e = run_stage2(qo.pack(codes, scales, bits), w, c, bits, e0, dev)
    oc, os_, oe = oracle_stage2(codes, scales, e0, bits)  # ranks first, then the residual
    assert torch.equal(wire, qo.pack(oc, os_, bits))
    assert same_bits(e, oe)
    per = os_.view(-1).repeat_interleave(QB)
    assert bool((e.abs() <= _half_step(per, c, bits)).all())


# ------------------------------------------------------------------------------------------------ 3. non-finite
def _check_blocks(wire, e, oc, os_, oe, nchunks, c, bits, bad, n):
    gc, gs = qo.unpack(wire, nchunks, c, bits)
    gc, gs, oc, os_ = gc.view(-1, QB), gs.view(-1), oc.reshape(-1, QB), os_.reshape(-1)
    for b in range(gc.shape[0]):
        lo, hi = b * QB, min((b + 1) * QB, n)
        if b in bad:
            assert torch.isnan(gs[b]) and bool((gc[b] == 0).all())
            assert bool(torch.isnan(e[lo:hi]).all()), f"block {b}: residual of a non-finite block must be NaN"
        else:
            assert torch.equal(gc[b], oc[b]) and same_bits(gs[b:b + 1], os_[b:b + 1])
            assert same_bits(e[lo:hi], oe[lo:hi]) and bool(torch.isfinite(e[lo:hi]).all())


def check_nonfinite_stage1(bits, dev):
    n = 4 * QB + 100
    sync, master = _span(n, 23 + bits)
    sync[QB + 5] = float("inf")
    sync[2 * QB + 7] = float("nan")
    e0 = _half_step_residual(n, bits, 3)
    wire, e = run_stage1(sync, master, e0, 1, bits, dev)
    oc, os_, oe = oracle_stage1(sync, master, e0, 1, bits)
    _check_blocks(wire, e, oc, os_, oe, 1, qo.chunk(n, 1), bits, {1, 2}, n)


def check_nonfinite_stage2(bits, dev):
    c, w = 5 * QB, 3
    codes, scales = make_chunks(w, c, bits, False, seed=29 + bits)
    scales[1, 1] = float("inf")   # code * inf: +-inf (NaN for a zero code)
    scales[2, 2] = float("nan")   # what a sender's non-finite block looks like on the wire
    codes[2, 2 * QB:3 * QB] = 0
    e0 = _half_step_residual(c, bits, 7, sigma=2e-3)
    wire, e = run_stage2(qo.pack(codes, scales, bits), w, c, bits, e0, dev)
    oc, os_, oe = oracle_stage2(codes, scales, e0, bits)
    _check_blocks(wire, e, oc, os_, oe, 1, c, bits, {1, 2}, c)


# ------------------------------------------------------------------------------------------------ 4. delivered sum
T_ROUNDS = 24


def delivered_sum(w, bits, dev, ef):
    """T rounds of a constant pseudo-gradient per worker through both stages (W quantisations, then the reduce).
    Returns, per element and in fp64, (|sum_t dq2_t - T sum_w d_w|, the bound sum_w s1_w/2 + s2/2 + slack, the
    last round's second scale) -- the bound is derived in docs/DESIGN.md "Error feedback": the left side equals
    |sum_w e1_w + e2| up to the fp32 roundings of the additions, and every residual is at most half its scale."""
    n = 6 * QB
    ds = []
    for k in range(w):
        d = torch.randn(n, generator=torch.Generator().manual_seed(40 + k)) * (1e-3 * (1 + k))
        d[::7] *= 0.02  # far below half a step: never sent by the stateless transport
        ds.append(d)
    pb = qo.chunk_bytes(n, bits)
    zero = torch.zeros(n, device=dev)
    syncs = [d.to(dev) for d in ds]  # master = 0: sync - master is d exactly
    e1 = [torch.zeros(n, device=dev) for _ in range(w)]
    e2 = torch.zeros(n, device=dev)
    recv = torch.zeros(w * pb, dtype=torch.uint8, device=dev)
    out = torch.zeros(pb, dtype=torch.uint8, device=dev)
    total = torch.zeros(n, dtype=torch.float64)
    for _ in range(T_ROUNDS):
        for k in range(w):
            if ef:
                ops.pseudograd_q_ef(syncs[k], zero, e1[k], recv[k * pb:(k + 1) * pb], 1, n, bits)
            else:
                ops.pseudograd_q(syncs[k], zero, recv[k * pb:(k + 1) * pb], 1, n, bits)
        if ef:
            ops.qreduce_ef(recv, w, n, bits, e2, out)
        else:
            ops.qreduce(recv, w, n, bits, out)
        c2, s2 = qo.unpack(out, 1, n, bits)
        total += qo.dequant(c2, s2).view(-1).double()
    _, s1 = qo.unpack(recv, w, n, bits)
    want = T_ROUNDS * torch.stack(ds).double().sum(dim=0)
    s1e = s1.double().repeat_interleave(QB, dim=1).sum(dim=0)
    s2e = s2.double().view(-1).repeat_interleave(QB)
    # every x that is added to a residual: |x_w| <= |d_w| + s1/2 and |x_2| <= sum_w |x_w| + s2/2 with steps of
    # at most amax / 7, so twice the sum of the workers' maxima bounds them all
    xmax = 2.0 * sum(d.abs().max().item() for d in ds)
    slack = T_ROUNDS * (w + 1) * 2.0 ** -23 * xmax
    return (total - want).abs(), s1e / 2 + s2e / 2 + slack, s2e


def check_delivered_sum(w, bits, dev):
    lhs, bound, s2 = delivered_sum(w, bits, dev, ef=True)
    print(f"W={w} int{bits} error feedback: max |delivered - sent| = {(lhs / s2).max().item():.3f} steps, "
          f"bound {(bound / s2).max().item():.3f}")
    assert bool((lhs <= bound).all()), (lhs - bound).max().item()
    # control: the same inputs through the stateless ops leave the bound far behind -- they can tell the two apart
    lhs0, bound0, s20 = delivered_sum(w, bits, dev, ef=False)
    print(f"W={w} int{bits} stateless: max |delivered - sent| = {(lhs0 / s20).max().item():.3f} steps")
    assert bool((lhs0 > bound0).any())
