"""Checks of the three quantised-transport ops against the in-test oracle (tests/_qoracle.py), written once
and run on CPU (tests/test_qcomm_cpu.py: the PyTorch path) and on the GPU (tests/test_qcomm_gpu.py: the HIP
kernels).  Wire buffers are sentinel-filled with guard bytes around them; fp32 buffers carry guard elements."""
import torch

from nanodiloco_amd import ops

from . import _qoracle as qo

GUARD = 64          # guard bytes / elements on both sides of every output
SENT = 0xA5


def guarded_bytes(n, dev):
    full = torch.full((n + 2 * GUARD,), SENT, dtype=torch.uint8, device=dev)
    return full, full[GUARD:GUARD + n]


def guards_intact(full):
    f = full.cpu()
    return bool((f[:GUARD] == SENT).all() and (f[-GUARD:] == SENT).all())


def guarded_f32(x, dev, fill=768.0):
    """x placed in the middle of a guard-padded fp32 buffer (the view keeps 16-byte alignment: GUARD = 64)."""
    full = torch.full((x.numel() + 2 * GUARD,), fill, dtype=x.dtype, device=dev)
    full[GUARD:GUARD + x.numel()] = x.to(dev)
    return full, full[GUARD:GUARD + x.numel()]


def f32_guards_intact(full, fill=768.0):
    f = full.float().cpu()
    return bool((f[:GUARD] == fill).all() and (f[-GUARD:] == fill).all())


def run_pseudograd_q(d, w, bits, dev, master=None):
    """Quantise the span sync - master into w chunks -> (codes [w, c], scales [w, c/256], c, the wire buffer);
    checks the guards around both buffers.  ``master`` None: sync = d and master = 0, so the difference is d
    exactly; otherwise sync = d + master, and the caller chooses values for which that sum is exact."""
    n = d.numel()
    c = qo.chunk(n, w)
    if master is None:
        master = torch.zeros(n)
    sync_full, sync = guarded_f32(d + master, dev)
    master = master.to(dev)
    full, out = guarded_bytes(w * qo.chunk_bytes(c, bits), dev)
    ops.pseudograd_q(sync, master, out, w, c, bits)
    assert guards_intact(full), "pseudograd_q wrote outside its wire buffer"
    assert f32_guards_intact(sync_full)
    codes, scales = qo.unpack(out, w, c, bits)
    return codes, scales, c, out


def check_exact_quantiser(n, w, bits, dev):
    """Exact-by-construction inputs: codes == k and scales == 2^-10, bitwise; zero in the padding."""
    vals, k = qo.exact_span(n, bits, seed=n + w)
    codes, scales, c, out = run_pseudograd_q(vals, w, bits, dev)
    want_k = torch.zeros(w * c, dtype=torch.int8)
    want_k[:n] = k
    nb_real = -(-n // qo.QB)
    want_s = torch.zeros(w * c // qo.QB)
    want_s[:nb_real] = 2.0 ** -10
    assert torch.equal(codes.view(-1), want_k)
    assert torch.equal(scales.view(-1), want_s)
    # and the whole wire image equals the oracle's packing of the oracle's quantisation
    oc, os_ = qo.quant_span(vals, w, bits)
    assert torch.equal(out.cpu(), qo.pack(oc, os_, bits))
    # a non-zero master: master = m * 2^-10, sync = (m + k) * 2^-10 with integers m, so sync - master == vals
    # exactly -- a kernel that ignored master, or added it, gives other codes
    m = torch.randint(-500, 501, (n,), generator=torch.Generator().manual_seed(n)).float() * 2.0 ** -10
    m[m == 0] = 3 * 2.0 ** -10
    assert torch.equal((vals + m) - m, vals)
    codes2, scales2, _, out2 = run_pseudograd_q(vals, w, bits, dev, master=m)
    assert torch.equal(codes2.view(-1), want_k) and torch.equal(scales2.view(-1), want_s)
    assert torch.equal(out2, out)


def check_random_quantiser(n, w, bits, dev):
    """|code*scale - x| <= scale/2 (1 + 2^-20); scale == amax/QMAX within 1 ulp; padding blocks are zero."""
    g = torch.Generator().manual_seed(1000 + n + w + bits)
    x = torch.randn(n, generator=g) * 1e-3
    codes, scales, c, _ = run_pseudograd_q(x, w, bits, dev)
    xp = torch.zeros(w * c)
    xp[:n] = x
    sc = scales.view(-1)
    dq = qo.dequant(codes.view(-1, qo.QB), sc[:, None]).view(-1)
    per = sc.repeat_interleave(qo.QB)
    err = (dq - xp).abs()
    print(f"n={n} W={w} int{bits}: max |err|/scale = {(err / per.clamp_min(1e-30)).max().item():.5f}")
    # every step of the quantiser is one correctly rounded fp32 operation, so codes and scales equal the oracle's
    oc, os_ = qo.quant_span(x, w, bits)
    assert torch.equal(codes, oc) and torch.equal(scales, os_)
    if n < 100_000:
        assert bool((err <= per / 2 * (1 + 2.0 ** -20)).all())
    else:
        # At millions of elements the 2^-20 slack is not a property of fp32 arithmetic: x * inv carries two
        # roundings, so a value within QMAX * 2^-23 codes of a tie may round the other way.  The ORACLE itself
        # gives max |err| / scale = 0.5000020 (n = 2097308) and 0.5000013 (n = 2097408) for int8 with these
        # seeds.  The grid-wrap size is held to the oracle bitwise (above) and to that arithmetic bound here.
        assert bool((err <= per / 2 * (1 + 4 * qo.qmax(bits) * 2.0 ** -23)).all())
    amax = xp.view(-1, qo.QB).abs().amax(dim=1)
    want = amax / qo.qmax(bits)
    lo, hi = torch.nextafter(want, torch.full_like(want, -1.0)), torch.nextafter(want, torch.full_like(want, 1.0))
    assert bool(((sc >= lo) & (sc <= hi)).all())
    assert bool((codes.view(-1).abs() <= int(qo.qmax(bits))).all())
    zero = amax == 0
    assert bool((sc[zero] == 0).all()) and bool((codes.view(-1, qo.QB)[zero] == 0).all())


def check_special_blocks(bits, dev):
    """zero block -> zero codes and zero scale; a block with an inf or a NaN -> NaN scale; int4 nibble order"""
    q = qo.qmax(bits)
    x = torch.zeros(4 * qo.QB)
    x[qo.QB:2 * qo.QB] = torch.linspace(-1, 1, qo.QB)
    x[qo.QB + 5] = float("inf")
    x[2 * qo.QB + 7] = float("nan")
    x[3 * qo.QB] = 1.0       # code QMAX
    x[3 * qo.QB + 1] = -1.0  # code -QMAX
    x[3 * qo.QB + 2] = 3.0 / q  # code 3
    codes, scales, c, out = run_pseudograd_q(x, 1, bits, dev)
    s = scales.view(-1)
    assert s[0] == 0 and bool((codes.view(-1)[:qo.QB] == 0).all())
    assert torch.isnan(s[1]) and torch.isnan(s[2])
    assert s[3] == 1.0 / q
    assert codes.view(-1)[3 * qo.QB:3 * qo.QB + 3].tolist() == [int(q), -int(q), 3]
    if bits == 4:
        raw = out.cpu()
        base = 3 * qo.QB // 2
        assert int(raw[base]) == (7 | ((-7 & 0xF) << 4)) and int(raw[base + 1]) == 3  # element 2i: low nibble
    # the NaN scale poisons the update, as a NaN pseudo-gradient does on the fp32 path
    n = x.numel()
    master, sync, mom = torch.ones(n, device=dev), torch.ones(n, device=dev), torch.zeros(n, device=dev)
    ops.outer_nesterov_q(master, sync, out, 1, c, bits, mom, None, 1.0, 0.7, 0.9, True)
    m = master.cpu()
    assert bool(torch.isnan(m[qo.QB:3 * qo.QB]).all()) and bool(torch.isfinite(m[:qo.QB]).all())


def check_tiny_block(bits, dev):
    """A block whose amax is so small that QMAX / amax overflows: inv is kept finite, so the zero elements
    still quantise to code 0 (0 * inf would be NaN and end up as -QMAX) and nothing is NaN."""
    x = torch.zeros(2 * qo.QB)
    x[3] = 2.0 ** -125
    x[9] = -(2.0 ** -125)
    x[qo.QB:] = torch.linspace(-1, 1, qo.QB)
    codes, scales, c, out = run_pseudograd_q(x, 1, bits, dev)
    k = codes.view(-1)[:qo.QB]
    assert k[3] > 0 and k[9] == -k[3]
    k[3] = k[9] = 0
    assert bool((k == 0).all())
    assert not bool(torch.isnan(scales).any())
    oc, os_ = qo.quant_span(x, 1, bits)  # the ordinary block beside it is untouched by the clamp
    assert torch.equal(codes.view(-1)[qo.QB:], oc.view(-1)[qo.QB:]) and scales.view(-1)[1] == os_.view(-1)[1]


def make_chunks(w, c, bits, exact, seed):
    """w wire chunks of c elements as every worker's quantised contribution to ONE owned chunk."""
    codes, scales = [], []
    for r in range(w):
        if exact:
            v, _ = qo.exact_span(c, bits, seed=seed + r)
        else:
            v = torch.randn(c, generator=torch.Generator().manual_seed(seed + r)) * 1e-3
        cq, sq = qo.quant(v.view(-1, qo.QB), bits)
        codes.append(cq.view(-1))
        scales.append(sq)
    return torch.stack(codes), torch.stack(scales)


def check_qreduce(c, w, bits, dev, exact):
    codes, scales = make_chunks(w, c, bits, exact, seed=31 * w + c)
    inp = qo.pack(codes, scales, bits).to(dev)
    full, out = guarded_bytes(qo.chunk_bytes(c, bits), dev)
    before = inp.clone()
    ops.qreduce(inp, w, c, bits, out)
    assert guards_intact(full), "qreduce wrote outside its output chunk"
    assert torch.equal(inp, before)
    got_c, got_s = qo.unpack(out, 1, c, bits)
    want_c, want_s = qo.reduce_chunks(codes, scales, bits)
    # bitwise on exact inputs (every partial sum is a small integer times 2^-10) and on random ones too: the
    # kernel rounds product and sum separately, in rank order, like the oracle -- every operation is one
    # correctly rounded IEEE operation on both sides
    assert torch.equal(got_c, want_c) and torch.equal(got_s, want_s)
    # the format's bound: the requantised sum is within scale2/2 of the fp32 sum of the dequantised inputs
    acc = torch.zeros(c)
    for r in range(w):
        acc = acc + qo.dequant(codes[r], scales[r])
    per = got_s.view(-1).repeat_interleave(qo.QB)
    err = (qo.dequant(got_c, got_s).view(-1) - acc).abs()
    assert bool((err <= per / 2 * (1 + 2.0 ** -20)).all())
    amax = acc.view(-1, qo.QB).abs().amax(dim=1) / qo.qmax(bits)
    lo, hi = torch.nextafter(amax, torch.full_like(amax, -1.0)), torch.nextafter(amax, torch.full_like(amax, 1.0))
    assert bool(((got_s.view(-1) >= lo) & (got_s.view(-1) <= hi)).all())


def check_outer_q(n, w, bits, dev, first, shadow, exact=True):
    """nd_outer_nesterov_q == the fp32 outer update fed with codes.float() * scale, bitwise: master, sync,
    momentum and the bf16 shadow; nothing outside [0, n) is touched."""
    if exact:
        vals, _ = qo.exact_span(n, bits, seed=7 * n + w)
    else:
        vals = torch.randn(n, generator=torch.Generator().manual_seed(5 * n + w)) * 1e-3
    codes, scales = qo.quant_span(vals, w, bits)
    c = codes.shape[1]
    wire = qo.pack(codes, scales, bits).to(dev)
    dsum = qo.dequant(codes, scales).view(-1)[:n].contiguous().to(dev)
    g = torch.Generator().manual_seed(n + 3)
    m0, s0, b0 = (torch.randn(n, generator=g) for _ in range(3))

    def state():
        out = [guarded_f32(t, dev) for t in (m0, s0, b0)]
        out.append(guarded_f32(torch.zeros(n, dtype=torch.bfloat16), dev) if shadow else (None, None))
        return out

    (mf, m), (sf, s), (bf, b), (hf, h) = state()
    (mf2, m2), (sf2, s2), (bf2, b2), (hf2, h2) = state()
    inv_w, lr, mu = 1.0 / w, 0.7, 0.9
    ops.outer_nesterov_q(m, s, wire, w, c, bits, b, h, inv_w, lr, mu, first)
    if dev == "cpu":  # PyTorch path: torch.optim.SGD(nesterov=True) on theta_sync is the reference
        p = torch.nn.Parameter(s2.clone())
        sgd = torch.optim.SGD([p], lr=lr, momentum=mu, nesterov=True)
        if not first:
            sgd.state[p]["momentum_buffer"] = b2.clone()
        p.grad = dsum * inv_w
        sgd.step()
        b2.copy_(sgd.state[p]["momentum_buffer"])
        for t in (m2, s2) + ((h2,) if shadow else ()):
            t.copy_(p.detach())
    else:  # HIP: the fp32-transport kernel fed with the dequantised sum
        ops.outer_nesterov(m2, s2, dsum, b2, h2, inv_w, lr, mu, first)
    for got, want in ((mf, mf2), (sf, sf2), (bf, bf2)):
        assert torch.equal(got, want)       # guards included: both leave them alone
        assert f32_guards_intact(got)
    assert not torch.equal(m, m0.to(dev))
    if shadow:
        assert torch.equal(hf, hf2) and f32_guards_intact(hf)
        assert torch.equal(h, m.to(torch.bfloat16))
