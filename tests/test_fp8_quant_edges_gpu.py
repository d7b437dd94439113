"""The fp8 quantisers at their edges, against the code-table oracle of ``tests/_oracle64.py`` (T3, bytes and bits).

``csrc/fp8.hip`` (``nd_fp8_cast``, ``nd_fp8_cast_t``), ``cvt4`` / ``fp8_put8`` / ``put8_bf16_q`` / ``block_amax_commit``
(``csrc/common.h``) through the fused side outputs of RMSNorm, SwiGLU and the cross-entropy kernel, and the first-use /
weight paths of ``ops/fp8.py``.  Nothing here has a tolerance: every fp8 assertion is on bytes (NaN codes compared as
"decodes to NaN"), every amax assertion on float bits.  The reference is ``_oracle64.fp8_quantise`` -- a search in the
256-entry code table after one fp32 multiply, checked against torch on the CPU in ``test_oracle64_cpu.py`` -- never
``fp8.cast``, which the older tests use as their reference and which shares ``cvt4`` with everything it is compared to.

Inputs are ``_oracle64.fp8_probes``: every code, every tie between two codes, the ties moved one input ulp either way,
the subnormal range, half the smallest subnormal, +-0, FMAX and just past it, 1e30, +-inf -- plus NaN, which must come
out as a NaN byte (csrc/common.h ``clamp_keep_nan``).  Outputs sit in sentinel frames (``tests/_frames.py``).
"""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import _ext, fp8

from . import _oracle64 as o64
from ._frames import _PATTERN, assert_frame_intact, framed_flat

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
FMTS = [fp8.E4M3, fp8.E5M2]
FMT_ID = {fp8.E4M3: "e4m3", fp8.E5M2: "e5m2"}
DTS = [BF16, F32]
DT_ID = {BF16: "bf16", F32: "fp32"}
SCALES = [1.0, 2.0 ** -3, 2.0 ** 5, 37.5]
NAN = float("nan")
INVALID = 1  # hipErrorInvalidValue
GRID_ELEMS = 2048 * 256 * 8  # elements one trip of nd_fp8_cast's capped grid covers

fmt_p = pytest.mark.parametrize("fmt", FMTS, ids=[FMT_ID[f] for f in FMTS])
dt_p = pytest.mark.parametrize("dt", DTS, ids=[DT_ID[d] for d in DTS])


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    torch.manual_seed(0)
    yield
    ops.set_backend("auto")


def S():
    return _ext.stream_ptr(torch.device(DEV))


def lib_cast(x, n, scale, out, fmt, amax, parts):
    return _ext.lib().nd_fp8_cast(_ext.ptr(x), _ext.dtcode(x), n, _ext.ptr(scale), _ext.ptr(out), fmt,
                                  _ext.ptr(amax), parts, S())


def lib_cast_t(x, rows, cols, ld, scale, out, outT, fmt, amax, parts):
    return _ext.lib().nd_fp8_cast_t(_ext.ptr(x), _ext.dtcode(x), rows, cols, ld, _ext.ptr(scale), _ext.ptr(out),
                                    _ext.ptr(outT), fmt, _ext.ptr(amax), parts, S())


def q_frame(n, fmt, pad=16):
    """n fp8 bytes inside a sentinel frame; the view starts 16 bytes into the allocation (8- and 16-byte aligned)."""
    return framed_flat(n, fp8.TORCH_DT[fmt], pad=pad)


def amax_frame(parts, prior=0.0):
    big, v = framed_flat(parts, F32)
    v.copy_(prior if torch.is_tensor(prior) else torch.full((parts,), float(prior)))
    return big, v


def sc(v):
    return torch.tensor([v], dtype=F32, device=DEV)


def true_amax(x):
    """max |x| over the non-NaN elements (0.0 if there is none), as a Python float of the fp32 value."""
    a = x.detach().double().abs().reshape(-1)
    a = a[~torch.isnan(a)]
    return float(a.max()) if a.numel() else 0.0


def assert_bytes(q, ref, fmt, what=""):
    """``q`` (fp8 / uint8, any device) holds the oracle's bytes; NaN codes are equal to each other."""
    qb = q.reshape(-1).view(torch.uint8)
    rb = ref.reshape(-1).to(qb.device)
    assert qb.shape == rb.shape, (what, qb.shape, rb.shape)
    ok = o64.fp8_same(qb, rb, fmt)
    if not bool(ok.all()):
        bad = (~ok).nonzero().reshape(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {qb.numel()} bytes differ from the oracle; first at {i}: "
                             f"got 0x{int(qb[i]):02x} expected 0x{int(rb[i]):02x}; positions mod 8: "
                             f"{sorted(set((bad % 8).tolist()))}")


def oracle(x, scale, fmt):
    """Oracle bytes of x (computed on the CPU: its fp32 arithmetic keeps subnormals)."""
    return o64.fp8_quantise(x.detach().cpu(), scale, fmt)


def probe_input(fmt, dt, scale, nan=True):
    """The probes arranged so that ``x * scale`` lands on them (power-of-two scales: probe / scale, exact), NaNs last."""
    p = o64.fp8_probes(fmt, dt)
    x = p if scale == 37.5 else (p.double() / scale).to(dt)
    if nan:
        x = torch.cat([x, torch.tensor([NAN, -NAN], dtype=dt)])
    return x


def cycled(x, n):
    return x[torch.arange(n) % x.numel()]


# ------------------------------------------------------------------------------------------ rounding table
@pytest.mark.parametrize("scale", SCALES)
@dt_p
@fmt_p
def test_rounding_table_in_every_lane(fmt, dt, scale):
    """Every probe (and NaN) through each of the eight lanes of a vector, so through each of cvt4's four slots in
    both packed words, by rolling the vector 0..7 elements; n % 8 == 5, so five elements per roll take the tail."""
    base = probe_input(fmt, dt, scale)
    n = base.numel()
    while n % 8 != 5:
        n += 1
    x0 = cycled(base, n)
    ref0 = oracle(x0, scale, fmt)
    s = sc(scale)
    for r in range(8):
        x = torch.roll(x0, r).to(DEV)
        big, out = q_frame(n, fmt)
        abig, amax = amax_frame(fp8.AMAX_PARTS)
        assert lib_cast(x, n, s, out, fmt, amax, fp8.AMAX_PARTS) == 0
        torch.cuda.synchronize()
        assert_frame_intact(big, out)
        assert_frame_intact(abig, amax)
        assert_bytes(out, torch.roll(ref0, r), fmt, f"roll {r}")
        assert amax.max().item() == float("inf")  # +-inf is among the probes; NaN does not enter amax
    nan_at = torch.isnan(x0.float())
    assert int(nan_at.sum()) >= 2 and bool(o64.fp8_is_nan(ref0, fmt)[nan_at].all())


@dt_p
@fmt_p
def test_rounding_table_in_the_tail_loop(fmt, dt):
    """n = 7 launches (n8 == 0: the single block runs only the scalar tail loop) over every probe, seven at a time;
    each launch's eighth output byte is a sentinel that must survive."""
    base = probe_input(fmt, dt, 1.0)
    chunks = (base.numel() + 6) // 7
    x0 = cycled(base, chunks * 7)
    ref = oracle(x0, 1.0, fmt).view(chunks, 7)
    xin = torch.full((chunks, 8), 3.0, dtype=dt)
    xin[:, :7] = x0.view(chunks, 7)
    xin = xin.to(DEV)
    big, flat = q_frame(chunks * 8, fmt)
    out = flat.view(chunks, 8)
    abig, amax = amax_frame(4)
    s = sc(1.0)
    for i in range(chunks):
        assert lib_cast(xin[i], 7, s, out[i], fmt, amax, 4) == 0
    torch.cuda.synchronize()
    assert_frame_intact(big, flat)
    assert_bytes(out[:, :7].contiguous(), ref, fmt, "tail")
    assert bool((out.view(torch.uint8)[:, 7] == _PATTERN[1]).all()), "the byte after a 7-element output was written"
    assert amax.tolist() == [float("inf"), 0.0, 0.0, 0.0]  # one block: slot 0 only


# ------------------------------------------------------------------------------------------ lengths and grid
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 15, 2048 + 3, GRID_ELEMS + 8 * 3 + 5])
@dt_p
@fmt_p
def test_lengths(fmt, dt, n):
    """The scalar tail at every remainder class that matters, n < 8, and one wrap of the capped grid with three more
    vectors and a five-element tail; probes cycled over the length at scale 37.5, output framed."""
    x0 = cycled(probe_input(fmt, dt, 37.5), n) if n else torch.empty(0, dtype=dt)
    xbig, x = framed_flat(n, dt)
    x.copy_(x0)
    big, out = q_frame(n, fmt)
    abig, amax = amax_frame(7, 0.5)
    assert lib_cast(x, n, sc(37.5), out, fmt, amax, 7) == 0
    torch.cuda.synchronize()
    assert_frame_intact(big, out)
    assert_frame_intact(abig, amax)
    assert_frame_intact(xbig, x)
    if n == 0:  # success, nothing written
        assert_frame_intact(big)
        assert amax.tolist() == [0.5] * 7
        return
    assert_bytes(out, oracle(x0, 37.5, fmt), fmt, f"n={n}")
    assert amax.max().item() == max(0.5, true_amax(x0))
    blocks = min(2048, max(1, (n // 8 + 255) // 256))
    assert bool((amax[min(blocks, 7):] == 0.5).all())


@fmt_p
def test_fp32_subnormal_inputs_are_not_flushed(fmt):
    """fp32 subnormal inputs: the product is the plain fp32 multiply (2^-130 * 2^124 = 2^-6, a normal code) and an
    all-subnormal tensor's amax is its largest subnormal, bit for bit."""
    vals = [2.0 ** -130, -(2.0 ** -127), 3 * 2.0 ** -149, -(2.0 ** -149), 2.0 ** -126 - 2.0 ** -149, -(2.0 ** -133), 0.0]
    x0 = cycled(torch.tensor(vals, dtype=F32), 8 * 3 + 5)
    assert x0.abs().max().item() < 2.0 ** -126
    for scale in (2.0 ** 124, 1.0):
        x = x0.to(DEV)
        big, out = q_frame(x0.numel(), fmt)
        abig, amax = amax_frame(3)
        assert lib_cast(x, x0.numel(), sc(scale), out, fmt, amax, 3) == 0
        torch.cuda.synchronize()
        assert_frame_intact(big, out)
        ref = oracle(x0, scale, fmt)
        assert scale == 1.0 or int(((ref & 0x7F) != 0).sum()) >= 12  # most products are non-zero codes
        assert_bytes(out, ref, fmt, f"subnormal inputs, scale {scale}")
        assert amax.tolist() == [2.0 ** -126 - 2.0 ** -149, 0.0, 0.0]


# ------------------------------------------------------------------------------------------ amax contract
AMAX_N = {"five-blocks": 8 * 256 * 5 + 5, "wrap": GRID_ELEMS + 8 * 3 + 5}
_BASE = {}


def _base_input(size, dt):
    """Uniform (-1, 1) values, made once per (size, dtype) and restored after every poke."""
    if (size, dt) not in _BASE:
        g = torch.Generator().manual_seed(7)
        _BASE[size, dt] = (torch.rand(AMAX_N[size], generator=g) * 2 - 1).to(dt).to(DEV)
    return _BASE[size, dt]


def _block_of(pos, n):
    """The block of nd_fp8_cast that reads element ``pos`` (its amax goes to slot block % parts)."""
    n8 = n // 8
    blocks = min(2048, max(1, (n8 + 255) // 256))
    if pos >= n8 * 8:
        return (pos - n8 * 8) // 256, blocks
    return (pos // 8) % (blocks * 256) // 256, blocks


@pytest.mark.parametrize("parts", [1, 3, 64, 100])
@pytest.mark.parametrize("size,dt", [("five-blocks", BF16), ("five-blocks", F32), ("wrap", BF16)])
def test_amax_contract(size, dt, parts):
    """amax_out[b % parts] = max(amax_out[b % parts], block b's max |x|): an atomic max onto the prior content, in
    slots below min(blocks, parts) only, wherever the maximum sits -- element 0, the last full vector, each tail
    position, the second grid trip -- and whatever its sign; the amax-only pass gives the same slots."""
    n = AMAX_N[size]
    x = _base_input(size, dt)
    n8 = n // 8
    spots = [0, n8 * 8 - 8 + 3] + [n8 * 8 + t for t in range(n % 8)]
    if size == "wrap":
        spots.append(GRID_ELEMS + 8 * 2 + 1)  # reached only in the second trip of the grid-stride loop
    M = 3.0
    slot = torch.arange(parts, dtype=F32, device=DEV)
    priors = {"zero": torch.zeros(parts, device=DEV), "below": 0.25 + slot * 2.0 ** -10, "above": 8.0 + slot}
    big, out = q_frame(n, fmt=fp8.E4M3)
    s = sc(2.0)
    for pname, prior in priors.items():
        for j, pos in enumerate(spots):
            keep = x[pos].clone()
            x[pos] = -M if j % 2 else M
            try:
                got = []
                for with_out in (True, False):
                    abig, amax = amax_frame(parts, prior)
                    rc = lib_cast(x, n, s if with_out else None, out if with_out else None, fp8.E4M3, amax, parts)
                    assert rc == 0
                    torch.cuda.synchronize()
                    assert_frame_intact(abig, amax)
                    got.append(amax.clone())
                assert_frame_intact(big, out)
            finally:
                x[pos] = keep
            a = got[0]
            note = (size, parts, pname, pos)
            assert torch.equal(got[0], got[1]), note  # the amax-only pass (out == 0, scale == 0): same slots
            blk, blocks = _block_of(pos, n)
            assert bool((a >= prior).all()), note  # never lowered: a max, not a store
            assert bool((a <= torch.clamp(prior, min=M)).all()), note
            assert bool((a[prior > M] == prior[prior > M]).all()), note
            assert bool((a[min(blocks, parts):] == prior[min(blocks, parts):]).all()), note
            assert a.max().item() == max(M, prior.max().item()), note
            assert a[blk % parts].item() == max(M, prior[blk % parts].item()), note
    assert x.double().abs().max().item() <= 1.0  # every poke restored


@dt_p
@fmt_p
def test_scale_pointer_zero_means_scale_one(fmt, dt):
    x0 = cycled(probe_input(fmt, dt, 1.0), 2048 + 5)
    x = x0.to(DEV)
    big, out = q_frame(x0.numel(), fmt)
    assert lib_cast(x, x0.numel(), None, out, fmt, None, 1) == 0  # no amax buffer either
    torch.cuda.synchronize()
    assert_frame_intact(big, out)
    assert_bytes(out, oracle(x0, 1.0, fmt), fmt, "scale == 0")


# ------------------------------------------------------------------------------------------ cast + transpose
def _finite_probes(fmt, dt):
    p = o64.fp8_probes(fmt, dt)
    return torch.cat([p[p.float().abs() <= o64.FP8_FMAX[fmt]], torch.tensor([NAN], dtype=dt)])


@pytest.mark.parametrize("pad,off", [(0, 0), (8, 0), (64, 8)], ids=["ld=cols", "ld=cols+8", "ld=cols+64"])
@pytest.mark.parametrize("rows,cols", [(64, 64), (64, 192), (192, 64), (128, 320)])
@dt_p
@fmt_p
def test_cast_t(fmt, dt, rows, cols, pad, off):
    """One tile, a row of tiles, a column of tiles, a 2 x 5 grid; contiguous rows and column slices of a wider
    probe-filled tensor; with and without the plain output.  Both outputs are the oracle's bytes and their
    transpose inside frames; the maximum sits in the last tile and lands in slot (last block) % parts."""
    ld = cols + pad
    wide0 = cycled(_finite_probes(fmt, dt), rows * ld).view(rows, ld).clone()
    M = -1e30 if (rows + cols + pad) % 128 else 1e30
    wide0[rows - 1, off + cols - 3] = M
    Mv = abs(wide0[rows - 1, off + cols - 3].item())
    wide = wide0.to(DEV)
    x = wide[:, off:off + cols]
    ref = oracle(wide0[:, off:off + cols], 1.0, fmt)
    s = sc(1.0)
    nblk = (rows // 64) * (cols // 64)
    parts = 3
    for plain in (True, False):
        big, out = q_frame(rows * cols, fmt)
        bigT, outT = q_frame(rows * cols, fmt)
        prior = torch.tensor([0.0, 0.125, 500.0], device=DEV)
        abig, amax = amax_frame(parts, prior)
        rc = lib_cast_t(x, rows, cols, ld, s, out if plain else None, outT, fmt, amax, parts)
        assert rc == 0
        torch.cuda.synchronize()
        assert_frame_intact(bigT, outT)
        assert_frame_intact(abig, amax)
        if plain:
            assert_frame_intact(big, out)
            assert_bytes(out, ref, fmt, "cast_t out")
        else:
            assert_frame_intact(big)  # out == nullptr: nothing written there
        assert_bytes(outT, ref.t().contiguous(), fmt, "cast_t outT")
        assert bool((amax >= prior).all()) and bool((amax <= Mv).all())
        assert bool((amax[min(nblk, parts):] == prior[min(nblk, parts):]).all())
        assert amax.max().item() == Mv and amax[(nblk - 1) % parts].item() == Mv


@dt_p
def test_cast_t_refusals(dt):
    """Shapes and pointers the kernel cannot take come back as hipErrorInvalidValue before any launch: both output
    frames and the amax buffer stay untouched."""
    wide = torch.randn(128, 136, device=DEV).to(dt)
    big, flat = q_frame(128 * 128 + 16, fp8.E4M3)
    bigT, flatT = q_frame(128 * 128 + 16, fp8.E4M3)
    abig, amax = amax_frame(4, 0.5)
    s = sc(1.0)
    cases = {
        "63 rows": (wide, 63, 64, 136, flat, flatT),
        "65 rows": (wide, 65, 64, 136, flat, flatT),
        "96 columns": (wide, 64, 96, 136, flat, flatT),
        "ld 68": (wide, 64, 64, 68, flat, flatT),
        "outT == 0": (wide, 64, 64, 136, flat, None),
        "x off by one element": (wide.view(-1)[1:], 64, 64, 136, flat, flatT),
        "out off by one byte": (wide, 64, 64, 136, flat[1:], flatT),
        "outT off by one byte": (wide, 64, 64, 136, flat, flatT[1:]),
        "outT off by eight bytes": (wide, 64, 64, 136, flat, flatT[8:]),
    }
    for name, (x, rows, cols, ld, o, oT) in cases.items():
        assert lib_cast_t(x, rows, cols, ld, s, o, oT, fp8.E4M3, amax, 4) == INVALID, name
    torch.cuda.synchronize()
    assert_frame_intact(big)
    assert_frame_intact(bigT)
    assert_frame_intact(abig, amax)
    assert amax.tolist() == [0.5] * 4


# ------------------------------------------------------------------------------------------ alignment
@dt_p
def test_cast_refuses_misaligned_pointers(dt):
    """x one element off a 16-byte boundary, out one byte off an 8-byte boundary: refused before any launch."""
    n = 64
    xbuf = torch.randn(n + 8, device=DEV).to(dt)
    big, out = q_frame(n + 8, fp8.E4M3)
    abig, amax = amax_frame(4, 0.5)
    s = sc(1.0)
    assert lib_cast(xbuf[1:], n, s, out, fp8.E4M3, amax, 4) == INVALID
    assert lib_cast(xbuf, n, s, out[1:], fp8.E4M3, amax, 4) == INVALID
    assert lib_cast(xbuf[1:], n, None, None, fp8.E4M3, amax, 4) == INVALID  # the amax-only pass loads 16 bytes too
    torch.cuda.synchronize()
    assert_frame_intact(big)
    assert_frame_intact(abig, amax)
    assert amax.tolist() == [0.5] * 4


@dt_p
@fmt_p
def test_wrappers_copy_misaligned_views(fmt, dt):
    """fp8.cast / absmax_into / cast_t on views that start one element off: copied to fresh storage, same bytes."""
    n = 1000 * 7 + 3
    flat0 = cycled(probe_input(fmt, dt, 37.5), n + 1)
    flat = flat0.to(DEV)
    amax = torch.zeros(fp8.AMAX_PARTS, device=DEV)
    q = fp8.cast(flat[1:1 + n], sc(37.5), fmt, amax)
    assert_bytes(q, oracle(flat0[1:1 + n], 37.5, fmt), fmt, "cast(flat[1:])")
    assert amax.max().item() == true_amax(flat0[1:1 + n])
    fin0 = cycled(_finite_probes(fmt, dt)[:-1], n + 1)
    a2 = torch.zeros(fp8.AMAX_PARTS, device=DEV)
    fp8.absmax_into(fin0.to(DEV)[1:], a2)
    assert a2.max().item() == true_amax(fin0[1:])
    wide0 = cycled(_finite_probes(fmt, dt), 64 * 129).view(64, 129)
    out, outT = fp8.cast_t(wide0.to(DEV)[:, 1:129], sc(1.0), fmt)
    ref = oracle(wide0[:, 1:129], 1.0, fmt)
    assert_bytes(out, ref, fmt, "cast_t(view)")
    assert_bytes(outT, ref.t().contiguous(), fmt, "cast_t(view)^T")


# ------------------------------------------------------------------------------------------ fused producers
PRIOR = 2.0 ** -24  # the non-zero prior content of every amax slot in the fused-producer tests


def _target(fmt, scale):
    r = fp8.Fp8Recipe(DEV, capacity=4)
    k = r.new_slot(fmt)
    r.scale[k] = scale
    r.ready[k] = True
    r.amax.fill_(PRIOR)
    return r, k, r.target(k, fmt)


def _bits(t):
    return t.detach().view(torch.int16)


def _check_side_output(q, bf, r, k, fmt, what):
    """q == oracle(the bf16 tensor the same launch returned); amax == max |bf16| folded onto the prior; the other
    recipe slots untouched."""
    assert bf.dtype == BF16 and q.shape == bf.shape
    ref = o64.fp8_quantise(bf.detach(), r.scale[k].item(), fmt)  # on the GPU: bf16 values, no subnormal products
    assert_bytes(q, ref, fmt, what)
    a = r.amax[k]
    assert a.max().item() == max(PRIOR, true_amax(bf)), what
    assert bool((a >= PRIOR).all()), what
    assert bool((r.amax[k + 1:] == PRIOR).all()), what


NORM_Q_ROWS, NORM_Q_COLS = [1, 3, 257], [8, 520, 4096]


def _norm_q_case(hdt, rows, cols, nonfinite=False):
    h = o64.spiked(rows, cols, DEV).to(hdt)
    a = o64.spiked(rows, cols, DEV, 0.5, start=3).bfloat16()
    w = 1 + 0.1 * torch.randn(cols, device=DEV)
    dy = o64.spiked(rows, cols, DEV, 1.0, start=5).bfloat16()
    if nonfinite:
        h[rows // 2, cols - 3] = NAN  # an input NaN: that row of y and of the branch gradient is NaN
        h[0, 2:4], a[0, 2:4] = 4.0, 0.0
        w[2], w[3] = 3e38, -3e38  # 4 / rms > 1.13: y[0, 2] = +inf, y[0, 3] = -inf
    outs = {}
    for fused in (True, False):
        r, k, q = _target(fp8.E4M3, 50.0)
        rb, kb, qb = _target(fp8.E5M2, 1000.0)
        hr, ar = h.clone().requires_grad_(True), a.clone().requires_grad_(True)
        y, hn = ops.add_rmsnorm(hr, ar, w, None, 1e-5, BF16, q8=q if fused else None, q8_bwd=qb if fused else None)
        (da,) = torch.autograd.grad(y, ar, dy)
        yp = ops.rmsnorm(h, w, None, 1e-5, BF16, q8=None)
        outs[fused] = (y.detach(), da)
        if not fused:
            continue
        _check_side_output(q.out, y.detach(), r, k, fp8.E4M3, f"rmsnorm y {rows}x{cols}")
        q8 = rb.take_stashed(kb, da)
        assert q8 is not None
        _check_side_output(q8, da, rb, kb, fp8.E5M2, f"rmsnorm da {rows}x{cols}")
        # the plain (no residual add) forward with a side output
        r2, k2, q2 = _target(fp8.E5M2, 7.0)
        yq = ops.rmsnorm(h, w, None, 1e-5, BF16, q8=q2)
        assert torch.equal(_bits(yq), _bits(yp))
        _check_side_output(q2.out, yq.detach(), r2, k2, fp8.E5M2, f"rmsnorm plain y {rows}x{cols}")
    # the bf16 outputs are bitwise those of the launchers without a side output
    assert torch.equal(_bits(outs[True][0]), _bits(outs[False][0]))
    assert torch.equal(_bits(outs[True][1]), _bits(outs[False][1]))
    return outs[True]


@pytest.mark.parametrize("hdt", [F32, BF16], ids=["res-fp32", "res-bf16"])
@pytest.mark.parametrize("cols", NORM_Q_COLS)
@pytest.mark.parametrize("rows", NORM_Q_ROWS)
def test_fused_rmsnorm_side_outputs(rows, cols, hdt):
    _norm_q_case(hdt, rows, cols)


@pytest.mark.parametrize("hdt", [F32, BF16], ids=["res-fp32", "res-bf16"])
def test_fused_rmsnorm_side_outputs_nonfinite(hdt):
    y, da = _norm_q_case(hdt, 3, 520, nonfinite=True)
    assert bool(torch.isnan(y[1]).all()) and y[0, 2:4].tolist() == [float("inf"), -float("inf")]
    assert bool(torch.isnan(da[1]).all())


def _swiglu_q_case(fmt, n, F, nonfinite=False):
    from nanodiloco_amd.ops.swiglu import SwiGLUFn
    if n * F <= 1 << 20:
        gu = o64.spiked(n, 2 * F, DEV, 2.0).bfloat16()
        dy = o64.spiked(n, F, DEV, 1.0, start=2).bfloat16()
    else:  # the wrap: cheap inputs
        gu = torch.randn(n, 2 * F, device=DEV, dtype=BF16)
        dy = torch.randn(n, F, device=DEV, dtype=BF16)
        gu[-1, F - 1], gu[-1, 2 * F - 1] = 30.0, -40.0  # the maximum in the last vector, second grid trip
    if nonfinite:
        gu[0, 1] = NAN  # gate
        gu[n - 1, F + 2] = NAN  # up
        gu[n // 2, F + 5], gu[n // 2, F + 6] = float("inf"), -float("inf")
        gu[n // 2, 5], gu[n // 2, 6] = 2.0, 3.0
    outs = {}
    for fused in (True, False):
        r, k, q = _target(fmt, 23.0)
        rb, kb, qb = _target(fp8.E5M2, 3.0)
        g = gu.clone().requires_grad_(True)
        out = SwiGLUFn.apply(g, q if fused else None, qb if fused else None)
        (dgu,) = torch.autograd.grad(out, g, dy)
        outs[fused] = (out.detach(), dgu)
        if fused:
            _check_side_output(q.out, out.detach(), r, k, fmt, f"swiglu fwd {n}x{F}")
            q8 = rb.take_stashed(kb, dgu)
            assert q8 is not None
            _check_side_output(q8, dgu, rb, kb, fp8.E5M2, f"swiglu bwd {n}x{F}")
            del q8, q
    assert torch.equal(_bits(outs[True][0]), _bits(outs[False][0]))
    assert torch.equal(_bits(outs[True][1]), _bits(outs[False][1]))
    return outs[True]


@pytest.mark.parametrize("n,F", [(1, 8), (3, 8), (777, 8), (1, 72), (3, 72), (777, 72), (4 * 1024 * 1024 + 5, 8)])
@fmt_p
def test_fused_swiglu_side_outputs(fmt, n, F):
    """n x F from one vector to a few blocks, and one wrap of the 16384-block grid cap with five vectors more."""
    _swiglu_q_case(fmt, n, F)


@fmt_p
def test_fused_swiglu_side_outputs_nonfinite(fmt):
    out, dgu = _swiglu_q_case(fmt, 3, 72, nonfinite=True)
    assert bool(torch.isnan(out[0, 1])) and bool(torch.isnan(out[2, 2]))
    assert out[1, 5].item() == float("inf") and out[1, 6].item() == -float("inf")


IGN = -100


def _ce_inputs(V):
    """The 18-row pattern of test_rowwise_edges_gpu._ce_inputs: three logit patterns (4 randn; one +60 among -60;
    constant) x six targets (0, V - 1, a column of the last partial chunk, a middle column, ignore_index, arg-max)."""
    n = 18
    x = 4 * torch.randn(n, V, device=DEV)
    peak = [V - 1, 0, max(0, V - 3), V // 2, V // 3, (V - 1) // 8 * 8]
    for k, r in enumerate(range(1, n, 3)):
        x[r] = -60.0
        x[r, peak[k]] = 60.0
    x[2::3] = 1.5
    x = x.bfloat16()
    tgt = torch.empty(n, dtype=torch.long, device=DEV)
    kinds = [0, V - 1, max(0, V - 3), V // 2, IGN, None]
    for r in range(n):
        k = kinds[(r // 3 + r % 3) % 6]
        tgt[r] = int(x[r].float().argmax()) if k is None else k
    return x, tgt


def _ce_q8(x, tgt, scale, fmt, qscale, loss0=3.0):
    """(q bytes, recipe, slot, loss, rc) of nd_ce_fwd_bwd_q8 on framed logits that must come back untouched."""
    n, V = x.shape
    lbig, lflat = framed_flat(n * V, BF16, pad=64)
    logits = lflat.view(n, V)
    logits.copy_(x)
    r, k, t = _target(fmt, qscale)
    big, qflat = q_frame(n * V, fmt, pad=64)
    loss = torch.full((1,), loss0, device=DEV)
    rc = _ext.lib().nd_ce_fwd_bwd_q8(logits.data_ptr(), _ext.dtcode(logits), tgt.data_ptr(), loss.data_ptr(),
                                     scale.data_ptr(), n, V, IGN, 0, 0, *t.args(qflat), S())
    torch.cuda.synchronize()
    assert_frame_intact(lbig, lflat)
    assert torch.equal(_bits(logits), _bits(x)), "the logits were modified"
    assert_frame_intact(big, qflat)
    return qflat.view(n, V), big, r, k, loss, rc


def _ce_bf16(x, tgt, scale, loss0=3.0):
    d = x.clone()
    loss = torch.full((1,), loss0, device=DEV)
    _ext.check(_ext.lib().nd_ce_fwd_bwd(d.data_ptr(), _ext.dtcode(d), tgt.data_ptr(), loss.data_ptr(),
                                        scale.data_ptr(), x.shape[0], x.shape[1], IGN, 0, 0, 0.0, S()), "nd_ce_fwd_bwd")
    return d, loss


@pytest.mark.parametrize("case", ["pattern", "nan-logit", "all-ignored"])
@pytest.mark.parametrize("V", [8200, 32768])
@fmt_p
def test_ce_q8_side_output(fmt, V, case):
    """V at the two ends of what nd_ce_fwd_bwd_q8 accepts: the fp8 dlogits are the oracle of the bf16 dlogits the
    in-place launcher writes; ignored rows are all-zero bytes; a NaN logit makes its row NaN bytes."""
    x, tgt = _ce_inputs(V)
    if case == "nan-logit":
        x[0, 17] = NAN
        assert tgt[0].item() != IGN
    if case == "all-ignored":
        tgt[:] = IGN
    scale = sc(1.0 / 16)
    d, loss_ref = _ce_bf16(x, tgt, scale)
    q, big, r, k, loss, rc = _ce_q8(x, tgt, scale, fmt, 2000.0)
    assert rc == 0
    _check_side_output(q, d, r, k, fmt, f"ce V={V} {case}")
    ign = tgt == IGN
    assert bool((q.view(torch.uint8)[ign] == 0).all())
    if case == "all-ignored":
        assert loss.item() == 3.0 and bool((r.amax[k] == PRIOR).all())
    elif case == "nan-logit":
        assert bool(o64.fp8_is_nan(q[0], fmt).all()) and not bool(o64.fp8_is_nan(q[1:], fmt).any())
        assert loss.item() != loss.item()
    else:
        assert abs(loss.item() - loss_ref.item()) <= 1e-5 * abs(loss_ref.item())


@pytest.mark.parametrize("V", [8192, 32776])
def test_ce_q8_refuses_outside_its_range(V):
    x, tgt = _ce_inputs(V)
    q, big, r, k, loss, rc = _ce_q8(x, tgt, sc(1.0 / 16), fp8.E5M2, 2000.0)
    assert rc == INVALID
    assert_frame_intact(big)
    assert loss.item() == 3.0 and bool((r.amax == PRIOR).all())


# ------------------------------------------------------------------------------------------ first use and weights
@fmt_p
def test_first_use_of_an_all_zero_tensor(fmt):
    r = fp8.Fp8Recipe(DEV, capacity=4)
    k = r.new_slot(fmt)
    q = r.quantize(torch.zeros(3, 520, device=DEV, dtype=BF16), k, fmt)
    assert bool((q.view(torch.uint8) == 0).all())
    assert r.ready[k] and torch.isfinite(r.scale[k]) and torch.isfinite(r.inv[k]) and r.scale[k] > 0
    assert r.inv[k].item() == (1.0 / r.scale[k]).item()


def test_weight_all_zero_and_amax_in_the_last_row():
    wq = fp8.Fp8Weight().get(torch.zeros(128, 64, device=DEV, dtype=BF16), version=0)
    assert bool((wq.w8.view(torch.uint8) == 0).all()) and bool((wq.wT8.view(torch.uint8) == 0).all())
    assert torch.isfinite(wq.inv).all() and wq.inv.item() > 0
    for shape in [(96, 72), (65, 8), (128, 64)]:  # the last one takes the cast + transpose kernel
        w0 = (torch.randn(*shape) * 0.02).bfloat16()
        w0[shape[0] - 1, shape[1] - 3] = -0.75
        w = w0.to(DEV)
        wq = fp8.Fp8Weight().get(w, version=0)
        s = 448.0 / w.float().abs().max()  # FMAX / amax: the fp32 division on the device, as Fp8Weight computes it
        assert abs(s.item() - 448.0 / 0.75) <= 2.0 ** -14 * 448.0 / 0.75  # within fp32 rounding of 597.33...
        assert wq.inv.item() == (1.0 / s).item()
        ref = oracle(w0, s.item(), fp8.E4M3)
        assert int(ref[shape[0] - 1, shape[1] - 3]) == 0xFE  # -FMAX
        assert_bytes(wq.w8, ref, fp8.E4M3, f"w8 {shape}")
        assert_bytes(wq.wT8, ref.t().contiguous(), fp8.E4M3, f"wT8 {shape}")
