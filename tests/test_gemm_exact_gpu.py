"""The MFMA GEMM family (csrc/gemm_pp.hip, gemm_w128.hip, gemm_wgrad.hip) on inputs for which the fp32 accumulator
is exact (tests/_gemm_exact.py): small-integer operands, so every fp32 output must equal the integer product bit
for bit and every bf16 output its one rounding, in any summation order, split-K or tile walk; and the fused
epilogues (RoPE, SwiGLU forward / backward in both saved forms, the fp8-output forms) on inputs whose projection
survives the bf16 rounding unchanged, so the float64 oracle knows the epilogue's input exactly and judges its output
per element by the rule of tests/_oracle64.py.  A handful of Gaussian cases hold the accumulator's own rounding to
the same rule.  docs/PARITY.md ("T3 GEMM") has the argument, the measured margins and what these tests see that the
norm-ratio tests do not.

Every output is a view in a sentinel frame (row stride wider than the row), operands are strided views of a wider
pool.  Tile arithmetic: gemm_pp / gemm_w128 tiles are 256 x 256 (8 waves: two 128-row groups x four 64-column
waves); the SwiGLU tile is 256 x 128 units (wave group = 32 units, pair16 block = 16 columns); the K-tile is 64
(bf16) or 128 (fp8) deep, two 32-deep k-steps; the weight-gradient kernels tile 256 x 256 (128 x 128 below 8 tiles)
over 64-token (fp8: 128-token) K-tiles."""
import functools

import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import _ext, fp8
from nanodiloco_amd.ops import gemm as G

from . import _gemm_exact as X
from . import _oracle64 as o64
from ._frames import assert_frame_intact, framed
from ._switches import switches

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, E4, E5 = torch.bfloat16, torch.float32, X.E4, X.E5
AMAX = 8  # |operand| <= 8

# per-output margins other than 8 (twice the measured ratio, rounded up to a power of two); docs/PARITY.md (T3 GEMM)
MARGINS = {
    # measured 476 (bf16 out) and 1090 to 1470 (fp32 out, two runs) on the spiked Gaussian operands:
    # v_mfma_scale_f32_16x16x128_f8f6f4 does not add its 128 products one by one in fp32.  Measured through wgrad_f8 with power-of-two operands: a
    # product 2^14 or more below the largest product of its sub-block (the 7 neighbours of a spike) is dropped whole,
    # one 2^13 below survives intact; the fp32 twin, the unit of the slack, keeps them all.  With 8-sigma spikes in
    # both operands a spike product stands 2^6 to 2^12 above the ordinary ones; that its neighbours then lose the
    # bits below that line is inferred from the probe, not measured bit by bit.  The same kernels are bitwise exact
    # on the integer operands above, whose products span 2^6.
    "pp_f8.gauss": 1024.0,
    "wgrad_f8.gauss": 4096.0,
}
REPORT = {}


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    G.set_gemm_backend("hip")
    gm, form = G.set_pp_group_m(4), G.mlp_coef()
    wgm = G.set_w128(group_m=4, nt=1, ovl=1)
    vb = G.set_w128_vb(0)
    torch.manual_seed(0)
    yield
    G.set_pp_group_m(gm)
    G.set_mlp_coef(form)
    G.set_w128(group_m=wgm, nt=1, ovl=1)
    G.set_w128_vb(vb)
    assert G.set_pp_variant(0) == 0, "a test left a ping-pong variant set"
    assert _ext.lib().nd_wgrad_force_splits(0) == 0, "a test left a forced split count"
    ops.set_backend("auto")


@pytest.fixture(scope="module", autouse=True)
def _slack_report():
    yield
    for k in sorted(REPORT):
        print(f"\n[slack] {k}: needs margin {REPORT[k]:.3g} (allowed {MARGINS.get(k, o64.MARGIN)})", end="")
    print()


def chk(out, ref64, twin, name, note=""):
    o64.check(out, ref64, twin, margin=MARGINS.get(name, o64.MARGIN), name=name, report=REPORT, note=note)


# ------------------------------------------------------------------------------------------ operands, references
POOL_R, POOL_C, OFF_R, OFF_C = 2720, 5504, 3, 128  # rows / columns of the pools; where the views start


@functools.lru_cache(maxsize=None)
def _pool(dtype, seed):
    return X.int_operand(POOL_R, POOL_C, -AMAX, AMAX, dtype, seed, DEV)


def operand(rows, cols, dtype, seed):
    """Integer-valued [rows, cols] in [-8, 8]: a strided view (row stride 5504, 16-B aligned start off the
    allocation's origin) of a pool that is drawn once."""
    assert OFF_R + rows <= POOL_R and OFF_C + cols <= POOL_C
    return _pool(dtype, seed)[OFF_R:OFF_R + rows, OFF_C:OFF_C + cols]


@functools.lru_cache(maxsize=None)
def ref_nt(adt, bdt, M, N, K):
    """The exact product of operand(M, K, adt, 1) and operand(N, K, bdt, 2), computed once, never written to."""
    return X.exact_nt(operand(M, K, adt, 1), operand(N, K, bdt, 2))


@functools.lru_cache(maxsize=None)
def gw_init(M, N):
    return X.int_operand(M, N, -1000, 1000, F32, 5, DEV)


@functools.lru_cache(maxsize=None)
def ref_tn(adt, bdt, M, N, K):
    return X.exact_tn(operand(K, M, adt, 3), operand(K, N, bdt, 4))


def scale(v):
    return torch.tensor([v], device=DEV, dtype=F32)


def into_frame(fn, M, N, dtype=BF16):
    """Run ``fn(out)`` on a framed [M, N] view and check the frame."""
    big, out = framed(M, N, dtype)
    fn(out)
    torch.cuda.synchronize()
    assert_frame_intact(big, out)
    return out


def frame8(rows, cols, dtype):
    """A [rows, cols] view of a 1-byte dtype in a frame of 0xA5 bytes (tests/_frames.py holds 2- and 4-byte ones)."""
    big = torch.full((rows + 2, cols + 32), 0xA5, dtype=torch.uint8, device=DEV)
    return big, big[1:1 + rows, 16:16 + cols].view(dtype)


def frame8_intact(big, rows, cols):
    b = big.clone()
    b[1:1 + rows, 16:16 + cols] = 0xA5
    assert bool((b == 0xA5).all()), "a neighbouring byte was overwritten"


# ------------------------------------------------------------------------------------------ plain NT products
# (M, N): one wave's corner of one tile; a 64-row strip; one half-tile (group 0, wave 0); one row into group 1 and 8
# columns into wave 1; one full tile; 1 row / 8 columns into the second tile row / column; 44-row and 8-column tails
# two tiles down / three across; 1-row tail in the third tile row, 232-column tail (40 past the 64-column wave 2 ->
# wave 3 boundary at 960) in the fourth tile column.
NT_SHAPES = [(16, 8), (64, 8), (128, 64), (129, 72), (256, 256), (257, 264), (300, 520), (513, 1000)]
# K-tiles of 64: 1 (prologue only), 2 (one steady step), 3 (odd), 5, 41
NT_KS = [64, 128, 192, 320, 2624]
SA, SB = 0.5, 0.25  # fp8 dequantisation scales: powers of two, the scaled product stays exact


def _nt_all_shapes(fn, adt, bdt, K, sc=1.0, name=""):
    assert X.exact_bound(K, AMAX, AMAX) < X.EXACT_LIMIT
    for M, N in NT_SHAPES:
        a, b = operand(M, K, adt, 1), operand(N, K, bdt, 2)
        out = into_frame(lambda o: fn(a, b, o), M, N)
        X.expect_bits(out, ref_nt(adt, bdt, M, N, K) * sc, f"{name} M={M} N={N} K={K}")


@pytest.mark.parametrize("K", NT_KS)
@pytest.mark.parametrize("gm", [4, 1, 3])
def test_gemm_pp_exact(gm, K):
    G.set_pp_group_m(gm)
    _nt_all_shapes(G.gemm_pp, BF16, BF16, K, name="gemm_pp")


# (group_m, ovl, nt, vb): the tile orders x epilogue placements of tests/test_gemm_w128_gpu.py, plain-policy stores
# in both placements, and the VGPR-staged B operand (which runs with ovl = 1, nt = 1 and K >= 128)
W128_CFG = [(4, 0, 1, 0), (1, 0, 1, 0), (3, 1, 1, 0), (4, 1, 1, 0), (4, 0, 0, 0), (4, 1, 0, 0), (4, 1, 1, 1)]


@pytest.mark.parametrize("K", NT_KS)
@pytest.mark.parametrize("cfg", W128_CFG, ids=lambda c: "gm%d-ovl%d-nt%d-vb%d" % c)
def test_gemm_w128_exact(cfg, K):
    gm, ovl, nt, vb = cfg
    G.set_w128(group_m=gm, nt=nt, ovl=ovl)
    G.set_w128_vb(vb)
    _nt_all_shapes(G.gemm_w128, BF16, BF16, K, name="gemm_w128")


@pytest.mark.parametrize("K", [2 * k for k in NT_KS])  # the fp8 K-tile is 128 deep: the same K-tile counts
@pytest.mark.parametrize("gm", [4, 1, 3])
@pytest.mark.parametrize("adt", [E4, E5], ids=["e4m3", "e5m2"])
def test_gemm_pp_f8_exact(adt, gm, K):
    G.set_pp_group_m(gm)
    sa, sb = scale(SA), scale(SB)
    _nt_all_shapes(lambda a, b, o: G.gemm_pp_f8(a, b, sa, sb, o), adt, E4, K, sc=SA * SB, name="gemm_pp_f8")


def _multi_tile_M(N):
    """Rows for which the 256 x 256 tiles number the first multiple of ceil(N / 256) at or above CUs + 17 (exactly
    CUs + 17 is not always a multiple of the 5 tile columns of N = 1032), with a 44-row tail tile last: every
    workgroup of the persistent grid owns one tile, the first 17 or more a second one."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tn = (N + 255) // 256
    tm = (cus + 17 + tn - 1) // tn
    return (tm - 1) * 256 + 44


@pytest.mark.parametrize("kind", ["pp", "w128", "w128-ovl0", "f8"])
@pytest.mark.parametrize("ktiles", [1, 2])
def test_multi_tile_per_workgroup_exact(kind, ktiles):
    """The epilogue inside the next tile's first phase, a tail tile last (N = 1032: 8 columns in the fifth tile
    column); one and two K-tiles per tile."""
    N = 1032
    M = _multi_tile_M(N)
    K = ktiles * (128 if kind == "f8" else 64)
    adt = E4 if kind == "f8" else BF16
    assert X.exact_bound(K, AMAX, AMAX) < X.EXACT_LIMIT
    a = X.int_operand(M, K + 64, -AMAX, AMAX, adt, 11, DEV)[:, 64:]
    b = operand(N, K, adt, 2)
    G.set_pp_group_m(3)
    if kind == "w128-ovl0":
        G.set_w128(ovl=0)
    sa, sb = scale(SA), scale(SB)
    fn = {"pp": G.gemm_pp, "w128": G.gemm_w128, "w128-ovl0": G.gemm_w128,
          "f8": lambda x, y, o: G.gemm_pp_f8(x, y, sa, sb, o)}[kind]
    out = into_frame(lambda o: fn(a, b, o), M, N)
    X.expect_bits(out, X.exact_nt(a, b, SA * SB if kind == "f8" else 1.0), f"{kind} M={M} N={N} K={K}")


@pytest.mark.parametrize("kind", ["pp", "w128", "e4m3", "e5m2"])
@pytest.mark.parametrize("K", [192, 320])
def test_one_hot_rows_pick_the_right_k(kind, K):
    """Row i of A holds a single 1 at k = (7 i) % K, B holds position-coded integers: C[i, j] = B[j, (7 i) % K]
    exactly -- a K-index or swizzle slip that random data could hide by symmetry moves a value."""
    f8 = kind in ("e4m3", "e5m2")
    if f8:
        K *= 2
    M, N = 300, 520
    adt = {"e4m3": E4, "e5m2": E5}.get(kind, BF16)
    i = torch.arange(M, device=DEV)
    kk = (7 * i) % K
    a = torch.zeros(M, K + 128, device=DEV)
    a[i, 128 + kk] = 1.0
    a = a.to(adt)[:, 128:]
    j, k = torch.arange(N, device=DEV)[:, None], torch.arange(K, device=DEV)[None, :]
    code = ((k * 7 + j * 3) % 31 - 15).float()  # |.| <= 15: exact in bf16 and e4m3
    b = code.to(E4 if f8 else BF16)
    assert torch.equal(b.float(), code)
    assert X.exact_bound(1, 1, 15) < X.EXACT_LIMIT  # one non-zero product per output
    want = code[:, kk].t().double()  # [M, N]
    sa, sb = scale(1.0), scale(1.0)
    fn = {"pp": G.gemm_pp, "w128": G.gemm_w128}.get(kind, lambda x, y, o: G.gemm_pp_f8(x, y, sa, sb, o))
    out = into_frame(lambda o: fn(a, b, o), M, N)
    X.expect_bits(out, want, f"one-hot {kind} K={K}")
    assert torch.equal(X.exact_nt(a, b), want)


# one full tile; M and N tails (44 rows, 8 columns); a single K-tile with 1-row / 8-column tails
VARIANT_SHAPES = [(256, 256, 320), (300, 520, 192), (257, 264, 64)]


@pytest.mark.parametrize("variant", [32, 256, 288, 1024, 2048, 2080])
def test_gemm_pp_store_and_staging_variants_exact(variant):
    """The correct-result A/B builds of the ping-pong kernel: store policy (32, 2048, 2080), the direct-store epilogue
    branch (256, 288), buffer-form DMA pieces for every half-tile (1024)."""
    for M, N, K in VARIANT_SHAPES:
        assert X.exact_bound(K, AMAX, AMAX) < X.EXACT_LIMIT
        a, b = operand(M, K, BF16, 1), operand(N, K, BF16, 2)
        base = into_frame(lambda o: G.gemm_pp(a, b, o), M, N)
        assert G.set_pp_variant(variant) == 0, f"variant {variant} is not in this build"
        try:
            out = into_frame(lambda o: G.gemm_pp(a, b, o), M, N)
        finally:
            assert G.set_pp_variant(0) == variant
        X.expect_bits(out, ref_nt(BF16, BF16, M, N, K), f"gemm_pp variant {variant} M={M} N={N} K={K}")
        assert torch.equal(out, base)


# ------------------------------------------------------------------------------------------ weight gradients
L = _ext.lib


def run_wgrad(M, N, K, name):
    """gw (framed, integer-valued start) += dy^T x with the slab workspace sized as ops.gemm.wgrad sizes it and
    prefilled with a finite wrong value: a stale plane shows as a wrong integer."""
    assert X.exact_bound(K, AMAX, AMAX, 1000) < X.EXACT_LIMIT
    dy, x = operand(K, M, BF16, 3), operand(K, N, BF16, 4)
    assert G.wgrad_supported(gw_init(M, N), dy, x)
    S = L().nd_wgrad_splits(M, N, K)
    ws = torch.full((max(S, 1) * M * N,), 3.0, device=DEV)

    def launch(gw):
        gw.copy_(gw_init(M, N))
        _ext.check(L().nd_wgrad(_ext.ptr(dy), _ext.ptr(x), _ext.ptr(gw), _ext.ptr(ws), M, N, K, dy.stride(0),
                                x.stride(0), gw.stride(0), _ext.stream_ptr(gw.device)), "nd_wgrad")

    gw = into_frame(launch, M, N, F32)
    X.expect_bits(gw, ref_tn(BF16, BF16, M, N, K) + gw_init(M, N).double(), f"{name} M={M} N={N} K={K} S={S}")
    return gw


# below 8 tiles of 256 x 256: the 128 x 128 kernel (one corner; one tile + 8 columns; 3 x 5 tiles with 8-row /
# 8-column tails = 6 tiles of 256); K: less than one k-step, one K-tile, one K-tile + 8, 12 K-tiles + 9
@pytest.mark.parametrize("K", [8, 64, 72, 777])
def test_wgrad_small_kernel_exact(K):
    for M, N in [(8, 8), (128, 136), (264, 520)]:
        run_wgrad(M, N, K, "wgrad 128x128")


# 8 tiles of 256 exactly (2 x 4), and 3 x 5 tiles with 8-row / 8-column tails
PP_MN = [(512, 1024), (520, 1032)]


@pytest.mark.parametrize("K", [64, 128, 192, 2624])
@pytest.mark.parametrize("variant", ["", "b", "dma0", "dmas"])
def test_wgrad_large_kernels_exact(variant, K):
    """The ping-pong kernel (default, and buffer-form pieces "b") and the LDS-DMA kernel through its switch."""
    with switches(ND_WGRAD_VARIANT=variant):
        for M, N in PP_MN:
            run_wgrad(M, N, K, f"wgrad {variant or 'pp'}")


@pytest.mark.parametrize("K", [72, 777, 2600])
def test_wgrad_dma_kernel_by_k_tail_exact(K):
    """K % 64 != 0 selects the LDS-DMA kernel with its register-staged last K-tile."""
    for M, N in PP_MN:
        run_wgrad(M, N, K, "wgrad dma (K tail)")


@pytest.mark.parametrize("K", [2624, 320])
@pytest.mark.parametrize("variant", ["", "dma0"])
def test_wgrad_forced_splits_all_give_the_same_bits(variant, K):
    """nd_wgrad_force_splits reaches split counts the plan does not choose; at K = 320 (5 K-tiles) and K = 2624
    (41) fit_kchunk must shrink 8 and 16.  Every count gives the exact integers, hence the same bits."""
    M, N = 520, 1032
    outs = {}
    with switches(ND_WGRAD_VARIANT=variant):
        for s in (1, 2, 3, 5, 8, 16):
            L().nd_wgrad_force_splits(s)
            try:
                assert L().nd_wgrad_splits(M, N, K) == s
                outs[s] = run_wgrad(M, N, K, f"wgrad {variant or 'pp'} forced {s}")
            finally:
                L().nd_wgrad_force_splits(0)
    for s, o in outs.items():
        assert torch.equal(o, outs[1]), s


# two pairs the plan groups: unequal tile counts (3 x 5 = 15 and 4 x 3 = 12; 4 x 5 = 20 and 3 x 8 = 24), tails of 8
# rows / columns in both products
W2_PAIRS = [((520, 1032), (776, 520)), ((1000, 1032), (520, 2048))]


@pytest.mark.parametrize("pair", W2_PAIRS, ids=["15+12", "20+24"])
def test_wgrad2_exact(pair):
    (M0, N0), (M1, N1) = pair
    K = 2624
    assert X.exact_bound(K, AMAX, AMAX, 1000) < X.EXACT_LIMIT
    S = L().nd_wgrad2_splits(M0, N0, M1, N1, K)
    if S <= 0:
        pytest.skip(f"the plan does not group {pair} at K = {K} on this device")
    dy0, x0 = operand(K, M0, BF16, 3), operand(K, N0, BF16, 4)
    dy1, x1 = operand(K, M1, BF16, 1), operand(K, N1, BF16, 2)
    G._workspace(torch.device(DEV), S * (M0 * N0 + M1 * N1)).fill_(3.0)
    b0, g0 = framed(M0, N0, F32)
    b1, g1 = framed(M1, N1, F32)
    g0.copy_(gw_init(M0, N0))
    g1.copy_(gw_init(M1, N1))
    assert G.wgrad2(g0, dy0, x0, g1, dy1, x1)
    torch.cuda.synchronize()
    assert_frame_intact(b0, g0)
    assert_frame_intact(b1, g1)
    X.expect_bits(g0, X.exact_tn(dy0, x0, gw_init(M0, N0)), f"wgrad2[0] {pair} S={S}")
    X.expect_bits(g1, X.exact_tn(dy1, x1, gw_init(M1, N1)), f"wgrad2[1] {pair} S={S}")


# one tile; 2 x 3 tiles with 16-row / 16-column tails; 8 tiles.  K-tiles of 128 tokens: 1, 2, 3, 10
@pytest.mark.parametrize("K", [128, 256, 384, 1280])
@pytest.mark.parametrize("ddt", [E5, E4], ids=["e5m2", "e4m3"])
def test_wgrad_f8_exact(ddt, K):
    sdy, sx = 0.5, 0.25  # the result is a multiple of 1/8: exact while 8 * |value| < 2^24
    assert 8 * X.exact_bound(K, AMAX, AMAX, 8 * 1000) < X.EXACT_LIMIT
    for M, N in [(256, 256), (272, 528), (512, 1024)]:
        dy, x = operand(K, M, ddt, 3), operand(K, N, E4, 4)
        assert G.wgrad_f8_supported(gw_init(M, N), dy, x)
        S = L().nd_wgrad_f8_splits(M, N, K)
        G._workspace(torch.device(DEV), max(S, 1) * M * N).fill_(3.0)

        def launch(gw):
            gw.copy_(gw_init(M, N))
            G.wgrad_f8(gw, dy, x, scale(sdy), scale(sx))

        gw = into_frame(launch, M, N, F32)
        X.expect_bits(gw, gw_init(M, N).double() + ref_tn(ddt, E4, M, N, K) * (sdy * sx), f"wgrad_f8 M={M} N={N} K={K}")


# ------------------------------------------------------------------------------------------ fused epilogues
def iso(M, N, K, seed, f8=False, adt=E4):
    """Epilogue-isolating operands as strided views, and the exact product."""
    x, w, sa, sb = X.iso_operands(M, N, K, seed, DEV, f8=f8, adt=adt)
    xs = torch.zeros(M + 1, K + 128, dtype=x.dtype, device=DEV)[1:, 128:]
    ws = torch.zeros(N + 2, K + 256, dtype=w.dtype, device=DEV)[2:, :K]
    xs.copy_(x)
    ws.copy_(w)
    ex = X.exact_nt(xs, ws, 1.0 if not f8 else float(sa) * float(sb))
    assert torch.equal(ex.float().bfloat16().double(), ex)
    return xs, ws, sa, sb, ex


# T: 1 and 24 wrap row % T inside one 16-row block, 100 does not divide the 256 tile rows, 256 is the tile; M = B T:
# 129 (1-row tail past group 0), 264 (8 rows into the second tile), 300 (44), 768 (whole tiles: T = 256 allows no tail)
ROPE_TM = {1: 129, 24: 264, 100: 300, 256: 768}
ROPE_K = {1: 64, 24: 128, 100: 256, 256: 128}


@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("T", [1, 24, 100, 256])
@pytest.mark.parametrize("hd", [32, 64])
def test_rope_epilogue_on_exact_accumulator(hd, T, f8):
    """N = 328 (72-column tail in the second tile column); rope_cols 64 (wave 0 only), 192 (the q|k / v boundary
    between waves 2 and 3 of the first tile), 320 (inside the tail tile, 8 v columns left)."""
    M, N = ROPE_TM[T], 328
    K = max(ROPE_K[T], 128) if f8 else ROPE_K[T]
    x, w, sa, sb, ex = iso(M, N, K, 20 + T, f8)
    cos, sin = ops.rope_cache(T, hd, 10000.0, None, DEV)
    for rc in (64, 192, 320):
        if f8:
            out = into_frame(lambda o: G.gemm_pp_rope_f8(x, w, sa, sb, cos, sin, T, hd, rc, o), M, N)
        else:
            out = into_frame(lambda o: G.gemm_pp_rope(x, w, cos, sin, T, hd, rc, o), M, N)
        note = f"hd={hd} T={T} M={M} rope_cols={rc}"
        X.expect_bits(out[:, rc:], ex[:, rc:], f"rope v columns {note}")
        ref = X.rope(ex, cos, sin, T, hd, rc)
        twin = X.rope_twin(ex, cos, sin, T, hd, rc)
        chk(out[:, :rc], ref[:, :rc], twin[:, :rc], "pp.rope" + (".f8" if f8 else ""), note)


# F: one 8-unit store; 72 = 64 + 8 (past the second 32-unit wave group); one SwiGLU tile; 128 + 8; 128 + 72;
# 2 x 128 + 8.  M: one 16-row block; 128 + 1; 256 + 44
SW_F = [8, 72, 128, 136, 200, 264]
SW_M = [16, 129, 300]
SW_K = {8: 64, 72: 128, 128: 256, 136: 64, 200: 128, 264: 256}


def _swiglu_fwd(kind, x, w, sa, sb, M, F, q=None):
    """(gu | [A | B], act) of the forward in its framed outputs; kind 'q': act as e4m3 bytes and amax."""
    bgu, gu = framed(M, 2 * F, BF16)
    if kind == "q":
        b8, act = frame8(M, F, E4)
        qs, amax = q
        G.gemm_pp_swiglu_f8q(x, w, sa, sb, qs, amax, gu, act)
    else:
        bact, act = framed(M, F, BF16)
        if kind == "bf16":
            G.gemm_pp_swiglu(x, w, gu, act)
        else:
            G.gemm_pp_swiglu_f8(x, w, sa, sb, gu, act)
    torch.cuda.synchronize()
    assert_frame_intact(bgu, gu)
    if kind == "q":
        frame8_intact(b8, M, F)
    else:
        assert_frame_intact(bact, act)
    return gu, act


@pytest.mark.parametrize("kind", ["bf16", "f8", "q"])
@pytest.mark.parametrize("form", [0, 1])
def test_swiglu_forward_on_exact_gate_up(form, kind):
    G.set_mlp_coef(form)
    tag = ".f8" if kind != "bf16" else ""
    for F in SW_F:
        for M in SW_M:
            K = max(SW_K[F], 128) if kind != "bf16" else SW_K[F]
            x, w, sa, sb, ex = iso(M, 2 * F, K, 40 + F, kind != "bf16")
            note = f"form={form} M={M} F={F} K={K}"
            gu, act = _swiglu_fwd("f8" if kind == "q" else kind, x, w, sa, sb, M, F)
            if form == 0:
                X.expect_bits(gu, ex, f"swiglu gu {note}")
            else:
                chk(gu, X.swiglu_coef(ex), X.swiglu_coef_twin(ex), "pp.swiglu.coef" + tag, note)
            chk(act, X.swiglu_act(ex), X.swiglu_act_twin(ex), "pp.swiglu.act" + tag, note)
            if kind == "q":
                qs, amax = scale(32.0), torch.zeros(64, device=DEV)
                gu2, act8 = _swiglu_fwd("q", x, w, sa, sb, M, F, (qs, amax))
                assert torch.equal(gu2, gu), note
                assert torch.equal(act8.view(torch.uint8), fp8.cast(act.contiguous(), qs, 0).view(torch.uint8)), note
                assert amax.max().item() == act.float().abs().max().item(), note


@pytest.mark.parametrize("variant", [512, 1024, 2048, 2080])
@pytest.mark.parametrize("form", [0, 1])
def test_swiglu_forward_store_variants_bitwise(form, variant):
    """The SwiGLU forward under its store-policy / staging A/B builds is bitwise the default kernel (and exact)."""
    G.set_mlp_coef(form)
    for M, F in [(300, 136), (129, 264)]:
        x, w, sa, sb, ex = iso(M, 2 * F, SW_K[F], 40 + F)
        gu0, act0 = _swiglu_fwd("bf16", x, w, sa, sb, M, F)
        assert G.set_pp_variant(variant) == 0, f"variant {variant} is not in this build"
        try:
            gu1, act1 = _swiglu_fwd("bf16", x, w, sa, sb, M, F)
        finally:
            assert G.set_pp_variant(0) == variant
        assert torch.equal(gu1, gu0) and torch.equal(act1, act0), (variant, M, F)
        if form == 0:
            X.expect_bits(gu1, ex, f"swiglu gu variant {variant} M={M} F={F}")


def _saved(M, F, seed):
    """Random bf16 saved tensor [M, 2F] (gate | up, or [A | B]) as a strided view."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.randn(M, 2 * F + 64, device=DEV, generator=g).bfloat16()
    return buf[:, 32:32 + 2 * F]


@pytest.mark.parametrize("kind", ["bf16", "e5m2", "e4m3", "q"])
@pytest.mark.parametrize("form", [0, 1])
def test_swiglu_backward_on_exact_dact(form, kind):
    """d(act) = dy . w_down^T is exact and never rounded; the oracle is d(act) times the float64 coefficient of the
    bf16 saved tensor that is actually passed in."""
    G.set_mlp_coef(form)
    f8 = kind != "bf16"
    adt = E4 if kind == "e4m3" else E5
    tag = ".f8" if f8 else ""
    for F in SW_F:
        for M in SW_M:
            K = max(SW_K[F], 128) if f8 else SW_K[F]
            dy, wdt, sa, sb, dact = iso(M, F, K, 60 + F, f8, adt)
            saved = _saved(M, F, 7 * F + M)
            note = f"form={form} M={M} F={F} K={K}"
            if f8:
                dgu = into_frame(lambda o: G.gemm_pp_dswiglu_f8(dy, wdt, sa, sb, saved, o), M, 2 * F)
            else:
                dgu = into_frame(lambda o: G.gemm_pp_dswiglu(dy, wdt, saved, o), M, 2 * F)
            chk(dgu, X.dswiglu(dact, saved, form), X.dswiglu_twin(dact, saved, form), "pp.dswiglu" + tag, note)
            if kind == "q":
                qs, amax = scale(64.0), torch.zeros(64, device=DEV)
                b8, d8 = frame8(M, 2 * F, E5)
                G.gemm_pp_dswiglu_f8q(dy, wdt, sa, sb, saved, qs, amax, d8)
                torch.cuda.synchronize()
                frame8_intact(b8, M, 2 * F)
                assert torch.equal(d8.view(torch.uint8), fp8.cast(dgu.contiguous(), qs, 1).view(torch.uint8)), note
                assert amax.max().item() == dgu.float().abs().max().item(), note


@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
def test_saved_form_round_trip(f8):
    """Forward form 1 -> backward form 1 against form 0 -> form 0 at the tail shapes, per element.  Both are held to
    the true gradient ref = d(act) * coefficient(exact gate | up) in float64.  Form 0 rounds once (its store):
    bound0 = 2^-8 |ref| + slack.  Form 1 rounds twice (the stored coefficient, then its store):
    bound1 = (2 * 2^-8 + 2^-16) |ref| + slack + |d(act)| * slack of the coefficient.  The two outputs differ by at
    most bound0 + bound1."""
    margin = o64.MARGIN
    h = o64.BF16_HALF_ULP
    for F in (72, 136, 264):
        for M in (129, 300):
            K = max(SW_K[F], 128) if f8 else SW_K[F]
            x, w, sa, sb, gu_ex = iso(M, 2 * F, K, 40 + F, f8)
            dy, wdt, sd, sw, dact = iso(M, F, K, 60 + F, f8, E5)
            outs = {}
            for form in (0, 1):
                G.set_mlp_coef(form)
                kind = "f8" if f8 else "bf16"
                saved, _ = _swiglu_fwd(kind, x, w, sa, sb, M, F)
                if f8:
                    outs[form] = into_frame(lambda o: G.gemm_pp_dswiglu_f8(dy, wdt, sd, sw, saved, o), M, 2 * F)
                else:
                    outs[form] = into_frame(lambda o: G.gemm_pp_dswiglu(dy, wdt, saved, o), M, 2 * F)
            ref = X.dswiglu(dact, gu_ex.float().bfloat16(), 0)
            slack = margin * (X.dswiglu_twin(dact, gu_ex.float().bfloat16(), 0).double() - ref).abs().max().item()
            slack_c = margin * (X.swiglu_coef_twin(gu_ex).double() - X.swiglu_coef(gu_ex)).abs().max().item()
            d2 = torch.cat([dact, dact], 1).abs()
            bound = (h * ref.abs() + slack) + ((2 * h + h * h) * ref.abs() + slack + d2 * slack_c)
            err = (outs[1].double() - outs[0].double()).abs()
            bad = ~(err <= bound)
            assert not bool(bad.any()), (f"M={M} F={F}: {int(bad.sum())} elements; worst excess "
                                         f"{(err - bound).max().item():.3e}")


# ------------------------------------------------------------------------------------------ Gaussian, per element
GAUSS_MN = [(257, 264), (300, 520)]


def _spiked_pair(M, N, K, dt_a=BF16, dt_b=BF16):
    a = o64.spiked(M, K, DEV)
    b = o64.spiked(N, K, DEV, scale=0.05, start=3)
    if dt_a == BF16:
        return a.bfloat16(), b.bfloat16(), 1.0, 1.0

    def q(x, dt):  # per-tensor current scaling to half the format's range, power-of-two scale
        fmax = 448.0 if dt == E4 else 57344.0
        s = 2.0 ** torch.floor(torch.log2(fmax / x.abs().amax() / 2)).item()
        return (x * s).to(dt), 1.0 / s

    a8, sa = q(a, dt_a)
    b8, sb = q(b, dt_b)
    return a8, b8, sa, sb


@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("kind", ["pp", "w128", "e4m3", "e5m2"])
def test_gaussian_nt_per_element(kind, K):
    """The accumulator's own rounding: spiked Gaussian operands (a dropped chunk meets a large value), the float64
    product of the operands as the kernel sees them (fp8: dequantised), slack from the fp32 torch twin."""
    f8 = kind in ("e4m3", "e5m2")
    for M, N in GAUSS_MN:
        a, b, sa, sb = _spiked_pair(M, N, K, {"e4m3": E4, "e5m2": E5}.get(kind, BF16), E4 if f8 else BF16)
        ref = X.exact_nt(a, b, sa * sb)
        twin = (a.float() @ b.float().t()) * (sa * sb)
        if f8:
            tsa, tsb = scale(sa), scale(sb)
            out = into_frame(lambda o: G.gemm_pp_f8(a, b, tsa, tsb, o), M, N)
        else:
            out = into_frame(lambda o: (G.gemm_pp if kind == "pp" else G.gemm_w128)(a, b, o), M, N)
        chk(out, ref, twin, {"pp": "pp.gauss", "w128": "w128.gauss"}.get(kind, "pp_f8.gauss"), f"M={M} N={N} K={K}")


@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("kind", ["bf16", "e5m2", "e4m3"])
def test_gaussian_wgrad_per_element(kind, K):
    """fp32 outputs: rel = 0, the whole bound is the slack from the fp32 torch twin."""
    f8 = kind != "bf16"
    for M, N in [(264, 520), (520, 1032)] if not f8 else [(272, 528), (512, 1024)]:
        dy, x, sdy, sx = _spiked_pair(M, N, K, {"e4m3": E4, "e5m2": E5}.get(kind, BF16), E4 if f8 else BF16)
        dy, x = dy.t().contiguous(), x.t().contiguous()  # [K, M], [K, N]: the spikes walk along the token axis
        gw0 = torch.randn(M, N, device=DEV)
        ref = X.exact_tn(dy, x, gw0, sdy * sx)
        twin = gw0 + (dy.float().t() @ x.float()) * (sdy * sx)

        def launch(gw):
            gw.copy_(gw0)
            if f8:
                G.wgrad_f8(gw, dy, x, scale(sdy), scale(sx))
            else:
                G.wgrad(gw, dy, x)

        gw = into_frame(launch, M, N, F32)
        chk(gw, ref, twin, "wgrad_f8.gauss" if f8 else "wgrad.gauss", f"M={M} N={N} K={K}")
