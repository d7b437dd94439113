"""``ops.gemv_w8`` (csrc/gemv_w8.hip) on the MI355X.  (8, 128): one group on one wave, N below a tile; (40, 384): an N
tail, three groups on three of the four waves (the K split through LDS); (272, 2688): 21 groups, the most in configs/,
in 6 workgroup slices, the last of one group (the K split through the workspace)."""
import pytest
import torch

from nanodiloco_amd import ops
from nanodiloco_amd.ops import gemv

from . import _gemm_exact as ge
from . import _oracle64 as o64
from ._frames import assert_frame_intact, framed_flat

pytestmark = pytest.mark.gpu
DEV, BF16, REPORT = "cuda", torch.bfloat16, {}
MS, SHAPES = (1, 3, 16), ((8, 128), (40, 384), (272, 2688))


@pytest.fixture(autouse=True)
def _hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.set_backend("hip")
    yield
    ops.set_backend("auto")


@pytest.fixture(scope="module", autouse=True)
def _slack_report():
    yield
    print("".join(f"\n[slack] {k}: needs margin {REPORT[k]:.3g} (allowed {o64.MARGIN})" for k in sorted(REPORT)))


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", MS)
def test_exact(M, N, K):
    # x in [-4, 4], codes in [-8, 8], exponents in [-2, 2]: every partial sum is a multiple of 1/4 below 2^24
    assert 4 * ge.exact_bound(K, 4, 8 * 4) < ge.EXACT_LIMIT
    x = ge.int_operand(M, K, -4, 4, BF16, 1, DEV)
    codes = ge.int_operand(N, K, -8, 8, ge.E4, 2, DEV).view(torch.uint8)
    exps = torch.randint(-2, 3, (N, K // 128), generator=torch.Generator().manual_seed(3)).to(torch.int8).to(DEV)
    big, flat = framed_flat(M * N, BF16)
    out = gemv.gemv_w8(x, codes, exps, out=flat.view(M, N))
    ge.expect_bits(out, ge.exact_nt(x, gemv.dequantize_weight(codes, exps)), name=f"gemv_w8 {M}x{N}x{K}")
    assert_frame_intact(big, flat)


def _edge_weight(N, K):
    """A quantised normal weight with the edges on channels of their own: 0 a zero group, 1 codes +-448, 2 / 3 every
    exponent 100 / -100 (outputs near 2^+-100, finite: checked as columns of their own, not to set the others' slack)."""
    codes, exps = gemv.quantize_weight(torch.randn(N, K, device=DEV) * 0.02)
    codes[0, :128], exps[0, 0] = 0, 0
    codes[1, K - 128:K:7], codes[1, K - 127:K:7] = 0x7e, 0xfe
    exps[2], exps[3] = 100, -100
    return codes, exps


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", MS)
def test_against_float64(M, N, K):
    torch.manual_seed(M * 1000 + N)
    x = o64.spiked(M, K, DEV).bfloat16()
    codes, exps = _edge_weight(N, K)
    Wd = gemv.dequantize_weight(codes, exps)
    out = gemv.gemv_w8(x, codes, exps)
    ref, twin = x.double() @ Wd.double().T, x.float() @ Wd.float().T
    rest = [c for c in range(N) if c not in (2, 3)]
    for name, cols in (("gemv_w8.exp+100", [2]), ("gemv_w8.exp-100", [3]), ("gemv_w8", rest)):
        o64.check(out[:, cols], ref[:, cols], twin[:, cols], name=name, report=REPORT, note=f"M {M} N {N} K {K}")


def test_nan_code_propagates():
    x = torch.ones(3, 256, dtype=BF16, device=DEV)
    codes, exps = gemv.quantize_weight(torch.randn(20, 256, device=DEV))
    codes[17, 200] = 0x7f
    nan = torch.isnan(gemv.gemv_w8(x, codes, exps))
    assert bool(nan[:, 17].all()) and int(nan.sum()) == 3


@pytest.mark.parametrize("N,K", SHAPES)
def test_row_invariance(N, K):
    torch.manual_seed(N)
    x = o64.spiked(16, K, DEV).bfloat16()
    codes, exps = gemv.quantize_weight(torch.randn(N, K, device=DEV) * 0.02)
    full = gemv.gemv_w8(x, codes, exps)
    for i in (0, 6, 15):
        one = gemv.gemv_w8(x[i:i + 1], codes, exps)
        three = gemv.gemv_w8(torch.stack([x[(i + 5) % 16], x[(i + 9) % 16], x[i]]), codes, exps)
        assert torch.equal(full[i].view(torch.int16), one[0].view(torch.int16)), (i, "M = 1")
        assert torch.equal(full[i].view(torch.int16), three[2].view(torch.int16)), (i, "M = 3, row 2")
